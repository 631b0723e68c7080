"""Dyadic-lattice ReLU networks for the field kernels, with their float64 reference.

The kernels take the activation as a run-time switch, so a ReLU network without positional encoding runs the same GEMMs,
stash layouts, hand-overs, split sums and fold / unfold kernels as the Siren one.  On such a network every operand can be
put on a dyadic lattice: every unit u of the network carries a LEVEL e_u (an integer), every weight between two units is
+-2^(e_out - e_in) in +-{1/4, 1/2, 1, 2}, every bias of unit u is 2^e_u Q0 times a small integer (Q0 = 1/8, the quantum of
the inputs).  Every forward value of unit u is then 2^e_u Q0 times an integer, every backward value 2^-e_u times an
integer multiple of the seeds' quantum, WHATEVER path it took - so a sum over paths adds integers and stays short.  The
builder keeps those integers below 2^7 (bf16 holds 8 significant bits) by choosing, row by row, among seeded random
candidates; nothing is random at run time and the same name always gives the same network.

Deviations from a literal "one or two non-zeros per row", and why:
  * the rows of the <= 3-row matrices (sigma_from_xyz, grad_from_xyz, every head's second layer) carry NARROW_NNZ = 4
SIGMA_NNZ = 8             # the sigma row starts the adjoint chain: with four columns most points have d sigma / d xyz = 0
    non-zeros (sigma_from_xyz: SIGMA_NNZ = 8) in columns no other row of the matrix uses: with two, an output would see two hidden units out of up to 512;
  * a head's first layer has F/2 rows for F (+ direction / embedding) input columns: every row carries two feature
    columns (two halves of one permutation, so all F are used) and the first rows a third, the extra input's.
feats_from_xyz is one-sparse per row (a signed, scaled permutation), so the folded product head.0.weight[:, :F] @
feats.weight has at most two non-zeros per row, each a power of two.

The float64 reference is oracle/field.py on these parameters (oracle_out, oracle_grads: autograd for the gradients).
forward_book / backward_chains carry the bookkeeping of the chains the kernels run (csrc/field_adjoint.hip,
field_bwd.hip, field_adjbwd.hip: every layer's pre-activation, mask and activation, a', delta', dz, gbar', abar', dbar'),
restated in float64 - on the lattice that arithmetic is exact - and tied to autograd by tests/test_lattice_cpu.py."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle.config import FieldConfig
from oracle import field as OF

Q0 = 0.125                 # quantum of xyz, directions and embeddings
LEVELS = (-2, -1, 0)       # levels of hidden units, feature units and outputs (the inputs sit at level 0)
INT_MAX = 127              # |value| / (2^level Q0) of every pre-activation over the case's points
NARROW_NNZ = 4
SIGMA_NNZ = 8             # the sigma row starts the adjoint chain: with four columns most points have d sigma / d xyz = 0
HEAD_Z_MAX = 2.0           # |pre-activation| of every sigmoid / softplus output and of sigma_raw (keeps act' away from 0)
NLR_INT_MAX = 15           # |learned-normal pre-activation| / quantum: four significant bits
U24 = 2.0 ** -24
FP32_EPS = OF.FP32_EPS
N_MAX = 1100

_RPV = dict(funcM=1, funcF=1, funcH=1)
# name -> (FieldConfig arguments, forward flags, seed, point counts)
CASES = {
    "lambert_F64_L8": (dict(feat=64, layers=8), dict(), 1, (1, 63, 65, 257, 600, 1100)),
    "rpv_an_F128_L4": (dict(feat=128, layers=4, normal="analystic", **_RPV), dict(apply_brdf=True, nr_an_on=True), 2, (1, 65, 257, 1100)),
    "rpv_anlr_F256_L8": (dict(feat=256, layers=8, normal="analystic_learned", **_RPV),
                         dict(apply_brdf=True, nr_an_on=True, nr_lr_on=True), 3, (63, 600)),
    "rpv_an_F512_L8": (dict(feat=512, layers=8, normal="analystic", **_RPV), dict(apply_brdf=True, nr_an_on=True), 4, (65, 600)),
    "viewdir_beta_F192_L8": (dict(feat=192, layers=8, input_viewdir=1, beta=True), dict(), 5, (65, 257, 1100)),
}


def case_sizes():
    return [(n, B) for n, (_, _, _, sizes) in CASES.items() for B in sizes]


# ------------------------------------------------------------------------------------------------ builder
def _pow2(e):
    return np.ldexp(1.0, np.asarray(e, dtype=np.int64))


class _Builder:
    def __init__(self, cfg, seed):
        self.cfg, self.rng = cfg, np.random.default_rng(1000 + seed)
        self.params, self.levels = {}, {}

    def _row_level(self, col_levels):
        lo = max(min(LEVELS), max(col_levels) - 2)
        hi = min(max(LEVELS), min(col_levels) + 1)
        assert lo <= hi
        return int(self.rng.integers(lo, hi + 1))

    def _dense(self, name, V, lev, cols_of_row, mixed=True, z_max=None, int_max=INT_MAX, level=None):
        """One lattice matrix + bias.  V (N, K) float64: the layer's input over the case's points; lev (K,) the input
        columns' levels; cols_of_row: per output row the list of its non-zero columns.  Signs, level and bias of a row
        are drawn until the row's pre-activation over the points is inside its range and (mixed) its ReLU mask is mixed."""
        rng, R, K = self.rng, len(cols_of_row), V.shape[1]
        W, b, out_lev = np.zeros((R, K)), np.zeros(R), np.zeros(R, dtype=np.int64)
        Z = np.zeros((V.shape[0], R))
        for n, cols in enumerate(cols_of_row):
            cols = np.asarray(cols)
            best = None
            for attempt in range(64):
                e = self._row_level(lev[cols]) if level is None else level
                w = rng.choice([-1.0, 1.0], size=len(cols)) * _pow2(e - lev[cols])
                pre = V[:, cols] @ w
                q = 2.0 ** e * Q0
                frac = rng.uniform(0.35, 0.75) if mixed else 0.5
                bias = -np.round(np.quantile(pre, frac) / q) * q + (0.0 if mixed else q * rng.integers(-1, 2))
                z = pre + bias
                on = float((z > 0).mean())
                big = float(np.abs(z).max())
                ok = big <= (z_max if z_max is not None else int_max * q) and big <= int_max * q and float(z.max()) > float(z.min())
                if mixed:
                    ok = ok and 0.2 <= on <= 0.8
                score = (not ok, big / q)
                if best is None or score < best[0]:
                    best = (score, e, w, bias, z)
                if ok:
                    break
            if best[0][0]:
                raise RuntimeError(f"{name} row {n}: no candidate on the lattice")
            _, e, w, bias, z = best
            W[n, cols], b[n], out_lev[n], Z[:, n] = w, bias, e, z
        self.params[name + ".weight"], self.params[name + ".bias"] = W, b
        self.levels[name] = out_lev
        return Z, out_lev

    def _disjoint_rows(self, R, K, nnz, forced=()):
        """R rows of nnz columns each, no column twice; the `forced` columns are dealt to the rows first."""
        rows = [[int(c) for c in forced[r::R]] for r in range(R)]
        rest = [int(c) for c in self.rng.permutation(K) if c not in set(forced)]
        for r in range(R):
            while len(rows[r]) < nnz:
                rows[r].append(rest.pop())
        return rows


def _build(name):
    kw, flags, seed, sizes = CASES[name]
    cfg = FieldConfig(siren=False, mapping=False, **kw)
    for attempt in range(50):
        try:
            return _build_once(name, cfg, flags, sizes, 97 * seed + attempt)
        except RuntimeError:
            continue
    raise RuntimeError(f"{name}: no lattice network found")


def _build_once(name, cfg, flags, sizes, seed):
    bd = _Builder(cfg, seed)
    rng, F, L = bd.rng, cfg.feat, cfg.layers
    skip = cfg.skips[0] if cfg.skips and 0 < cfg.skips[0] < L else -1
    xyz = rng.integers(-8, 9, size=(N_MAX, 3)) * Q0
    dirs = rng.integers(-4, 5, size=(N_MAX, 3)) * (2 * Q0) if cfg.dir_dim else None
    t = rng.integers(-4, 5, size=(N_MAX, cfg.t_dim)) * (2 * Q0) if cfg.beta else None
    lev_x = np.zeros(3, dtype=np.int64)

    h, lev = xyz, lev_x
    for l in range(L):
        if l == skip:
            h, lev = np.concatenate([xyz, h], 1), np.concatenate([lev_x, lev])
        K = h.shape[1]
        rows = []
        if l == 0:
            for n in range(F):
                c = [n % 3]
                if rng.random() < 0.5:
                    c.append(int((n + 1 + rng.integers(0, 2)) % 3))
                rows.append(c)
        else:
            off = K - F                                  # 3 at the skip layer: the hidden columns come after xyz
            p1, p2 = rng.permutation(F), rng.permutation(F)
            for n in range(F):
                c = [off + int(p1[n])]
                if off and n < F // 4:
                    c.append(n % 3)                      # the skip layer's input part
                elif rng.random() < 0.5 and p2[n] != p1[n]:
                    c.append(off + int(p2[n]))
                rows.append(c)
        z, e = bd._dense(f"fc_net.{2*l}", h, lev, rows)
        h, lev = np.maximum(z, 0.0), e
    yL, levL = h, lev

    used = rng.permutation(F)                            # disjoint column sets for the narrow rows that read y_L
    sig_cols = [list(used[:SIGMA_NNZ])]
    bd._dense("sigma_from_xyz.0", yL, levL, sig_cols, mixed=False, z_max=HEAD_Z_MAX)
    if cfg.normal in ("learned", "analystic_learned"):
        nlr_cols = [list(used[SIGMA_NNZ + NARROW_NNZ * r:SIGMA_NNZ + NARROW_NNZ * (r + 1)]) for r in range(3)]
        bd._dense("grad_from_xyz", yL, levL, nlr_cols, mixed=False, int_max=NLR_INT_MAX)
    # feats: a signed, scaled permutation (one-sparse: the folded first layers stay two-sparse powers of two)
    pf = rng.permutation(F)
    Wf, bf, levf = np.zeros((F, F)), np.zeros(F), np.zeros(F, dtype=np.int64)
    for n in range(F):
        e = bd._row_level(levL[[pf[n]]])
        Wf[n, pf[n]] = rng.choice([-1.0, 1.0]) * 2.0 ** (e - levL[pf[n]])
        bf[n], levf[n] = 2.0 ** e * Q0 * rng.integers(-2, 3), e
    bd.params["feats_from_xyz.weight"], bd.params["feats_from_xyz.bias"] = Wf, bf
    feats = yL @ Wf.T + bf

    heads = [("rgb_from_xyzdir", 3, dirs)]
    if cfg.beta:
        heads.append(("beta_from_xyz", 1, t))
    heads += [(h_, cfg.dim_RPV, None) for h_ in cfg.brdf_head_names(flags.get("apply_brdf", False), False)]
    for hname, nout, extra in heads:
        vin, lin = feats, levf
        if extra is not None:
            vin, lin = np.concatenate([feats, extra], 1), np.concatenate([levf, np.zeros(extra.shape[1], dtype=np.int64)])
        p = rng.permutation(F)
        rows = [[int(p[n]), int(p[F // 2 + n])] + ([F + n] if extra is not None and n < extra.shape[1] else []) for n in range(F // 2)]
        z, e = bd._dense(f"{hname}.0", vin, lin, rows)
        forced = list(range(extra.shape[1])) if extra is not None else []      # the hidden units that read the extra input reach an output
        bd._dense(f"{hname}.2", np.maximum(z, 0.0), e, bd._disjoint_rows(nout, F // 2, NARROW_NNZ, forced), mixed=False, z_max=HEAD_Z_MAX)

    want = [k for k, _, _ in cfg.param_shapes()]
    assert set(want) == set(bd.params), sorted(set(want) ^ set(bd.params))
    params = {k: torch.from_numpy(np.ascontiguousarray(bd.params[k], dtype=np.float64)) for k in want}
    for k, shape, _ in cfg.param_shapes():
        assert tuple(params[k].shape) == tuple(shape), (k, tuple(params[k].shape), shape)
    tt = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    case = SimpleNamespace(name=name, cfg=cfg, flags=dict(flags), sizes=tuple(sizes), params=params, pts=(tt(xyz), tt(dirs), tt(t)),
                           skip=skip, heads=[(h_, n_) for h_, n_, _ in heads], levels=bd.levels, seed=seed)
    _choose_seeds(case, rng)
    return case


_CASES = {}


def get_case(name):
    if name not in _CASES:
        _CASES[name] = _build(name)
    return _CASES[name]


def state_dict32(case):
    """The parameters as the module loads them (fp32: every lattice value is exact there)."""
    return {k: v.float() for k, v in case.params.items()}


def take(pts, B):
    return tuple(None if a is None else a[:B].contiguous() for a in pts)


# ------------------------------------------------------------------------------------------------ channels
def channels(case):
    """Output channel layout [(kind, head or None, first column, width)] in the forward's order."""
    cfg, out, c = case.cfg, [], 0
    out.append(("sigmoid", "rgb_from_xyzdir", 0, 3)); c = 3
    out.append(("sigma", None, 3, 1)); c = 4
    if cfg.beta:
        out.append(("softplus", "beta_from_xyz", c, 1)); c += 1
    if case.flags.get("nr_an_on"):
        out.append(("normal_an", None, c, 3)); c += 3
    if case.flags.get("nr_lr_on"):
        out.append(("normal_lr", None, c, 3)); c += 3
    for h in cfg.brdf_head_names(case.flags.get("apply_brdf", False), False):
        kind = {"k_from_xyz": "rpv_k", "theta_rpv_from_xyz": "rpv_theta"}.get(h, "tile3")
        out.append((kind, h, c, 3)); c += 3
    return out, c


# ------------------------------------------------------------------------------------------------ float64 chains
def forward_book(case, B, params=None):
    """Float64 forward of the first B points with every layer's input, pre-activation, mask and activation, the heads'
    hidden layers, and the adjoint chain a', delta', g' (field_adjoint.hip: seeded with w_sigma alone)."""
    p = case.params if params is None else params
    cfg, L, F, skip = case.cfg, case.cfg.layers, case.cfg.feat, case.skip
    xyz, dirs, t = take(case.pts, B)
    bk = SimpleNamespace(xyz=xyz, dirs=dirs, t=t, ins=[], z=[], D=[], y=[])
    h = xyz
    for l in range(L):
        if l == skip:
            h = torch.cat([xyz, h], 1)
        bk.ins.append(h)
        z = h @ p[f"fc_net.{2*l}.weight"].T + p[f"fc_net.{2*l}.bias"]
        bk.z.append(z); bk.D.append((z > 0).double())
        h = torch.relu(z)
        bk.y.append(h)
    yL = h
    ws = p["sigma_from_xyz.0.weight"]
    bk.sraw = (yL @ ws.T + p["sigma_from_xyz.0.bias"])[:, 0]
    bk.sp = torch.sigmoid(bk.sraw)
    bk.feats = yL @ p["feats_from_xyz.weight"].T + p["feats_from_xyz.bias"]
    bk.head_in, bk.head_z1, bk.head_D, bk.head_g, bk.head_z2 = {}, {}, {}, {}, {}
    for hname, _ in case.heads:
        vin = bk.feats
        if hname == "rgb_from_xyzdir" and dirs is not None:
            vin = torch.cat([bk.feats, dirs], 1)
        if hname == "beta_from_xyz":
            vin = torch.cat([bk.feats, t], 1)
        z1 = vin @ p[f"{hname}.0.weight"].T + p[f"{hname}.0.bias"]
        g = torch.relu(z1)
        bk.head_in[hname], bk.head_z1[hname], bk.head_D[hname], bk.head_g[hname] = vin, z1, (z1 > 0).double(), g
        bk.head_z2[hname] = g @ p[f"{hname}.2.weight"].T + p[f"{hname}.2.bias"]
    if "grad_from_xyz.weight" in p:
        bk.nraw = yL @ p["grad_from_xyz.weight"].T + p["grad_from_xyz.bias"]
    # adjoint chain on a' = a / s'
    a = ws.expand(B, F)
    bk.adj_a, bk.adj_delta = [None] * L, [None] * L
    gp = torch.zeros(B, 3, dtype=torch.float64)
    for l in reversed(range(L)):
        bk.adj_a[l] = a
        delta = a * bk.D[l]
        bk.adj_delta[l] = delta
        back = delta @ p[f"fc_net.{2*l}.weight"]
        if l == skip:
            gp, a = gp + back[:, :3], back[:, 3:]
        elif l == 0:
            gp = gp + back
        else:
            a = back
    bk.gprime = gp
    return bk


def backward_chains(case, bk, seeds, absolute=False, params=None):
    """The parameter gradients from pre-activation seeds, as the kernels form them (field_bwd.hip, field_adjbwd.hip,
    the weight-gradient jobs, bn_unfold_heads), in float64.  seeds: 'heads' {name: (B, nout)}, 'sraw' (B,), 'nlr' (B, 3)
    or None, 'gbar' (B, 3) or None (gbar' = s' gbar, the adjoint backward's seed).  absolute=True: the same sums over
    |seeds|, |W|, |y| with the masks unchanged - the sum of the absolute contributions to every gradient element.
    Also returns the bookkeeping: dz per layer, the heads' dG, gbar', abar', dbar'."""
    p = case.params if params is None else params
    ab = (lambda v: v.abs()) if absolute else (lambda v: v)
    cfg, L, F, skip = case.cfg, case.cfg.layers, case.cfg.feat, case.skip
    B = bk.xyz.shape[0]
    G = {}
    yL = ab(bk.y[-1])
    dfe = torch.zeros(B, F, dtype=torch.float64)
    book = SimpleNamespace(dG={}, dz=[None] * L, abar=[None] * (L + 1), dbar=[None] * L)
    adj_jobs, sbar = {}, torch.zeros(B, dtype=torch.float64)
    if seeds.get("gbar") is not None:
        gb = ab(seeds["gbar"])
        book.gbar = gb
        abar = None
        for l in range(L):
            W = ab(p[f"fc_net.{2*l}.weight"])
            inb = gb if l == 0 else (torch.cat([gb, abar], 1) if l == skip else abar)
            adj_jobs[l] = ab(bk.adj_delta[l]).T @ inb
            dbar = inb @ W.T
            book.dbar[l] = dbar
            abar = dbar * bk.D[l]
            book.abar[l + 1] = abar
        adj_jobs["sigma"] = abar.sum(0, keepdim=True)
        # sbar = (w_sigma . abar'_L)(1 - s'): exactly 0 on the lattice (gbar' . g' = 0); its absolute terms are not
        sbar = (abar @ ab(p["sigma_from_xyz.0.weight"]).T)[:, 0] * (1 - bk.sp)
    book.sbar = sbar
    for hname, _ in case.heads:
        sd = ab(seeds["heads"][hname])
        W1, W2 = ab(p[f"{hname}.0.weight"]), ab(p[f"{hname}.2.weight"])
        G[f"{hname}.2.weight"], G[f"{hname}.2.bias"] = sd.T @ ab(bk.head_g[hname]), sd.sum(0)
        dG = (sd @ W2) * bk.head_D[hname]
        book.dG[hname] = dG
        G[f"{hname}.0.weight"], G[f"{hname}.0.bias"] = dG.T @ ab(bk.head_in[hname]), dG.sum(0)
        dfe = dfe + dG @ W1[:, :F]
        if hname == "beta_from_xyz":
            G["d_t_embed"] = dG @ W1[:, F:]
    G["feats_from_xyz.weight"], G["feats_from_xyz.bias"] = dfe.T @ yL, dfe.sum(0)
    dy = dfe @ ab(p["feats_from_xyz.weight"])
    ds = ab(seeds["sraw"]) + sbar
    ws = ab(p["sigma_from_xyz.0.weight"])
    G["sigma_from_xyz.0.weight"], G["sigma_from_xyz.0.bias"] = ds[None, :] @ yL, ds.sum().reshape(1)
    if "sigma" in adj_jobs:
        G["sigma_from_xyz.0.weight"] = G["sigma_from_xyz.0.weight"] + adj_jobs["sigma"]
    dy = dy + ds[:, None] * ws
    book.noisy = ds[:, None] * ws                      # fp32 terms of dy_L (not yet rounded to 16 bits when they are added)
    if seeds.get("nlr") is not None:
        dn = ab(seeds["nlr"])
        Wg = ab(p["grad_from_xyz.weight"])
        G["grad_from_xyz.weight"], G["grad_from_xyz.bias"] = dn.T @ yL, dn.sum(0)
        dy = dy + dn @ Wg
        book.noisy = book.noisy + dn @ Wg
    book.dyL = dy
    for l in reversed(range(L)):
        W = ab(p[f"fc_net.{2*l}.weight"])
        dz = dy * bk.D[l]
        book.dz[l] = dz
        G[f"fc_net.{2*l}.weight"], G[f"fc_net.{2*l}.bias"] = dz.T @ ab(bk.ins[l]), dz.sum(0)
        if l in adj_jobs:
            G[f"fc_net.{2*l}.weight"] = G[f"fc_net.{2*l}.weight"] + adj_jobs[l]
        back = dz @ W
        dy = back[:, 3:] if l == skip else back
    return G, book


def oracle_out(case, B, params=None, t_in=None, sigma_only=False):
    p = case.params if params is None else params
    xyz, dirs, t = take(case.pts, B)
    out = OF.field_forward(p, case.cfg, xyz, dirs=dirs, t_embed=t if t_in is None else t_in, sigma_only=sigma_only, **case.flags)
    return out if params is not None else out.detach()


def reference_out(case, B, bk=None):
    """oracle/field.py's float64 output with the analytic-normal channels taken from the restated chain, -normalize(s' g'):
    autograd sums s' times every path, so a component whose paths cancel comes out as 1e-16 instead of the lattice's exact
    0 (the two agree to float64 rounding: tests/test_lattice_cpu.py)."""
    out = oracle_out(case, B).clone()
    if case.flags.get("nr_an_on"):
        bk = forward_book(case, B) if bk is None else bk
        c0 = [c for k, _, c, _ in channels(case)[0] if k == "normal_an"][0]
        out[:, c0:c0 + 3] = -OF.l2_normalize(bk.gprime * bk.sp[:, None])
    return out


def oracle_grads(case, B, coef):
    """d sum(out * coef) / d parameter by autograd through oracle/field.py in float64 (+ 'd_t_embed' with --beta)."""
    p = {k: v.clone().requires_grad_(True) for k, v in case.params.items()}
    t_in = None
    if case.cfg.beta:
        t_in = take(case.pts, B)[2].clone().requires_grad_(True)
    out = oracle_out(case, B, p, t_in)
    leaves = list(p.values()) + ([t_in] if t_in is not None else [])
    gr = torch.autograd.grad((out * coef).sum(), leaves, allow_unused=True)
    G = {k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(p.items(), gr)}
    if t_in is not None:
        G["d_t_embed"] = gr[-1]
    return G


# ------------------------------------------------------------------------------------------------ seeds and d_out
def _perp(g):
    """Per row of the integer-valued (B, 3) array g: a small integer vector q with q . g == 0 exactly, q_c != 0 wherever
    g_c != 0 (an exactly zero component would be filled with the rounding noise of g . dn in the kernel's seed line),
    smallest max |q_c| first.  Rows without one inside [-7, 7]^3 (and rows g == 0: any q, here (1, -2, 3)) are flagged."""
    r = np.arange(-7, 8)
    cand = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    cand = cand[np.abs(cand).max(1) > 0]
    cand = cand[np.lexsort((np.abs(cand).sum(1), np.abs(cand).max(1)))]
    q, ok = np.zeros_like(g), np.zeros(len(g), dtype=bool)
    for i, gi in enumerate(g):
        if not gi.any():
            q[i], ok[i] = (1.0, -2.0, 3.0), True
            continue
        good = (cand @ gi == 0) & ((cand != 0) | (gi == 0)[None, :]).all(1)
        j = np.flatnonzero(good)
        if len(j):
            q[i], ok[i] = cand[j[0]], True
    return q, ok


def act_prime(kind, z):
    """d out / d pre-activation of a head channel."""
    s = torch.sigmoid(z)
    if kind == "softplus":
        return s
    return s * (1 - s) * (2.0 if kind in ("rpv_k", "rpv_theta") else 1.0)


def _choose_seeds(case, rng):
    """Lattice pre-activation seeds for every point (case.seeds) and the per-point upstream gradient d_out that produces
    them (case.coef, float64; the tests hand its fp32 rounding to the module).

    A seed of output channel c is 2^-e_c times an integer of at most four bits (e_c the channel's level), so that every
    backward value of a unit u is 2^-e_u times an integer whatever path it took.  Head channels take EVEN integers, the
    sigma channel ODD ones: the sigma term of d y_L is still an fp32 value (14 roundings off the lattice) when the
    backward chain adds it to the heads' exact term and rounds to 16 bits; where the lattice sum is not zero that
    rounding snaps, where it were zero it would keep the noise.  Even + odd is never zero.  The learned-normal seeds are
    perpendicular to v and cannot be given a parity; their columns of y_L are their own (the builder keeps the narrow
    rows' columns disjoint) and points where such a column's lattice sum cancels get a zero learned-normal seed.
      sigmoid / softplus channel:  coef = seed / act'(z)       (head_y_dy, bwd_dpre)
      sigma:                       coef = seed / s'             (sbar is exactly 0: gbar' . g' = -q . g' = 0)
      learned normal:              dn = |v| q, q . v = 0  ->  seed = -q          (bwd_dpre)
      analytic normal:             dn = |g'| q, q . g' = 0 ->  gbar' = -q        (field_adjbwd.hip seed line; k = 0, gs aside);
                                   at g' = 0 (the eps floor):  dn = sqrt(eps) q / s'  ->  gbar' = -q."""
    chans, C = channels(case)
    bk = forward_book(case, N_MAX)
    lv = case.levels
    coef = torch.zeros(N_MAX, C, dtype=torch.float64)
    seeds = dict(heads={}, sraw=None, nlr=None, gbar=None)
    info = SimpleNamespace(an_ok=None, nlr_ok=None)

    def ints(shape, even):
        m = rng.integers(1, 4, size=shape) * 2 if even else rng.integers(0, 4, size=shape) * 2 + 1
        return torch.from_numpy((m * rng.choice([-1, 1], size=shape)).astype(np.float64))
    for kind, hname, c0, w in chans:
        if hname is not None:
            nout = dict(case.heads)[hname]
            e = torch.from_numpy(lv[hname + ".2"].astype(np.float64))
            sd = ints((N_MAX, nout), True) * torch.exp2(-e)
            seeds["heads"][hname] = sd
            coef[:, c0:c0 + nout] = sd / act_prime(kind, bk.head_z2[hname])     # (tile3 heads: the first of the three channels)
        elif kind == "sigma":
            sd = ints((N_MAX,), False) * 2.0 ** -float(lv["sigma_from_xyz.0"][0])
            seeds["sraw"] = sd
            coef[:, c0] = sd / bk.sp
        elif kind == "normal_lr":
            e = lv["grad_from_xyz"].astype(np.float64)
            v = bk.nraw.numpy()
            vi = np.round(v / (2.0 ** e * Q0)[None, :])   # v_c = 2^e_c Q0 vi_c, seed_c = -2^-e_c q_c:  seed . v = -Q0 q . vi
            q, ok = _perp(vi)
            ok &= vi.any(1)                               # v = 0: the eps floor of normal_lr; no seed there
            q[~ok] = 0.0
            qv = torch.from_numpy(q * (2.0 ** -e)[None, :])
            seeds["nlr"] = -qv
            coef[:, c0:c0 + 3] = qv * bk.nraw.norm(dim=1, keepdim=True)
            info.nlr_ok = ok
        elif kind == "normal_an":
            es = float(lv["sigma_from_xyz.0"][0])
            gi = np.round(bk.gprime.numpy() / 2.0 ** es)
            q, ok = _perp(gi)
            q[~ok] = 0.0
            qt = torch.from_numpy(q)
            seeds["gbar"] = -qt
            nrm = bk.gprime.norm(dim=1, keepdim=True)
            floor = torch.from_numpy(~gi.any(1))[:, None]
            coef[:, c0:c0 + 3] = torch.where(floor, qt * math.sqrt(FP32_EPS) / bk.sp[:, None], qt * nrm)
            info.an_ok = ok
    # cancellations of the learned-normal columns of d y_L (see the docstring)
    if seeds["nlr"] is not None:
        for _ in range(4):
            _, book = backward_chains(case, bk, seeds)
            Wg = case.params["grad_from_xyz.weight"]
            cols = (Wg != 0).any(0)
            bad = ((book.dyL[:, cols] == 0) & (book.noisy[:, cols] != 0)).any(1)
            if not bool(bad.any()):
                break
            seeds["nlr"][bad] = 0.0
            c0 = [c for k, _, c, _ in chans if k == "normal_lr"][0]
            coef[bad, c0:c0 + 3] = 0.0
    case.seeds, case.coef, case.seed_info = seeds, coef, info


def seeds_of(case, B):
    s = case.seeds
    return dict(heads={k: v[:B] for k, v in s["heads"].items()}, sraw=s["sraw"][:B],
                nlr=None if s["nlr"] is None else s["nlr"][:B], gbar=None if s["gbar"] is None else s["gbar"][:B])


# ------------------------------------------------------------------------------------------------ rounding counts
# Units: u = 2^-24, the relative error of ONE correctly rounded fp32 operation (half an ulp).  The HIP device functions
# the kernels call are documented at 1 ulp (expf, log1pf, expm1f, sqrtf) = 2 u; +, *, fma and (hipcc's default) / are
# correctly rounded = 1 u.
def sigmoid_err(z):
    """Relative error bound, in u, of sigmoid_f(z) = 1 / (1 + expf(-z)) for an exact z: expf 2 u weighed by e^-z / (1 + e^-z),
    the addition 1 u, the division 1 u."""
    return 2.0 + 2.0 * torch.sigmoid(-z)


def seed_roundings(kind, z):
    """Bound, in u, on the relative error of the fp32 pre-activation seed the backward chain forms (bwd_dpre, head_y_dy
    in csrc/field_bwd.hip) from d_out = fp32(seed / act'(z)), per element of the exact pre-activation z.
      d_out's own rounding                                   1
      sigma:     dgo * sigmoid_f(sraw)                       sigmoid_err + 1
      softplus:  y = log1pf(expf(z)) stored; dy * -expm1f(-y):
                 y: expf 2, log1pf 2 (both relative to y, the first weighed by <= 1) -> 4; -expm1f(-y) = s: the error of y
                 enters as y e^-y / s * 4 <= 4 (y e^-y <= 1 - e^-y), expm1f 2, the product 1
      sigmoid:   y = sigmoid_f(z) stored (sigmoid_err = E); dy * y * (1 - y): y E; 1 - y: E y / (1 - y) + 1 = E e^z + 1;
                 two products 2
      rpv_k / rpv_theta: the forward stores o = (y - 0.5) * 2 + 1 resp. (y - 0.5) * 2 and the backward recovers
                 y' = (o - 1) * 0.5 + 0.5 resp. o * 0.5 + 0.5: y - 0.5 is exact for y in [1/4, 1] (|z| <= 1.09; else 1 u of
                 it: <= 1/y u of y), * 2 exact, + 1: one rounding of a value in [1, 2): 2^-24 absolute = 1 / y u of y;
                 o - 1 exact, * 0.5 exact, + 0.5: 1 u.  rpv_theta has no "+ 1".  So E' = E + 2 / y + 1 (k), E + 1 / y + 1
                 (theta) replaces E, and dy = 2 dv is exact."""
    if kind == "sigma":
        return 1.0 + sigmoid_err(z) + 1.0
    if kind == "softplus":
        return torch.full_like(z, 1.0 + 4.0 + 2.0 + 1.0)
    E = sigmoid_err(z)
    y = torch.sigmoid(z)
    if kind == "rpv_k":
        E = E + 2.0 / y + 1.0
    elif kind == "rpv_theta":
        E = E + 1.0 / y + 1.0
    return 1.0 + E + (E * torch.exp(z) + 1.0) + 2.0


def normal_seed_roundings(vec, q, S):
    """Bound, in u, per component, on the relative error of the seed -(dn_c inv - v_c k) [* s'] around -q_c, for both
    normalisations (bwd_dpre's learned normal: v exact, S = 0; field_adjbwd.hip's seed line: v = gx = s' g' as
    field_adjoint.hip stashed it, S = sigmoid_err + 1 per component, and the result is multiplied by s').
      inv = 1 / sqrtf(max(n2, eps)):  n2 = sum v_c^2 is exact for an exact v (squares of 4-bit integers); else 2 S + 1 per
          square and 2 for the sums, halved by the root; sqrtf 2, the division 1
      dn_c (fp32 of the float64 value) 1;  dn_c * inv 1;  the subtraction 1
      v_c k, k = (v . dn) inv^3 with v . q = 0 exactly: v . dn is pure rounding noise, at most (1 + 1 + 2) u sum |v_j dn_j|
          (v_j's own last rounding, dn_j's, the fma chain's), i.e. relative to dn_c inv: 4 |v_c| sum_j |v_j q_j| / (|v|^2 |q_c|)
      * s' (analytic only): sigmoid_err + 1 = S
    q_c = 0 is only chosen where v_c = 0, and then the seed is exactly 0.  At v = 0 (the eps floor; analytic only):
    inv = 1 / sqrtf(eps) 3, dn 1, two products 2, s' S."""
    S = S if torch.is_tensor(S) else torch.full((vec.shape[0], 1), float(S), dtype=torch.float64)
    exact = bool((S == 0).all())
    n2 = (vec * vec).sum(1, keepdim=True)
    noise = 4.0 * vec.abs() * (vec * q).abs().sum(1, keepdim=True) / (n2.clamp_min(1e-300) * q.abs().clamp_min(1e-300))
    k = (0.0 if exact else (2 * S + 3) / 2) + 3 + 1 + 1 + 1 + noise + S
    return torch.where(q == 0, torch.zeros_like(k), torch.where(n2 == 0, 6 + S + torch.zeros_like(k), k))


def seed_k(case, bk, B):
    """|seed| * (its rounding count) for every seed, in the layout of seeds_of: the input of backward_chains(absolute=True)
    that yields sum |contribution| * k, the bound on |G - G64| / u."""
    chans, _ = channels(case)
    sd = seeds_of(case, B)
    out = dict(heads={}, sraw=None, nlr=None, gbar=None)
    for kind, hname, c0, w in chans:
        if hname is not None:
            out["heads"][hname] = sd["heads"][hname].abs() * seed_roundings(kind, bk.head_z2[hname])
        elif kind == "sigma":
            out["sraw"] = sd["sraw"].abs() * seed_roundings("sigma", bk.sraw)
        elif kind == "normal_lr":
            out["nlr"] = sd["nlr"].abs() * normal_seed_roundings(bk.nraw, sd["nlr"], 0.0)
        elif kind == "normal_an":
            out["gbar"] = sd["gbar"].abs() * normal_seed_roundings(bk.gprime, sd["gbar"], (sigmoid_err(bk.sraw) + 1.0)[:, None])
    return out


# ------------------------------------------------------------------------------------------------ lattice helpers
def lsb_exponent(t):
    """Exponent of the lowest set bit of every non-zero float64 of t (int64 array); zeros give a large value."""
    a = np.asarray(t, dtype=np.float64)
    m, e = np.frexp(a)
    mi = np.abs(np.ldexp(m, 53)).astype(np.int64)
    low = mi & -mi
    tz = np.where(mi == 0, 0, np.round(np.log2(np.maximum(low, 1))).astype(np.int64))
    return np.where(a == 0, 10 ** 6, e - 53 + tz)


def significant_bits(t):
    a = np.asarray(t, dtype=np.float64)
    _, e = np.frexp(a)
    return np.where(a == 0, 0, e - lsb_exponent(a))


def survives(t, dtype):
    """True where a float64 value survives a round trip through the 16-bit type (and is not subnormal there)."""
    t = torch.as_tensor(t, dtype=torch.float64)
    r = t.to(dtype).double()
    tiny = float(torch.finfo(dtype).tiny)
    return (r == t) & ((t == 0) | (t.abs() >= tiny))
