"""The field kernels held to exact arithmetic on dyadic-lattice ReLU networks (tests/lattice_cases.py), in fp32, bf16 and
fp16 alike.  On these networks every 16-bit operand is exactly representable and every fp32 accumulation is exact in any
order (the premises, asserted on the CPU by tests/test_lattice_cpu.py), so a kernel result differs from the float64
reference only by the few fp32 operations of the head activations and of the normalisations.  Every tolerance below is a
count of those operations, in units of u = 2^-24 (one correctly rounded fp32 operation; the device functions expf, log1pf,
expm1f, sqrtf are documented at 1 ulp = 2 u), never a measurement of the kernels.

Nothing here reads the stash; everything goes through the module's forward / backward."""
import pytest
import torch

import lattice_cases as LC
from test_gpu_parity import build_model, diag, DEV
from test_gpu_half_invariants import _fault_word

pytestmark = pytest.mark.gpu

DTYPES = ["fp32", "bf16", "fp16"]
U = LC.U24
_MODELS, _REFS = {}, {}


def _model(name, dtype):
    if (name, dtype) not in _MODELS:
        case = LC.get_case(name)
        model = build_model(case.cfg, 0, dtype)
        model.load_state_dict(LC.state_dict32(case))
        _MODELS[(name, dtype)] = model
    return _MODELS[(name, dtype)]


def _ref(name, B):
    """The float64 reference of the first B points of a case, computed once and shared: outputs, bookkeeping, gradients
    of sum(out * coef), and the two absolute backwards (|seeds| and |seeds| x their rounding counts)."""
    if (name, B) not in _REFS:
        case = LC.get_case(name)
        bk = LC.forward_book(case, B)
        r = dict(case=case, bk=bk, out=LC.reference_out(case, B, bk), sigma=LC.oracle_out(case, B, sigma_only=True))
        # the restated chains on the lattice seeds: exact float64 integers-times-powers-of-two; autograd through the oracle
        # (with d_out = seed / act', a float64 quotient) agrees with them to 1e-10 relative (tests/test_lattice_cpu.py)
        r["G64"], _ = LC.backward_chains(case, bk, LC.seeds_of(case, B))
        r["A1"], _ = LC.backward_chains(case, bk, LC.seeds_of(case, B), absolute=True)
        r["AK"], _ = LC.backward_chains(case, bk, LC.seed_k(case, bk, B), absolute=True)
        _REFS[(name, B)] = r
    return _REFS[(name, B)]


def _dev_pts(case, B):
    return tuple(None if a is None else a.float().to(DEV) for a in LC.take(case.pts, B))


def _call(model, case, pts, **kw):
    xyz, dirs, t = pts
    return model(xyz, input_dir=dirs, input_t=t, **dict(case.flags, **kw))


# ------------------------------------------------------------------------------------------------ forward
def _forward_tolerance(case, bk, out):
    """Element-wise absolute tolerance of the full forward's output, from the exact pre-activations (float64)."""
    chans, C = LC.channels(case)
    tol = torch.zeros_like(out)
    for kind, h, c0, w in chans:
        if kind == "sigma":
            tol[:, c0] = 4 * U * out[:, c0]
        elif kind == "softplus":
            tol[:, c0:c0 + 1] = 4 * U * out[:, c0:c0 + 1]
        elif kind in ("sigmoid", "tile3", "rpv_k", "rpv_theta"):
            z = bk.head_z2[h]
            y, E = torch.sigmoid(z), LC.sigmoid_err(z)
            if kind in ("sigmoid", "tile3"):
                t = E * y * U
            else:
                t = (2 * y * E + out[:, c0:c0 + z.shape[1]].abs() + (2 * y - 1).abs()) * U
            tol[:, c0:c0 + w] = t if t.shape[1] == w else t.expand(-1, w)
        elif kind == "normal_lr":
            tol[:, c0:c0 + 3] = 4 * U * out[:, c0:c0 + 3].abs()
        elif kind == "normal_an":
            S = (LC.sigmoid_err(bk.sraw) + 1.0)[:, None]
            tol[:, c0:c0 + 3] = ((2 * S + 3) / 2 + 3 + S + 1) * U * out[:, c0:c0 + 3].abs()
    return tol


def _forward_params():
    return [(n, B) for n, B in LC.case_sizes()]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,B", _forward_params())
def test_forward_is_the_float64_reference(name, B, dtype):
    """Training forward (stash kept), inference forward and sigma-only forward against oracle/field.py in float64.

    The head pre-activations, sigma_raw, the learned-normal vector v and g' = (d sigma / d xyz) / s' are exact.  Counting the
    fp32 operations from there to the stored value (csrc/field_fwd.hip, csrc/field_adjoint.hip), relative unless noted:
      sigma, beta   softplus_f = log1pf(expf(x)): expf 2 u weighed by sigmoid(x) / softplus(x) <= 1, log1pf 2 u         4 u
      sigmoid head  sigmoid_f = 1 / (1 + expf(-x)): expf 2 u weighed by e^-x / (1 + e^-x), + 1 u, / 1 u          E <= 4 u
      rpv k, theta  (y - 0.5) * 2 [+ 1]: absolute 2 y E u from y, u |2y - 1| from the subtraction, u |out| from the + 1
      normal_lr     -v / sqrtf(max(|v|^2, eps)): |v|^2 exact, sqrtf 2 u, the division 1 u, the product 1 u            4 u
      normal_an     gx_c = s' g'_c: S = E + 1; |gx|^2: 2 S + 1 per square, 2 for the sums, halved by sqrtf (+ 2 u),
                    the division 1 u, the product with gx_c S + 1                                ((2 S + 3) / 2 + S + 4) u <= 16 u
    All are below 1e-5 relative (16 u = 9.5e-7), asserted - relative to the sigmoid's value y for the RPV theta channel,
    whose 2 y - 1 crosses zero (its premise is intact: the error is that of y).  Where v = 0 or g' = 0 the reference's eps floor gives exactly 0
    (0 / sqrt(eps)), and so must the kernel; ReLU units whose pre-activation is exactly 0 (a third of them here) take the
    reference's branch (derivative 0) or the analytic normal differs by far more than 16 u."""
    r = _ref(name, B)
    case, bk = r["case"], r["bk"]
    model, pts = _model(name, dtype), _dev_pts(r["case"], B)
    tol = _forward_tolerance(case, bk, r["out"])
    chans, _ = LC.channels(case)
    scale = r["out"].abs()
    for kind, h, c0, w in chans:
        if kind == "rpv_theta":          # 2 y - 1 crosses zero: its error is relative to y, the value before the affine map
            scale[:, c0:c0 + w] = torch.maximum(scale[:, c0:c0 + w], torch.sigmoid(bk.head_z2[h]).expand(-1, w))
    nz = scale != 0
    assert float((tol[nz] / scale[nz]).max()) < 1e-5
    for mode in ("train", "infer", "sigma"):
        if mode == "train":
            got = _call(model, case, pts).detach()
        else:
            with torch.no_grad():
                got = _call(model, case, pts, sigma_only=True) if mode == "sigma" else _call(model, case, pts)
        got = got.double().cpu()
        want, t = (r["sigma"], 4 * U * r["sigma"]) if mode == "sigma" else (r["out"], tol)
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), f"{mode}: shape / finite"
        err = (got - want).abs()
        ratio = float((err / t.clamp_min(1e-300))[t > 0].max())
        diag(f"lattice forward {name} {dtype} B={B} {mode}: worst |err| / tolerance {ratio:.3f}")
        if not bool((err <= t).all()):
            i, c = [int(v) for v in (err > t).nonzero()[0]]
            kind = [k for k, _, c0, w in chans if c0 <= c < c0 + w][0] if mode != "sigma" else "sigma"
            raise AssertionError(f"{name} {dtype} B={B} {mode}: {int((err > t).sum())} values off, first at point {i} channel {c} ({kind}): "
                                 f"got {float(got[i, c])!r} want {float(want[i, c])!r}, |err| {float(err[i, c]):.3e} > {float(t[i, c]):.3e}")
    assert _fault_word() == 0


# ------------------------------------------------------------------------------------------------ gradients
def _backward(model, case, pts, coef):
    xyz, dirs, t = pts
    model.zero_grad(set_to_none=True)
    t_in = None if t is None else t.clone().requires_grad_(True)
    out = _call(model, case, (xyz, dirs, t_in))
    (out * coef).sum().backward()
    G = {k: (torch.zeros_like(v) if v.grad is None else v.grad).double().cpu() for k, v in model.named_parameters()}
    if t_in is not None:
        G["d_t_embed"] = t_in.grad.double().cpu()
    return G


def _exact_in_16_bits(k):
    """Gradients every operand of which is a 16-bit value when it is multiplied: trunk, feats, the heads' (folded) first
    layers, d_t_embed.  The others are sums of fp32 seed x 16-bit activation (skinny_wgrad_kernel keeps d pre-activation
    in fp32): the heads' second layers, sigma_from_xyz, grad_from_xyz."""
    return k.startswith("fc_net.") or k.startswith("feats_from_xyz.") or k.endswith(".0.weight") and not k.startswith("sigma") \
        or k.endswith(".0.bias") and not k.startswith("sigma") or k == "d_t_embed"


def _check_gradients(tag, dtype, G, G64, A1, AK, n_extra):
    assert set(G) == set(G64), sorted(set(G) ^ set(G64))
    bad, worst = [], 0.0
    for k in sorted(G64):
        g, w = G[k], G64[k]
        assert bool(torch.isfinite(g).all()), f"{tag} {k}: non-finite"
        if dtype != "fp32" and _exact_in_16_bits(k):
            assert torch.equal(w.float().double(), w), f"{k}: the reference is not an fp32 value"
            if not torch.equal(g, w):
                n = int((g != w).sum())
                i = tuple(int(v) for v in (g != w).nonzero()[0])
                bad.append(f"{k}: {n} of {g.numel()} elements differ, first at {i}: got {float(g[i])!r} want {float(w[i])!r}")
            continue
        bound = U * (AK[k] + n_extra * A1[k])
        err = (g - w).abs()
        ratio = float((err / bound.clamp_min(1e-300))[(bound > 0) | (err > 0)].max()) if bool(((bound > 0) | (err > 0)).any()) else 0.0
        worst = max(worst, ratio)
        diag(f"lattice gradient {tag} {k}: worst |G - G64| / bound {ratio:.3e}")
        if not bool((err <= bound).all()):
            i = tuple(int(v) for v in (err > bound).nonzero()[0])
            bad.append(f"{k}: {int((err > bound).sum())} elements outside the bound, first at {i}: got {float(g[i])!r} want {float(w[i])!r}, "
                       f"|err| {float(err[i]):.3e} > {float(bound[i]):.3e}")
    diag(f"lattice gradient {tag}: worst ratio {worst:.3e}")
    assert not bad, f"{tag}: " + "; ".join(bad[:6])


def _n_extra(case, B, dtype):
    """Roundings downstream of the seeds, in u of the sum of the absolute contributions (A1).
    16-bit modes, the tensors held to the bound (fp32 seed x 16-bit activation summed over the points): the product 1, the
    sum of B terms in any order B - 1, the split sums' final adds and the store: B + 8.
    fp32 mode, every tensor: nothing snaps, so a seed's 24 bits travel the whole chain (its products with the weights,
    powers of two, and with the masks are exact; the sums round): a trunk or head GEMM adds at most 2 non-zero terms per
    row and, by the builder's permutations, per hidden column; d y_L collects one term per head, sigma's and the learned
    normal's, <= 7 -> 6 roundings.  3 per layer over L + 3 layers (second layer, folded first layer, feats inside it, the
    trunk) plus 4 covers both.  Then the weight gradient's product and sum over B points as above; bn_unfold_heads' chains
    have <= 3 non-zero products each (inside the 8)."""
    return B + 8 + (3 * (case.cfg.layers + 3) + 4 if dtype == "fp32" else 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,B", LC.case_sizes())
def test_gradients_are_the_float64_reference(name, B, dtype):
    """Every parameter's gradient (and d_t_embed with --beta) of sum(out * d_out) against the float64 reference: the chains of
    lattice_cases.backward_chains on the lattice seeds, which tests/test_lattice_cpu.py ties to autograd through
    oracle/field.py (the autograd value itself carries float64 rounding, 1e-16, that an exact comparison would see).  d_out is chosen per point from the reference (lattice_cases._choose_seeds) so that every pre-activation
    seed the kernels form lies k u from a lattice value of <= 4 bits; k is counted per seed from the code
    (lattice_cases.seed_roundings: 5 .. 7 for sigma, 8 for softplus, 9 .. 21 for a sigmoid channel at |z| <= 2, up to 38 for the
    RPV k channel; normal_seed_roundings: <= 18 learned, <= 24 analytic - above the 16 the construction hoped for in the
    channels named in test_lattice_cpu.test_the_seeds_snap_onto_the_lattice, and for the reasons given there).

    Bound, every mode:  |G - G64| <= u (A_K + n A_1) element-wise; A_1 is the same backward in float64 over |seeds|, |W|,
    |y| with the masks unchanged, A_K the same with every |seed| multiplied by its k; n = _n_extra.
    16-bit modes: rounding to 16 bits snaps every seed onto the lattice and all that follows is exact, so the trunk
    weights and biases, feats_from_xyz, every head's first layer (evaluated folded, unfolded by bn_unfold_heads) and
    d_t_embed are asserted torch.equal to the reference.  NOT bit-equal, by design: the heads' second layers,
    grad_from_xyz and sigma_from_xyz.0 - skinny_wgrad_kernel multiplies the 16-bit activation by the fp32 d pre-activation
    (csrc/field_wgrad.hip), which never passes a 16-bit rounding; they are held to the bound.  (The issue expected the
    sigma head to be bit-equal; it is the same kernel.)  With analytic normals sigma_from_xyz.0.weight also receives the
    exact adjoint job 1^T abar'_L."""
    r = _ref(name, B)
    case = r["case"]
    G = _backward(_model(name, dtype), case, _dev_pts(case, B), case.coef[:B].float().to(DEV))
    _check_gradients(f"{name} {dtype} B={B}", dtype, G, r["G64"], r["A1"], r["AK"], _n_extra(case, B, dtype))
    assert _fault_word() == 0


_AN = [(n, B) for n, B in LC.case_sizes() if LC.CASES[n][1].get("nr_an_on") and B in (65, 600, 1100)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,B", _AN)
def test_normals_only_loss_has_no_primal_gradient(name, B, dtype):
    """A loss on the analytic normal alone.  With ReLU dD/dz = 0, so zbar_l, what the adjoint backward hands to the primal
    chain at every layer, is exactly 0, and sbar = (w_sigma . abar'_L)(1 - s') is 0 on the lattice (gbar' . g' = 0): the
    primal chain runs on zero seeds.  16-bit modes: every bias gradient and every head gradient is exactly 0 and the
    trunk matrices are the adjoint job delta'^T [gbar' ; abar'] alone, torch.equal to the reference.  fp32 mode: sbar is the
    rounding noise of an fp32 dot product; its absolute terms are part of A (backward_chains carries them), the bound is
    that of test_gradients_are_the_float64_reference."""
    case = LC.get_case(name)
    chans, C = LC.channels(case)
    c0 = [c for k, _, c, _ in chans if k == "normal_an"][0]
    key = (name, B, "normals only")
    if key not in _REFS:
        coef = torch.zeros(B, C, dtype=torch.float64)
        coef[:, c0:c0 + 3] = case.coef[:B, c0:c0 + 3]
        bk = LC.forward_book(case, B)
        sd, sk = LC.seeds_of(case, B), LC.seed_k(case, bk, B)
        for s in (sd, sk):
            s["heads"] = {h: torch.zeros_like(v) for h, v in s["heads"].items()}
            s["sraw"] = torch.zeros_like(s["sraw"])
            s["nlr"] = None if s["nlr"] is None else torch.zeros_like(s["nlr"])
        _REFS[key] = dict(coef=coef, G64=LC.backward_chains(case, bk, sd)[0], A1=LC.backward_chains(case, bk, sd, absolute=True)[0],
                          AK=LC.backward_chains(case, bk, sk, absolute=True)[0])
    r = _REFS[key]
    G = _backward(_model(name, dtype), case, _dev_pts(case, B), r["coef"].float().to(DEV))
    _check_gradients(f"{name} {dtype} B={B} normals only", dtype, G, r["G64"], r["A1"], r["AK"], _n_extra(case, B, dtype))
    adj = {f"fc_net.{2*l}.weight" for l in range(case.cfg.layers)} | {"sigma_from_xyz.0.weight"}
    for k, w in r["G64"].items():
        if k not in adj:
            assert float(w.abs().max()) == 0.0, f"the reference's d {k} is not zero"
            if dtype != "fp32":
                assert float(G[k].abs().max()) == 0.0, f"{name} {dtype} B={B}: d {k} is not exactly zero (max {float(G[k].abs().max()):.3e}): zbar or sbar leaks"
        else:
            assert float(w.abs().max()) > 0.0
    assert _fault_word() == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [n for n in LC.CASES if LC.CASES[n][1].get("nr_an_on")])
def test_relu_at_zero_takes_the_reference_branch(name, dtype):
    """Units whose pre-activation is exactly 0 (torch: derivative 0).  The other convention (derivative 1 at 0) gives, in
    float64, a different d sigma / d xyz at many points of the case; at those points the kernel's analytic normal
    (forward stash -> adjoint chain) must be the reference's, within the forward test's 16 u, and not the other one.  The
    backward's side of the same branch is held by test_gradients_are_the_float64_reference: dz_l = dy (.) [z > 0] enters
    every trunk gradient, a third of the pre-activations are 0, and those gradients are compared bit for bit."""
    case = LC.get_case(name)
    B = case.sizes[-1]
    r = _ref(name, B)
    bk = r["bk"]
    F, L, skip = case.cfg.feat, case.cfg.layers, case.skip
    a, gp = case.params["sigma_from_xyz.0.weight"].expand(B, F), torch.zeros(B, 3, dtype=torch.float64)
    for l in reversed(range(L)):
        back = (a * (bk.z[l] >= 0).double()) @ case.params[f"fc_net.{2*l}.weight"]
        if l == skip:
            gp, a = gp + back[:, :3], back[:, 3:]
        elif l == 0:
            gp = gp + back
        else:
            a = back
    other = -LC.OF.l2_normalize(gp * bk.sp[:, None])
    chans, _ = LC.channels(case)
    c0 = [c for k, _, c, _ in chans if k == "normal_an"][0]
    want = r["out"][:, c0:c0 + 3]
    differs = ((other - want).abs() > 1e-3).any(1)
    assert int(differs.sum()) >= B // 10, f"only {int(differs.sum())} points tell the two conventions apart"
    got = _call(_model(name, dtype), case, _dev_pts(case, B)).detach().double().cpu()[:, c0:c0 + 3]
    tol = 16 * U * want.abs()
    off = ((got - want).abs() > tol).any(1) & differs
    assert not bool(off.any()), f"{name} {dtype}: {int(off.sum())} of {int(differs.sum())} points with a unit at z = 0 do not take the reference's branch " \
                                f"({int((((got - other).abs() < 1e-6).all(1) & differs).sum())} of them match the derivative-1 convention)"
    assert _fault_word() == 0
