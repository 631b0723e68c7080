"""Premises of the lattice tests (tests/lattice_cases.py, tests/test_gpu_lattice.py), asserted on the float64 reference.
They are conditions, not measurements: if one fails, the GPU tests' exactness argument does not hold and the builder has
to change, not a tolerance."""
import numpy as np
import pytest
import torch

import lattice_cases as LC

HALF = {"bf16": torch.bfloat16, "fp16": torch.float16}
NAMES = list(LC.CASES)
GS_TARGET_CHAIN, GS_TARGET_ADJ = 8, 6          # BN_GS_TARGET_CHAIN / BN_GS_TARGET_ADJ (csrc/common.h)


def _full(name):
    case = LC.get_case(name)
    bk = LC.forward_book(case, LC.N_MAX)
    G, book = LC.backward_chains(case, bk, LC.seeds_of(case, LC.N_MAX))
    return case, bk, G, book


def _folded(case):
    F = case.cfg.feat
    Wf = case.params["feats_from_xyz.weight"]
    return {h: case.params[f"{h}.0.weight"][:, :F] @ Wf for h, _ in case.heads}


def _held_in_16_bits(case, bk, book):
    """name -> tensor of every value a kernel holds in the 16-bit type."""
    vals = {"xyz": bk.xyz}
    if bk.dirs is not None:
        vals["dirs"] = bk.dirs
    if bk.t is not None:
        vals["t_embed"] = bk.t
    for k, v in case.params.items():
        if k.endswith(".weight"):
            vals[k] = v
    for h, w in _folded(case).items():
        vals[f"folded {h}.0.weight"] = w
    for l in range(case.cfg.layers):
        vals[f"y{l}"], vals[f"a'{l}"], vals[f"delta'{l}"], vals[f"dz{l}"] = bk.y[l], bk.adj_a[l], bk.adj_delta[l], book.dz[l]
        if book.dbar[l] is not None:
            vals[f"dbar'{l}"], vals[f"abar'{l+1}"] = book.dbar[l], book.abar[l + 1]
    for h, _ in case.heads:
        vals[f"g {h}"], vals[f"dG {h}"] = bk.head_g[h], book.dG[h]
    if case.seeds["gbar"] is not None:
        vals["gbar'"] = case.seeds["gbar"]
    return vals


def _grad_scale(amax, target):
    """grad_scale_from (csrc/common.h)."""
    if not amax > 0:
        return 1.0
    _, e = np.frexp(np.float32(amax))
    return float(np.ldexp(1.0, int(np.clip(target - e, -24, 40))))


@pytest.mark.parametrize("name", NAMES)
def test_the_restated_chains_are_the_oracles_gradient(name):
    """forward_book / backward_chains restate in float64 what the kernels run (seeds -> chains -> weight-gradient sums ->
    unfold).  With the case's seeds they must give autograd's gradient of sum(out * coef) through oracle/field.py to
    float64 rounding: this ties the seeds to d_out (coef) and the bookkeeping to the reference."""
    case = LC.get_case(name)
    for B in case.sizes:
        bk = LC.forward_book(case, B)
        G, _ = LC.backward_chains(case, bk, LC.seeds_of(case, B))
        G64 = LC.oracle_grads(case, B, case.coef[:B])
        assert set(G) == set(G64), sorted(set(G) ^ set(G64))
        for k in G64:
            A = float(G64[k].abs().max())
            assert float((G[k] - G64[k]).abs().max()) <= 1e-10 * max(A, 1.0), f"{name} B={B} {k}"
    out, ref = LC.oracle_out(case, case.sizes[-1]), LC.reference_out(case, case.sizes[-1])
    assert out.shape[1] == LC.channels(case)[1]
    assert float((out - ref).abs().max()) < 1e-12
    # the normals-only loss of test_gpu_lattice.py
    if case.flags.get("nr_an_on"):
        B = case.sizes[-1]
        c0 = [c for k, _, c, _ in LC.channels(case)[0] if k == "normal_an"][0]
        coef = torch.zeros_like(case.coef[:B])
        coef[:, c0:c0 + 3] = case.coef[:B, c0:c0 + 3]
        sd = LC.seeds_of(case, B)
        sd.update(heads={h: torch.zeros_like(v) for h, v in sd["heads"].items()}, sraw=torch.zeros_like(sd["sraw"]),
                  nlr=None if sd["nlr"] is None else torch.zeros_like(sd["nlr"]))
        G, _ = LC.backward_chains(case, LC.forward_book(case, B), sd)
        G64 = LC.oracle_grads(case, B, coef)
        for k in G64:
            assert float((G[k] - G64[k]).abs().max()) <= 1e-10 * max(float(G64[k].abs().max()), 1.0), f"{name} normals only {k}"


@pytest.mark.parametrize("dtype", list(HALF))
@pytest.mark.parametrize("name", NAMES)
def test_every_16_bit_operand_is_representable(name, dtype):
    """Inputs, packed and folded weights, activations, a', delta', dz, dG, gbar', abar', dbar' survive a round trip through
    the type; in fp16 every non-zero gradient-side value also stays a normal number under the loss scale the kernels
    choose for the batch (grad_scale_from: max |seed| -> [128, 256) for the primal chain, max |gbar_PE| -> [32, 64) for the
    adjoint backward) and under the two neighbouring powers of two, for every batch size of the case."""
    case, bk, _, book = _full(name)
    T = HALF[dtype]
    vals = _held_in_16_bits(case, bk, book)
    for k, v in vals.items():
        ok = LC.survives(v, T)
        assert bool(ok.all()), f"{name} {dtype}: {k} does not survive ({int((~ok).sum())} values, e.g. {float(v[~ok][0])!r})"
        assert int(LC.significant_bits(v.numpy()).max()) <= 8, k
    if dtype != "fp16":
        return
    tiny, big = float(torch.finfo(T).tiny), float(torch.finfo(T).max)
    for B in case.sizes:
        sd = LC.seeds_of(case, B)
        primal = max([float(v.abs().max()) for v in sd["heads"].values()] + [float(sd["sraw"].abs().max())] +
                     ([float(sd["nlr"].abs().max())] if sd["nlr"] is not None else []))
        scales = {"chain": _grad_scale(primal, GS_TARGET_CHAIN)}
        if sd["gbar"] is not None:
            scales["adj"] = _grad_scale(float(sd["gbar"].abs().max()), GS_TARGET_ADJ)
        for k, v in vals.items():
            which = "adj" if k[:4] in ("gbar", "abar", "dbar") else ("chain" if k[:2] in ("dz", "dG") else None)
            if which is None or which not in scales:
                continue
            nz = v[:B][v[:B] != 0].abs()
            if nz.numel() == 0:
                continue
            for f in (0.5, 1.0, 2.0):
                gs = scales[which] * f
                assert float(nz.min()) * gs >= tiny and float(nz.max()) * gs <= big, f"{name} B={B} {k}: outside fp16's normal range at scale {gs}"


def _assert_exact_sum(tag, X, W, extra=None):
    """out[i][n] = sum_k X[i][k] W[n][k] (+ extra[n]): every term is a multiple of 2^(lsb(column k of X) + lsb(W[n][k])); the
    sum of the absolute terms must stay below 2^24 of the smallest such quantum of the row, so that every partial sum of
    any summation order is an integer below 2^24 quanta: exact in fp32."""
    X, W = X.numpy(), W.numpy()
    lx = LC.lsb_exponent(X).min(0)                               # (K,)
    lw = LC.lsb_exponent(W)                                      # (R, K)
    q = np.minimum((lw + lx[None, :]).min(1), 10 ** 5)           # (R,)
    S = np.abs(X) @ np.abs(W).T
    if extra is not None:
        q = np.minimum(q, LC.lsb_exponent(extra.numpy()))
        S = S + np.abs(extra.numpy())[None, :]
    live = q < 10 ** 5
    if live.any():
        worst = float((S[:, live] / np.ldexp(1.0, q[live])[None, :]).max())
        assert worst < 2.0 ** 24, f"{tag}: {worst:.3e} quanta"


def _assert_exact_outer(tag, A, Bm, plus=None):
    """G[n][k] = sum_i A[i][n] Bm[i][k] (a weight-gradient job; plus: a second job added in fp32 afterwards)."""
    la, lb = LC.lsb_exponent(A.numpy()).min(0), LC.lsb_exponent(Bm.numpy()).min(0)
    q = np.minimum(la[:, None] + lb[None, :], 10 ** 5)
    S = np.abs(A.numpy()).T @ np.abs(Bm.numpy())
    if plus is not None:
        A2, B2 = plus
        q = np.minimum(q, np.minimum(LC.lsb_exponent(A2.numpy()).min(0)[:, None] + LC.lsb_exponent(B2.numpy()).min(0)[None, :], 10 ** 5))
        S = S + np.abs(A2.numpy()).T @ np.abs(B2.numpy())
    live = q < 10 ** 5
    if live.any():
        worst = float((S[live] / np.ldexp(1.0, q[live])).max())
        assert worst < 2.0 ** 24, f"{tag}: {worst:.3e} quanta"


@pytest.mark.parametrize("name", NAMES)
def test_every_accumulation_is_exact_in_fp32(name):
    """Every GEMM output of the forward, the adjoint chain, the backward chain and the adjoint backward, every bias column
    sum, every weight-gradient element (trunk: primal job + adjoint job) and the unfold's products, over the case's
    largest point set (sub-batches sum fewer terms)."""
    case, bk, _, book = _full(name)
    p, L, F, skip = case.params, case.cfg.layers, case.cfg.feat, case.skip
    ones = torch.ones(LC.N_MAX, 1, dtype=torch.float64)
    for l in range(L):
        W = p[f"fc_net.{2*l}.weight"]
        _assert_exact_sum(f"forward {l}", bk.ins[l], W, p[f"fc_net.{2*l}.bias"])
        _assert_exact_sum(f"adjoint {l}", bk.adj_delta[l], W.T.contiguous())
        _assert_exact_sum(f"backward {l}", book.dz[l], W.T.contiguous())
        plus = None
        if book.dbar[l] is not None:
            gb = book.gbar
            inb = gb if l == 0 else (torch.cat([gb, book.abar[l]], 1) if l == skip else book.abar[l])
            _assert_exact_sum(f"adjoint backward {l}", inb, W)
            plus = (bk.adj_delta[l], inb)
        _assert_exact_outer(f"dW {l}", book.dz[l], bk.ins[l], plus)
        _assert_exact_outer(f"db {l}", book.dz[l], ones)
    yL = bk.y[-1]
    _assert_exact_sum("sigma", yL, p["sigma_from_xyz.0.weight"], p["sigma_from_xyz.0.bias"])
    if "grad_from_xyz.weight" in p:
        _assert_exact_sum("grad_from_xyz", yL, p["grad_from_xyz.weight"], p["grad_from_xyz.bias"])
    Wf, bf = p["feats_from_xyz.weight"], p["feats_from_xyz.bias"]
    dfe = torch.zeros(LC.N_MAX, F, dtype=torch.float64)
    for h, _ in case.heads:
        W1, W2 = p[f"{h}.0.weight"], p[f"{h}.2.weight"]
        Wfold = torch.cat([W1[:, :F] @ Wf, W1[:, F:]], 1)
        hin = torch.cat([yL, bk.head_in[h][:, F:]], 1)
        _assert_exact_sum(f"{h} folded first layer", hin, Wfold, W1[:, :F] @ bf + p[f"{h}.0.bias"])
        _assert_exact_sum(f"{h} second layer", bk.head_g[h], W2, p[f"{h}.2.bias"])
        _assert_exact_sum(f"{h} dG", case.seeds["heads"][h], W2.T.contiguous())
        _assert_exact_sum(f"{h} d y_L", book.dG[h], Wfold[:, :F].T.contiguous())
        _assert_exact_outer(f"{h} folded dW", book.dG[h], hin)
        _assert_exact_outer(f"{h} folded db", book.dG[h], ones)
        M, s = book.dG[h].T @ yL, book.dG[h].sum(0)
        _assert_exact_sum(f"{h} unfold dW1", torch.cat([M, s[:, None]], 1), torch.cat([Wf, bf[:, None]], 1))
        dfe = dfe + book.dG[h] @ W1[:, :F]
    # dWf = sum_h W1_h^T M_h, dbf = sum_h W1_h^T s_h: bounded together through d feats (one more regrouping of the same terms)
    _assert_exact_outer("unfold dWf", dfe, yL)
    _assert_exact_outer("unfold dbf", dfe, ones)


@pytest.mark.parametrize("name", NAMES)
def test_the_networks_are_not_degenerate(name):
    case, bk, _, book = _full(name)
    for l in range(case.cfg.layers):
        on = float(bk.D[l].mean())
        assert 0.2 <= on <= 0.8, f"{name} layer {l}: {on:.2f} of the mask is one"
        unit = bk.D[l].mean(0)
        assert float(unit.min()) > 0 and float(unit.max()) < 1, f"{name} layer {l}: a unit is always on or always off"
        W = case.params[f"fc_net.{2*l}.weight"]
        nnz = (W != 0).sum(1)
        assert int(nnz.min()) >= 1 and int(nnz.max()) <= 2, f"{name} layer {l}: non-zeros per row"
        assert bool((W != 0).any(0).all()), f"{name} layer {l}: an input column is used by no row"
        mags = set(W[W != 0].abs().tolist())
        assert mags <= {0.25, 0.5, 1.0, 2.0}, mags
    if case.skip > 0:
        W = case.params[f"fc_net.{2*case.skip}.weight"]
        assert bool((W[:, :3] != 0).any()) and bool((W[:, 3:] != 0).any())
    for h, _ in case.heads:
        W = case.params[f"{h}.0.weight"]
        assert bool((W != 0).any(0).all()), f"{name} {h}.0: an input column is used by no row"
        on = float(bk.head_D[h].mean())
        assert 0.2 <= on <= 0.8, f"{name} {h}: {on:.2f}"
    out = LC.oracle_out(case, LC.N_MAX)
    spread = out.max(0).values - out.min(0).values
    assert float(spread.min()) > 0, f"{name}: output channel {int(spread.argmin())} is constant over the batch"
    if case.flags.get("nr_an_on"):
        es = float(case.levels["sigma_from_xyz.0"][0])
        gi = bk.gprime / 2.0 ** es
        assert bool((gi == gi.round()).all()), "g' is not on its lattice"
        n_floor = int((gi.abs().sum(1) == 0).sum())
        assert 0 < n_floor < LC.N_MAX // 2, f"{name}: {n_floor} points at the eps floor"      # both kinds are present
        for B in case.sizes[1:]:
            assert bool((gi[:B].abs().sum(1) != 0).any()) and bool((gi[:B].abs().sum(1) == 0).any()), f"{name} B={B}"
        assert float(case.seed_info.an_ok.mean()) > 0.5, "fewer than half the points carry an analytic-normal seed"
    # every gradient element that a gradient test compares is fed: no parameter's gradient is identically zero
    G = _full(name)[2]
    for k, g in G.items():
        assert float(g.abs().max()) > 0, f"{name}: d {k} is zero"


@pytest.mark.parametrize("name", NAMES)
def test_relu_sits_at_zero_on_purpose(name):
    """At least 1 % of the trunk pre-activations are exactly 0 and the reference's derivative there is 0 (torch's relu).
    -0.0: the arithmetic cannot produce it here - a pre-activation is bias + a dot product whose accumulator starts at
    +0.0 (the MFMA's C operand, torch's addmm alike), and in round-to-nearest (+0) + (-0) and x + (-x) are +0 - so the
    reference must show none; the kernels' branch `z > 0` is the same for both zeros anyway."""
    case, bk, _, _ = _full(name)
    for l in range(case.cfg.layers):
        z = bk.z[l]
        assert float((z == 0).double().mean()) >= 0.01, f"{name} layer {l}"
        assert not bool(((z == 0) & torch.signbit(z)).any()), f"{name} layer {l}: a -0.0 pre-activation"
        assert bool((bk.D[l][z == 0] == 0).all())
    z = torch.tensor([0.0, -0.0, 1.0, -1.0], dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(torch.relu(z).sum(), z)
    assert g.tolist() == [0.0, 0.0, 1.0, 0.0]
    # ... and the oracle's d sigma / d xyz uses that branch: the restated adjoint chain (mask z > 0) equals autograd
    B = 257
    g64 = LC.OF.sigma_grad(case.params, case.cfg, LC.take(case.pts, B)[0], create_graph=False)
    bkB = LC.forward_book(case, B)
    assert torch.equal(g64, bkB.gprime * bkB.sp[:, None]) or float((g64 - bkB.gprime * bkB.sp[:, None]).abs().max()) < 1e-14


def _emulated_seeds(case, bk):
    """The kernels' seed arithmetic (bwd_dpre / head_y_dy in csrc/field_bwd.hip, the seed line of csrc/field_adjbwd.hip)
    in torch float32 on the host, from the exact pre-activations and fp32(d_out)."""
    f = torch.float32
    coef = case.coef.to(f)
    chans, _ = LC.channels(case)
    got, want, k = [], [], []
    sd = case.seeds
    for kind, h, c0, w in chans:
        if h is not None:
            z = bk.head_z2[h].to(f)
            nout = z.shape[1]
            dy = coef[:, c0:c0 + nout]
            if kind == "softplus":
                y = torch.log1p(torch.exp(z))
                s = dy * -torch.expm1(-y)
            else:
                y = 1 / (1 + torch.exp(-z))
                if kind == "rpv_k":
                    y, dy = ((y - 0.5) * 2 + 1 - 1) * 0.5 + 0.5, 2 * dy
                elif kind == "rpv_theta":
                    y, dy = ((y - 0.5) * 2) * 0.5 + 0.5, 2 * dy
                s = dy * y * (1 - y)
            got.append(s.double()); want.append(sd["heads"][h]); k.append(LC.seed_roundings(kind, bk.head_z2[h]))
        elif kind == "sigma":
            s = coef[:, c0] * (1 / (1 + torch.exp(-bk.sraw.to(f))))
            got.append(s.double()[:, None]); want.append(sd["sraw"][:, None]); k.append(LC.seed_roundings("sigma", bk.sraw)[:, None])
        elif kind in ("normal_lr", "normal_an"):
            dn = coef[:, c0:c0 + 3]
            if kind == "normal_lr":
                v, spm, S, q, vec = bk.nraw.to(f), 1.0, 0.0, sd["nlr"], bk.nraw
            else:
                spm = (1 / (1 + torch.exp(-bk.sraw.to(f))))[:, None]
                v, S, q, vec = bk.gprime.to(f) * spm, (LC.sigmoid_err(bk.sraw) + 1.0)[:, None], sd["gbar"], bk.gprime
            n2 = (v * v).sum(1, keepdim=True)
            inv = 1 / torch.sqrt(torch.clamp_min(n2, LC.FP32_EPS))
            kk = torch.where(n2 > LC.FP32_EPS, (v * dn).sum(1, keepdim=True) * inv * inv * inv, torch.zeros_like(n2))
            s = -(dn * inv - v * kk) * spm
            got.append(s.double()); want.append(q); k.append(LC.normal_seed_roundings(vec, q, S))
    return torch.cat(got, 1), torch.cat(want, 1), torch.cat(k, 1)


@pytest.mark.parametrize("name", NAMES)
def test_the_seeds_snap_onto_the_lattice(name):
    """Every pre-activation seed is a lattice value of at most four significant bits, and the seed the kernel forms in
    fp32 from fp32(d_out) lies within its derived rounding count k u of it (u = 2^-24; seed_roundings,
    normal_seed_roundings).  Rounding to 16 bits snaps a value onto a representable neighbour at a relative distance
    below 2^-9 (bf16) resp. 2^-12 (fp16); the counts must leave a factor 2 to fp16's: k u <= 2^-13.
    The issue's target of 2^-20 (k <= 16) holds for the sigma channel, the softplus channel and the plain sigmoid
    channels at z <= 1; it does NOT hold for the RPV k / theta channels, whose y the backward recovers from the rescaled
    output (two more roundings, amplified by y / (1 - y) = e^z in 1 - y), for sigmoid channels at z in (1, 2] (e^z again)
    and for the normal channels (the projection term is rounding noise of v . dn relative to |v| |dn|, not to a
    component).  The largest count per case is asserted below its derived ceiling, 200."""
    case = LC.get_case(name)
    bk = LC.forward_book(case, LC.N_MAX)
    got, want, k = _emulated_seeds(case, bk)
    assert int(LC.significant_bits(want.numpy()).max()) <= 4
    assert float(k.max()) * LC.U24 <= 2.0 ** -13 and float(k.max()) <= 200.0, float(k.max())
    err = (got - want).abs()
    bad = err > k * LC.U24 * want.abs()
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} emulated seeds are further than their count from the lattice, " \
                                f"worst {float((err / (k * LC.U24 * want.abs()).clamp_min(1e-300))[bad].max()):.2f} x"
    assert bool((got[want == 0] == 0).all()), "a zero seed is not exactly zero"
    # no cancellation to zero where an fp32 term of d y_L meets exact ones (lattice_cases._choose_seeds)
    _, book = LC.backward_chains(case, bk, LC.seeds_of(case, LC.N_MAX))
    assert not bool(((book.dyL == 0) & (book.noisy != 0)).any()), "an fp32 term of d y_L cancels exactly: its noise would survive the 16-bit rounding"
    ratio = (book.noisy.abs() / book.dyL.abs().clamp_min(1e-300))[book.noisy != 0]
    assert float(ratio.max()) * float(k.max()) * LC.U24 <= 2.0 ** -13, "a cancellation in d y_L amplifies the seed error past the snap"
