"""Exact properties of the field kernels in the 16-bit modes (and fp32 as a control), checked without a tolerance taken
from the code under test.  The statistical bounds of test_gpu_parity.py / test_gpu_fuzz.py (absolute output error, gradient
cosines) measure rounding; an INDEXING fault in the 16-bit kernels (a dropped stage of a point split, a row of padding read
at a tile edge, a k-chunk left at zero, a point counted twice at a slab boundary) passes them.  Three properties do not:

P1  A point's forward result is a function of the point alone: bitwise equal wherever it sits in whatever batch.
P2  The batch gradient is the sum of the one-point gradients.  The kernels add in fp32 in a fixed order; for ANY order of an
    fp32 sum of n terms |fl(sum) - sum| <= (n - 1) 2^-24 sum |t_i| to first order, and both sides are observable:
    |G(X) - S| <= 2 B 2^-24 A + 1e-30 element-wise, with S = sum_i G({x_i}), A = sum_i |G({x_i})| accumulated in fp64.
    The factor 2 covers the second-order terms and the one rounding of every one-point run's own store.
P3  A one-point trunk gradient in a 16-bit mode is exactly rank one: dW_l[n][k] = dz_l[n] * y_l[k], a product of two 16-bit
    values (16 resp. 22 significand bits: exact in fp32) added to zeros and multiplied by a power of two (the loss scale).

Nothing here reads the stash, and the library has no entry point for these tests: everything goes through the module's
forward / backward in the default (bitwise reproducible) gradient mode."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import tparams
from oracle.config import FieldConfig
from oracle import field as OF
from test_gpu_parity import build_model, make_args, diag, DEV  # noqa: F401  (make_args: build_model's argument set)

pytestmark = pytest.mark.gpu

_RPV = dict(funcM=1, funcF=1, funcH=1)
# name -> (FieldConfig arguments, forward flags, parameter seed, seed of the P2 / P3 point set).  The point-set seeds of the
# configurations P3 covers were picked with the fp64 oracle (on the CPU) so that no trunk-layer input of the first 16 points is
# below fp16's smallest normal: about one seed in seven for the widest of them, P3 asserts it.
CASES = {
    "lambert_F512": (dict(feat=512), dict(), 21, 520),
    "rpv_nlr_F256": (dict(feat=256, normal="learned", **_RPV), dict(apply_brdf=True, nr_lr_on=True), 22, 505),
    "rpv_nan_F64": (dict(feat=64, normal="analystic", **_RPV), dict(apply_brdf=True, nr_an_on=True), 23, 523),
    "rpv_nan_F512": (dict(feat=512, normal="analystic", **_RPV), dict(apply_brdf=True, nr_an_on=True), 24, 524),
    "viewdir_beta_F192": (dict(feat=192, input_viewdir=1, beta=True), dict(), 25, 500),
    "relu_nope_F128_L4": (dict(feat=128, layers=4, siren=False, mapping=False), dict(), 26, 500),
}
NO_AN = [n for n, (kw, _, _, _) in CASES.items() if kw.get("normal") != "analystic"]
DTYPES = ["fp32", "bf16", "fp16"]
N_PROBES = 40
P1_SIZES = (63, 64, 65, 255, 256, 257, 1000, 4097)
P2_SIZES = (1, 2, 63, 65, 257, 600, 1100)     # 600 / 1100: two / three point splits of the 16-bit weight gradient, last one ragged
P2_CONTROL = ("lambert_F512", "rpv_nlr_F256")  # fp32 runs of the same harness: a failure there blames the harness, not the kernel
N_RANK_ONE = 16
U24 = 2.0 ** -24


def _cfg(name):
    kw, flags, seed, _ = CASES[name]
    return FieldConfig(**kw), flags, seed


def _points(cfg, n, seed):
    """n points of the unit cube with what travels with them: a view direction (--input_viewdir) and an image embedding (--beta)."""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(n, 3, generator=g) * 2 - 1
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).contiguous() if cfg.dir_dim else None
    t = torch.randn(n, cfg.t_dim, generator=g) if cfg.beta else None
    return xyz, dirs, t


def _take(pts, idx):
    return tuple(None if a is None else a[idx].contiguous() for a in pts)


def _call(model, flags, pts, **kw):
    xyz, dirs, t = pts
    return model(xyz, input_dir=dirs, input_t=t, **dict(flags, **kw))


def _forward(model, flags, pts, mode):
    """The three forward kernels' variants: 'train' keeps the stash (grad mode), 'infer' does not, 'sigma' stops at sigma."""
    if mode == "train":
        return _call(model, flags, pts).detach()
    with torch.no_grad():
        return _call(model, flags, pts, sigma_only=True) if mode == "sigma" else _call(model, flags, pts)


def _fault_word():
    from brdf_nerf_amd import _lib
    faults = C.c_uint(123)
    _lib.check(_lib.lib().bn_device_faults(C.byref(faults), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "bn_device_faults")
    return faults.value


# ------------------------------------------------------------------------------------------------ P1
def _probe_rows(B, g):
    """Rows of a batch of B that receive a probe: row 0, the last row, both sides of every multiple of 64 and of 256 that B
    reaches (tile, wave-group and workgroup edges of every kernel variant), and N_PROBES scattered rows."""
    rows = {0, B - 1}
    for m in (64, 256):
        for k in range(m, B + 1, m):
            rows.add(k - 1)
            if k < B:
                rows.add(k)
    rows.update(int(i) for i in torch.randperm(B, generator=g)[:N_PROBES])
    return sorted(rows)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_point_results_do_not_depend_on_the_batch(name, dtype):
    """P1.  Every MFMA row is one point and the contraction order over k is fixed by the kernel, not by the row's position,
    so out(X)[i] depends on x_i (its direction, its embedding) only.  40 probe points are evaluated alone (B = 40: the
    reference), one at a time (the first 5), and embedded in filler batches of 63 ... 4097 points at row 0, the last row,
    both sides of every multiple of 64 and 256 and at scattered rows (a probe may sit at several rows of one batch).  Every
    copy must be torch.equal to the reference - for the training forward (stash kept), the inference forward and the
    sigma-only forward, each against itself, in fp32, bf16 and fp16.  The analytic normal of the forward
    (field_adjoint_kernel) carries no loss scale in any mode (only the backward chains read the amax words), so its three
    channels are held to the same zero tolerance."""
    cfg, flags, seed = _cfg(name)
    model = build_model(cfg, seed, dtype)
    probes = tuple(None if a is None else a.to(DEV) for a in _points(cfg, N_PROBES, 100 + seed))
    g = torch.Generator().manual_seed(7)
    n_cmp = 0
    for mode in ("train", "infer", "sigma"):
        ref = _forward(model, flags, probes, mode)
        assert ref.shape[0] == N_PROBES and bool(torch.isfinite(ref).all()), f"{mode}: reference run"
        for i in range(5):
            one = _forward(model, flags, _take(probes, slice(i, i + 1)), mode)
            assert torch.equal(one[0], ref[i]), f"{mode}: probe {i} alone (B = 1) differs from the B = {N_PROBES} run"
            n_cmp += ref.shape[1]
        for B in P1_SIZES:
            rows = _probe_rows(B, g)
            which = torch.arange(len(rows)) % N_PROBES
            batch = [None if a is None else a.to(DEV) for a in _points(cfg, B, 1000 * seed + B)]
            r = torch.tensor(rows, device=DEV)
            for a, p in zip(batch, probes):
                if a is not None:
                    a[r] = p[which.to(DEV)]
            out = _forward(model, flags, tuple(batch), mode)
            got, want = out[r], ref[which.to(DEV)]
            if not torch.equal(got, want):
                bad = (got != want).any(1).nonzero().flatten().tolist()
                raise AssertionError(f"{name} {dtype} {mode} B={B}: probes at rows {[rows[i] for i in bad][:12]} differ from their "
                                     f"B = {N_PROBES} result, max |diff| {float((got - want).abs().max()):.3e}")
            n_cmp += got.numel()
    diag(f"P1 {name} {dtype}: {n_cmp} output values bitwise equal to the probe-only run")
    assert _fault_word() == 0


# ------------------------------------------------------------------------------------------------ P2 / P3: shared runs
def _seed_maxima(cfg, flags, p32, pts, coef):
    """max_j |d loss / d pre-activation_j| per point over the small outputs (every head's pre-sigmoid values, sigma_raw, the
    learned-normal vector): the quantity grad_amax_kernel<0> takes its maximum over (bwd_dpre, csrc/field_bwd.hip).  From the
    fp32 oracle: a bias broadcast to one row per point receives exactly that point's d loss / d pre-activation."""
    xyz, dirs, t = pts
    n = xyz.shape[0]
    p, per = dict(p32), {}
    for k, v in p32.items():
        if k.endswith(".2.bias") or k in ("sigma_from_xyz.0.bias", "grad_from_xyz.bias"):
            per[k] = v.expand(n, -1).clone().requires_grad_(True)
            p[k] = per[k]
    out = OF.field_forward(p, cfg, xyz, dirs=dirs, t_embed=t, **flags)
    gr = torch.autograd.grad((out * coef).sum(), list(per.values()), allow_unused=True)
    return torch.cat([x.abs() for x in gr if x is not None], 1).max(1).values


def _make_inputs(name):
    """The P2 point set of a configuration (the same for every type; a batch of B is its first B points) and the per-point
    coefficient rows.  Analytic-normal channels are weighed down by 0.1 as the fuzz does.

    fp16 and the loss scale: the primal backward chain of the fp16 mode is scaled by the power of two that takes the
    batch-wide max |d pre-activation| (amax slot 0, see _seed_maxima) into [128, 256).  P2 needs the batch and its one-point
    runs to use the same scale, so every point's coefficient row is rescaled to put its OWN maximum at 1.5, the middle of
    the binade [1, 2) - the 16-bit forward's outputs move a seed by a few per cent at most, not by a quarter.  The
    assertion below (from fp32 values) makes a change that breaks the construction fail instead of loosening anything.
    With analytic normals two more maxima steer the scales: slot 1 (max |gbar_PE|, the adjoint chain's seeds) could be
    equalised the same way through the normal channels' coefficients, but slot 2 is the maximum of zbar_l, an interior
    quantity of the adjoint backward that no output of the library reports (and this file does not read the stash), and
    chain_scale takes max(slot 0, slot 2): the construction cannot equalise it, so the analytic-normal configurations run
    P2 in bf16 only (bf16 runs unscaled, amax == nullptr)."""
    cfg, flags, seed = _cfg(name)
    n = max(P2_SIZES)
    pts = _points(cfg, n, CASES[name][3])
    g = torch.Generator().manual_seed(900 + seed)
    p32 = tparams(cfg, seed)
    C_out = OF.field_forward(p32, cfg, pts[0][:2], dirs=None if pts[1] is None else pts[1][:2],
                             t_embed=None if pts[2] is None else pts[2][:2], **flags).shape[1]
    coef = torch.randn(n, C_out, generator=g)
    an = cfg.normal == "analystic"
    if an:
        c0 = 5 if cfg.beta else 4
        coef[:, c0:c0 + 3] *= 0.1
    else:
        coef = coef * (1.5 / _seed_maxima(cfg, flags, p32, pts, coef))[:, None]
        m = _seed_maxima(cfg, flags, p32, pts, coef)
        assert float(m.min()) > 1.25 and float(m.max()) < 1.75 and len(set(torch.frexp(m)[1].tolist())) == 1, \
            f"{name}: the points' seed maxima do not share one binade ({float(m.min()):.4f} .. {float(m.max()):.4f})"
    return cfg, flags, seed, pts, coef.contiguous()


def _folded_spec(model, flags):
    """The FieldSpec the forward flags select, made to keep a copy of the FOLDED head gradients M_h = dL/d(W1_h Wf), s_h =
    dL/d(W1_h bf + b1_h) - what the weight-gradient kernels sum over the points - before unfold_grads turns them into the
    gradients of W1_h, Wf, bf and clears them (brdf_nerf_amd/functions.py; a wrapper around the Python method, the library
    is not touched)."""
    spec = model.spec(flags.get("apply_brdf", False), False, flags.get("nr_lr_on", False), flags.get("nr_an_on", False))
    if not hasattr(spec, "folded_seen"):
        spec.folded_seen = {}
        inner = spec.unfold_grads

        def unfold_grads(named, named_grads, zero=True):
            spec.folded_seen = {name: (m.clone(), sv.clone()) for name, (m, sv) in spec.fold_grads.items()}
            return inner(named, named_grads, zero)
        spec.unfold_grads = unfold_grads
    return spec


def _backward(model, flags, pts, coef):
    """One forward + backward of (out * coef).sum(); returns {parameter name: gradient}, 'd_t_embed' with --beta, and the
    folded head gradients as 'folded <head>.0.weight' / 'folded <head>.0.bias'."""
    xyz, dirs, t = pts
    spec = _folded_spec(model, flags)
    spec.folded_seen = {}
    model.zero_grad(set_to_none=True)
    t_in = None if t is None else t.clone().requires_grad_(True)
    out = _call(model, flags, (xyz, dirs, t_in))
    (out * coef).sum().backward()
    grads = {k: v.grad for k, v in model.named_parameters() if v.grad is not None}
    assert spec.fold_feats and set(spec.folded_seen) == {h for h, _, _ in spec.heads}, "the folded head gradients were not seen"
    for h, (m, sv) in spec.folded_seen.items():
        grads[f"folded {h}.0.weight"], grads[f"folded {h}.0.bias"] = m, sv
    if t_in is not None:
        grads["d_t_embed"] = t_in.grad
    return grads


def _unfold_bounds(model, spec, B, A):
    """Element-wise bounds for the three gradients that bn_unfold_heads (csrc/head_fold.hip) computes FROM the sums over
    points: dW1_h[:, :F] = M_h Wf^T + s_h bf^T, dWf = sum_h W1_h[:, :F]^T M_h, dbf = sum_h W1_h[:, :F]^T s_h - fp32 fmaf
    chains of length K over the folded gradients, after the sum over points.  Their rounding is relative to
    sum_k |w_k| |M_k|, not to the (cancelling) result, so P2's right-hand side does not bound it; what does, for a linear
    map U with |U| its matrix of absolute values, is
        |fl U(M(X)) - sum_i fl U(M_i)| <= |U| (2 B u A_M)  +  2 (K + 4) u |U| A_M,      u = 2^-24,
    the first term P2's bound on M carried through U, the second the K + 4 roundings of U's own chain (products fused,
    three partial tiles, the final add, the store) once in the batch run and once over the one-point runs (|M(X)| and
    sum_i |M_i| are both A_M to first order)."""
    F = spec.feat
    named = {k: v.detach().double().cpu() for k, v in model.named_parameters()}
    Wf, bf = named["feats_from_xyz.weight"].abs(), named["feats_from_xyz.bias"].abs()
    heads = [h for h, _, _ in spec.heads]
    rows = named[f"{heads[0]}.0.weight"].shape[0]
    out = {"feats_from_xyz.weight": torch.zeros(F, F, dtype=torch.float64), "feats_from_xyz.bias": torch.zeros(F, dtype=torch.float64)}
    for h in heads:
        AM, As = A[f"folded {h}.0.weight"], A[f"folded {h}.0.bias"]
        W1 = named[f"{h}.0.weight"][:, :F].abs()
        out[f"{h}.0.weight"] = (2 * B + 2 * (F + 5)) * U24 * (AM @ Wf.T + As[:, None] * bf[None, :])
        out["feats_from_xyz.weight"] += W1.T @ AM
        out["feats_from_xyz.bias"] += W1.T @ As
    for k in ("feats_from_xyz.weight", "feats_from_xyz.bias"):
        out[k] *= (2 * B + 2 * (rows * len(heads) + 4)) * U24
    return out


_RUNS = {}
_INPUTS = {}


def _point_runs(name, dtype):
    """The one-point runs of (configuration, type, parameter seed), made once: prefix sums S_B, A_B in fp64 at every B of
    P2_SIZES (torch fp64 additions, IEEE like the host's) and the first N_RANK_ONE one-point gradients themselves."""
    key = (name, dtype) + CASES[name][2:]
    if key in _RUNS:
        return _RUNS[key]
    if name not in _INPUTS:
        _INPUTS[name] = _make_inputs(name)
    cfg, flags, seed, pts, coef = _INPUTS[name]
    model = build_model(cfg, seed, dtype)
    dpts = tuple(None if a is None else a.to(DEV) for a in pts)
    dcoef = coef.to(DEV)
    S = A = None
    sums, singles, d_t = {}, [], []
    for i in range(max(P2_SIZES)):
        gi = _backward(model, flags, _take(dpts, slice(i, i + 1)), dcoef[i:i + 1])
        if "d_t_embed" in gi:
            d_t.append(gi.pop("d_t_embed")[0].clone())
        if S is None:
            names = list(gi)
            S = {k: torch.zeros_like(v, dtype=torch.float64) for k, v in gi.items()}
            A = {k: torch.zeros_like(v, dtype=torch.float64) for k, v in gi.items()}
        assert list(gi) == names
        for k, v in gi.items():
            S[k] += v.double()
            A[k] += v.abs().double()
        if i < N_RANK_ONE:
            singles.append({k: v.cpu().clone() for k, v in gi.items() if k.startswith("fc_net.")})
        gi = None
        if i + 1 in P2_SIZES:
            sums[i + 1] = ({k: v.cpu().clone() for k, v in S.items()}, {k: v.cpu().clone() for k, v in A.items()})
    _RUNS[key] = dict(model=model, sums=sums, singles=singles, d_t=torch.stack(d_t).cpu().double() if d_t else None,
                      inputs=(cfg, flags, dpts, dcoef))
    return _RUNS[key]


def _p2_params():
    out = []
    for name, (kw, _, _, _) in CASES.items():
        for dtype in DTYPES:
            if dtype == "fp32" and name not in P2_CONTROL:
                continue
            if dtype == "fp16" and kw.get("normal") == "analystic":
                continue        # amax slot 2 cannot be equalised from outside the library: see _make_inputs
            out += [(name, dtype, B) for B in P2_SIZES]
    return out


@pytest.mark.parametrize("name,dtype,B", _p2_params())
def test_batch_gradient_is_the_sum_of_point_gradients(name, dtype, B):
    """P2, for every parameter that receives a gradient (trunk matrices, head matrices, the <= 4-row matrices, biases) and
    for d_t_embed per point where --beta is on (one term: the batch's row against that point's own run).  The batch is the
    first B points of the configuration's point set, so the one-point runs are shared by all sizes.  With P1 a point
    hands the same operands to the weight gradient in any batch - the 8-bit derivative stash is signed-normalised with a
    FIXED scale (d8_pack4 / d8_consts in csrc/field_kernels.h), not a batch-wide one - and in fp16 the coefficients are built
    so that the batch and its one-point runs choose the same loss scale (_make_inputs; the analytic-normal configurations run
    in bf16 only for the reason given there).  The bound is derived, not measured: a 700-term fp32 sum sits near 1e-3 of
    it (5e-4 .. 8e-4 at B = 1100 here), while one point's contribution dropped, repeated or misplaced is about A / B against
    a bound of 2^-23 B A: 1e6 x the bound at B = 2, 1e4 x at B = 63, still 13 .. 100 x at B = 1100 (a mutant of this test
    that leaves the last point out of the batch run failed at every size).
    Where the property does not hold by design: the heads' first layers are evaluated FOLDED with the linear feats layer
    (W1_h Wf), so what the weight-gradient kernels sum over points is M_h = dL/d(W1_h Wf) and s_h; the gradients of
    <head>.0.weight[:, :F], feats_from_xyz.weight and feats_from_xyz.bias are fp32 products of M_h, s_h with the weights,
    taken after that sum (bn_unfold_heads), and their rounding is relative to sum_k |w_k| |M_k|, not to the cancelling
    result (first seen in the fp32 control at B = 2: 3.5e2 x the bound at an element 3000 x smaller than its row's
    typical one).  So the bound above is asserted on M_h and s_h themselves (`folded <head>.0.*`, kept by a wrapper around
    FieldSpec.unfold_grads) and on every other parameter - <head>.0.bias, which is s_h added to zero, and the direction /
    embedding columns of <head>.0.weight included - and those three gradients are held to the same bound carried through
    the unfold's linear map plus that map's own rounding (_unfold_bounds), equally derived.
    With analytic normals every trunk matrix and sigma_from_xyz.0.weight are the sum of TWO jobs, the primal one
    (dz_l^T y_{l-1}) and the adjoint chain's (delta_l^T [gbar_PE ; abar_l]), each summed over the points on its own and
    added in fp32 afterwards (wgrad_reduce_kernel / skinny_reduce_kernel walk the jobs of a matrix in job order).  A
    one-point gradient is the rounded sum p_i + a_i of its two terms, and where they cancel |p_i| + |a_i|, which the
    rounding of the batch sums is relative to, exceeds |p_i + a_i|, which A adds up (seen at B = 2, bf16: 1.2 x the bound
    at F = 64, 26 x at F = 512, at elements a thousand times smaller than their two terms; every larger B passed).  The
    terms are not reported separately, but they can be bounded from what is: the bias of the layer is written by the primal
    job alone, so a one-point run's bias gradient IS dz_l (for sigma: its d pre-activation), and |y| <= 1 for SIREN
    activations and encoded inputs, hence |p_i[n][k]| <= |db_i[n]| and |a_i[n][k]| <= |g_i[n][k]| + |db_i[n]|.  For these
    matrices of the analytic-normal configurations the asserted bound is therefore 2 B 2^-24 (A[n][k] + 2 A_bias[n]);
    every other parameter of those configurations keeps the bound above.
    Also asserted: every gradient of the batch run is finite and the device fault word is 0 afterwards."""
    runs = _point_runs(name, dtype)
    cfg, flags, dpts, dcoef = runs["inputs"]
    G = _backward(runs["model"], flags, _take(dpts, slice(0, B)), dcoef[:B])
    d_t = G.pop("d_t_embed", None)
    S, A = runs["sums"][B]
    assert set(G) == set(S), sorted(set(G) ^ set(S))
    spec = _folded_spec(runs["model"], flags)
    unfolded = _unfold_bounds(runs["model"], spec, B, A)
    # analytic normals: matrices that two jobs add into (primal + adjoint), see the docstring
    two_jobs = {}
    if cfg.normal == "analystic":
        assert cfg.siren and cfg.mapping
        two_jobs = {f"fc_net.{2*l}.weight": f"fc_net.{2*l}.bias" for l in range(cfg.layers)}
        two_jobs["sigma_from_xyz.0.weight"] = "sigma_from_xyz.0.bias"
    worst, bad = (0.0, ""), []
    for k, g in G.items():
        assert bool(torch.isfinite(g).all()), f"{k}: non-finite gradient in the batch run"
        err = (g.cpu().double() - S[k]).abs()
        bound = 2 * B * U24 * A[k] + 1e-30
        if k in unfolded:
            w = unfolded[k].shape[-1]
            bound = bound.clone()
            bound[..., :w] = unfolded[k] + 1e-30        # (columns F.. of a head's first layer, the direction / embedding inputs, are summed over points)
        elif two_jobs and k in two_jobs:
            bound = 2 * B * U24 * (A[k] + 2 * A[two_jobs[k]][:, None]) + 1e-30
        ratio = float((err / bound).max())
        diag(f"P2 {name} {dtype} B={B} {k}{' (unfold bound)' if k in unfolded else ''}: worst |G - S| / bound {ratio:.3e}")
        worst = max(worst, (ratio, k))
        if not ratio <= 1.0:
            i = np.unravel_index(int(torch.argmax(err / bound)), tuple(err.shape))
            bad.append(f"{k}{[int(j) for j in i]}: |G - S| {float(err[i]):.3e} = {ratio:.3e} x bound (G {float(g.cpu()[i]):.6e}, S {float(S[k][i]):.6e})")
    if d_t is not None:
        assert bool(torch.isfinite(d_t).all()), "d_t_embed: non-finite"
        one = runs["d_t"][:B]
        err = (d_t.cpu().double() - one).abs()
        ratio = float((err / (2 * B * U24 * one.abs() + 1e-30)).max())
        diag(f"P2 {name} {dtype} B={B} d_t_embed: worst |G - S| / bound {ratio:.3e}")
        worst = max(worst, (ratio, "d_t_embed"))
        if not ratio <= 1.0:
            bad.append(f"d_t_embed: {ratio:.3e} x bound at point {int(torch.argmax(err.max(1).values))}")
    diag(f"P2 {name} {dtype} B={B}: worst ratio over all parameters {worst[0]:.3e} ({worst[1]})")
    assert not bad, f"{name} {dtype} B={B}: the batch gradient is not the sum of the one-point gradients: " + "; ".join(bad[:6])
    assert _fault_word() == 0


def _oracle_layer_inputs(cfg, p64, xyz):
    """fp64 input vector of every trunk layer ([PE ; y_{l-1}] at the skip layer) and the rounding margin of a ReLU unit."""
    pe = OF.positional_encoding(xyz, cfg.pe_freqs) if cfg.mapping else xyz
    h, ins, mags = pe, [], []
    for l in range(cfg.layers):
        if l in cfg.skips:
            h = torch.cat([pe, h], -1)
        ins.append(h)
        W, b = p64[f"fc_net.{2*l}.weight"], p64[f"fc_net.{2*l}.bias"]
        z = h @ W.T + b
        mags.append(h.abs() @ W.abs().T + b.abs())
        h = torch.sin((30.0 if l == 0 else 1.0) * z) if cfg.siren else torch.relu(z)
    return ins, mags


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", NO_AN)
def test_one_point_trunk_gradient_is_rank_one(name, dtype):
    """P3, on the first 16 one-point runs that P2 makes.  Covered: EVERY trunk matrix fc_net.{2l}.weight, l = 0 .. L-1,
    the first layer and the positional-encoding columns of the skip layer included: in the 16-bit modes wgrad256_kernel
    reads both operands as 16-bit values - A = the dZ_l image the backward chain stores, B = the Y_{l-1} image or the
    positional-encoding rows the forward stores (StashLayout.pe is `T [Mpad][KP]`, csrc/field.h; jobs in
    bn_field_backward, csrc/field_bwd.hip) - multiplies them in the MFMA, adds slabs of zeros and multiplies by the inverse
    loss scale, a power of two (wgrad_reduce_kernel).  No further fp32 rounding: the checks are exact.
    Not covered, and why: sigma_from_xyz / grad_from_xyz / every head's second layer (skinny_wgrad_kernel multiplies a
    16-bit activation by an fp32 d pre-activation: 8 + 24 resp. 11 + 24 significand bits do not fit fp32); feats_from_xyz
    and the heads' first layers (what the kernels accumulate is the gradient of the FOLDED matrix W1 Wf; the parameters'
    gradients come out of bn_unfold_heads' fp32 products); models with analytic normals (a second, adjoint job adds into
    every trunk matrix: rank two).
    With (r, c) the largest entry of G = dW_l, in fp64 (44 significand bits at most): G[n][k] G[r][c] == G[n][c] G[r][k] for
    all n, k; the bias gradient is dz_l, hence db[n] G[r][c] == G[n][c] db[r]; and no column k of G is entirely zero unless
    the fp64 oracle's layer input y[k] is below the type's smallest normal (SIREN and encoded inputs; the number of such
    inputs over the 16 points is printed and asserted to be 0 for these seeds) or, for a ReLU unit, not above the rounding
    margin 4 l eps (|W| |y| + |b|) of its pre-activation in that type (l layers of 16-bit roundings before it, eps = 2^-8 /
    2^-11), while a column whose
    oracle input IS zero (a dead ReLU unit beyond that margin) must be zero."""
    runs = _point_runs(name, dtype)
    cfg, flags, dpts, dcoef = runs["inputs"]
    p64 = tparams(cfg, CASES[name][2], torch.float64)
    ins, mags = _oracle_layer_inputs(cfg, p64, dpts[0][:N_RANK_ONE].cpu().double())
    tiny = float(torch.finfo(torch.bfloat16 if dtype == "bf16" else torch.float16).tiny)
    eps = 2.0 ** -8 if dtype == "bf16" else 2.0 ** -11
    n_cmp = n_small = 0
    for i, gi in enumerate(runs["singles"]):
        for l in range(cfg.layers):
            tag = f"{name} {dtype} point {i} fc_net.{2*l}"
            G, db = gi[f"fc_net.{2*l}.weight"].double(), gi[f"fc_net.{2*l}.bias"].double()
            assert float(G.abs().max()) > 0, f"{tag}: the gradient is all zero"
            r, c = np.unravel_index(int(torch.argmax(G.abs())), tuple(G.shape))
            lhs, rhs = G * G[r, c], G[:, c:c + 1] * G[r:r + 1, :]
            if not torch.equal(lhs, rhs):
                n, k = (lhs != rhs).nonzero()[0].tolist()
                raise AssertionError(f"{tag}.weight is not rank one: G[{n}][{k}] G[{r}][{c}] = {float(lhs[n, k])!r} but G[{n}][{c}] G[{r}][{k}] = "
                                     f"{float(rhs[n, k])!r}; {int((lhs != rhs).sum())} entries, columns {sorted(set((lhs != rhs).nonzero()[:, 1].tolist()))[:20]}")
            assert torch.equal(db * G[r, c], G[:, c] * db[r]), f"{tag}.bias is not proportional to column {c} of the weight gradient"
            n_cmp += G.numel() + db.numel()
            y = ins[l][i]
            zero_col = (G == 0).all(0)
            if cfg.siren or l == 0:
                may_be_zero = y.abs() < tiny
                n_small += int(may_be_zero.sum())
                must_be_zero = torch.zeros_like(may_be_zero)
            else:
                P = ins[l].shape[1] - cfg.feat                     # (encoded-input columns of a skip layer come first)
                margin = 4 * l * eps * mags[l - 1][i]
                may_be_zero = torch.cat([y[:P].abs() < tiny, y[P:] <= margin])
                must_be_zero = torch.cat([torch.zeros(P, dtype=torch.bool), y[P:] == 0]) & torch.cat(
                    [torch.zeros(P, dtype=torch.bool), (ins[l - 1][i] @ p64[f"fc_net.{2*l-2}.weight"].T + p64[f"fc_net.{2*l-2}.bias"]) < -margin])
            assert not bool((zero_col & ~may_be_zero).any()), \
                f"{tag}.weight: columns {(zero_col & ~may_be_zero).nonzero().flatten().tolist()[:20]} are entirely zero, the oracle's inputs there are not"
            assert not bool((must_be_zero & ~zero_col).any()), \
                f"{tag}.weight: columns {(must_be_zero & ~zero_col).nonzero().flatten().tolist()[:20]} of dead ReLU units carry a gradient"
    diag(f"P3 {name} {dtype}: {n_cmp} exact cross-products over {len(runs['singles'])} points x {cfg.layers} layers; "
         f"{n_small} oracle layer inputs below the type's smallest normal")
    assert n_small == 0, f"{n_small} layer inputs below the smallest normal: choose another seed (the zero-column check would be vacuous there)"
