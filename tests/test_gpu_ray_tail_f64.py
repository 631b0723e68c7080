"""The ray tail - csrc/ray_tail.hip (ray_shade_loss_kernel<KIND> behind bn_ray_shade_loss) and lambert_loss_kernel of
csrc/render_kernels.hip (bn_lambert_loss) - against the float64 reference of tests/ray_tail_cases.py: rendering.shade_ray + losses
restated with the BRDF of oracle/brdf.py, evaluated in float64 on the CPU from the same float32 inputs, gradients by autograd.
Tolerances: ray_tail_cases.TOL, fixed on the CPU from the reference's own float32 evaluation (tests/test_ray_tail_cpu.py); the
on-branch triples of ray_tail_cases.ILL: their derived bound.  Every output buffer is NaN-filled and 64 rows longer than the
launch: "written" and "not written beyond R" are part of each comparison."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_tail_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
OUTS = ("rgb", "ray_loss", "d_acc", "d_wsum", "d_depth")


@pytest.fixture(scope="module", autouse=True)
def _one_thread():
    """The reference runs on a few hundred rays at a time: intra-op threads only wait for each other there.  One thread while this
    module runs, the caller's setting after it."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _run(c, forms=None, acc=None, extra="case", nonfinite=None, desc=None):
    """bn_ray_shade_loss on a case through Fn.ray_shade_loss.  forms: overrides of the case's operand forms (strided / prior / irr);
    acc, extra, desc: overrides of the inputs.  -> the outputs' first R rows, loss_acc [slots] and loss = its sum; asserts that the
    SENTINEL_ROWS rows beyond R of every output, and the entries of loss_acc beyond the slots, still hold their NaN."""
    from brdf_nerf_amd import functions as Fn
    R, S, slots = c["R"], T.SENTINEL_ROWS, c["slots"]
    d = T.copy_desc(c["desc"] if desc is None else desc)
    f = dict(strided=c["strided"], prior=c["prior"], irr=c["irr_form"])
    f.update(forms or {})
    rays = c["rays"].to(DEV)
    rd, sd = rays[:, 3:6], rays[:, 8:11]
    if not f["strided"]:
        rd, sd = rd.contiguous(), sd.contiguous()
    pr = [None] * 4
    if f["prior"] != "off":
        pt = c["ptab"].to(DEV)
        pr = [pt[:, i] if f["prior"] == "strided" else pt[:, i].contiguous() for i in range(4)]
    if f["irr"] is not None:
        it = c["irr"].to(DEV)
        iv = it[:, 0] if f["irr"] == "strided" else it[:, 0].contiguous()
        assert iv.stride(0) == (2 if f["irr"] == "strided" else 1)
        d.irr, d.irr_stride, d._keep = iv.data_ptr(), (iv.stride(0) if R > 1 else 1), iv
    full = {k: torch.full((R + S,) + sh, NAN, device=DEV) for k, sh in
            (("rgb", (3,)), ("d_acc", (d.C,)), ("d_wsum", ()), ("d_depth", ()), ("ray_loss", ()))}
    lacc = torch.cat([torch.zeros(slots), torch.full((S,), NAN)]).to(DEV)
    ex = (c["extra"] if c["use_extra"] else None) if isinstance(extra, str) else extra
    Fn.ray_shade_loss(d, (c["acc"] if acc is None else acc).to(DEV).contiguous(), c["wsum"].to(DEV), c["depth"].to(DEV), c["var"].to(DEV), rd,
                      None if c["sun_none"] else sd, c["rgbs"].to(DEV), {k: full[k][:R] for k in ("rgb", "d_acc", "d_wsum", "d_depth")},
                      pr[0], pr[1], pr[2], pr[3], ray_loss=full["ray_loss"][:R], loss_acc=lacc[:slots], nonfinite=nonfinite,
                      extra_loss=None if ex is None else ex.to(DEV))
    torch.cuda.synchronize()
    for k, t in full.items():
        assert bool(torch.isnan(t[R:]).all()), f"{c['name']}: {k} was written at row R or beyond"
    assert bool(torch.isnan(lacc[slots:]).all()), f"{c['name']}: loss_acc was written beyond its {slots} slots"
    out = {k: t[:R].cpu() for k, t in full.items()}
    out["loss_acc"] = lacc[:slots].cpu()
    out["loss"] = lacc[:slots].sum().cpu()
    return out


def _hold(name, e, kind, bound=None):
    print(name, {q: f"{v / T.TOL[(kind, q)]:.2f}" for q, (v, _) in e.items()}, "(max error / TOL)")
    for q, (v, row) in e.items():
        tol = T.TOL[(kind, q)] if bound is None else bound(q)
        assert v <= tol, f"{name} row {row}: {q} error {v:.2e} > {tol:.0e}"


# ------------------------------------------------------------------------------------------------ the well-posed tables
@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_well_posed(name):
    """rgb, ray_loss, loss_acc per slot, the batch loss, d_acc per input group, d_wsum and d_depth within TOL of the float64
    reference; every entry written; the channels that the kind does not read exactly 0."""
    c = T.case(name)
    got, ref = _run(c), T.reference(name)
    for k in OUTS + ("loss_acc",):
        assert bool(torch.isfinite(got[k]).all()), f"{name}: {k} holds entries that were not written or are not finite"
    assert T.nonzero_unread(got["d_acc"], c["desc"]) == 0, f"{name}: channels {T.unread_channels(c['desc'])} of d_acc must be exactly 0"
    _hold(name, T.compare(got, ref, c["desc"]), T.kind_of(c["desc"]))


# ------------------------------------------------------------------------------------------------ the on-branch tables
@pytest.mark.parametrize("name", T.ON_BRANCH)
def test_on_branch(name):
    """Rows exactly on a switch: held to TOL (the triples of ILL: their derived bound) on what is finite in float64; what is not
    is exactly 0 where a replaced factor is the only path (REPLACED_ZERO) and non-finite on the device elsewhere; the arm itself
    (the clamp passes the gradient on 0 and on 1 and not outside, the gate is strict) read off the gradients."""
    c, names = T.on_branch(name)
    d, kind = c["desc"], T.kind_of(c["desc"])
    got, ref = _run(c), T.ob_reference(c, torch.float64)
    m = T.finite_masks(ref)
    zero = torch.zeros_like(m["d_acc"])
    for (tab, nm), gs in T.REPLACED_ZERO.items():
        if tab == name:
            for g in gs:
                c0, w = T.groups_of(d)[g]
                zero[names.index(nm), c0:c0 + w] = True
    assert bool((got["d_acc"][zero] == 0).all()), f"{name}: the gradient through a replaced factor is {got['d_acc'][zero].tolist()}, not 0"
    for q in OUTS + ("loss_acc",):
        bad = ~m[q] if q != "d_acc" else ~m[q] & ~zero
        assert not bool(torch.isfinite(got[q][bad]).any()), f"{name}: {q} is finite where the float64 reference is not"
        assert bool(torch.isfinite(got[q][m[q]]).all()), f"{name}: {q} is not finite where the float64 reference is"
    assert T.nonzero_unread(got["d_acc"], d) == 0
    e = T.compare_rows(c, names, got, ref, m)
    print(name, {f"{nm}:{q}": f"{v / T.on_branch_bound(name, nm, q) if nm != '*' else v / T.TOL[(kind, q)]:.2f}" for (nm, q), v in e.items() if v},
          "(error / bound)")
    for (nm, q), v in e.items():
        bound = T.TOL[(kind, q)] if nm == "*" else T.on_branch_bound(name, nm, q)
        assert v <= bound, f"{name} row {nm}: {q} error {v:.2e} > {bound:.0e}"
    if kind == "lambert":
        depth, ws = c["depth"].double(), c["wsum"].double()
        hs_only = -2 * (d.lambda_hs / c["R"]) * (depth - depth * ws)
        for i, nm in enumerate(names):
            want = T.EXPECTED_TRACE[nm]
            assert bool((got["d_depth"][i].double() - hs_only[i]).abs() > 1e-6) == want["applied"], f"{name} row {nm}: the depth term"
            if "passes" in want:
                assert tuple(bool(v != 0) for v in got["d_acc"][i, :3]) == want["passes"], f"{name} row {nm}: the clamp's gradient"
    else:
        i = names.index("n_below_eps")            # the clamped normaliser is a constant: d normal_s / d n = 1 / sqrt(eps), no radial part
        for j in ("n_zero", "n_below_eps"):
            assert bool(torch.isfinite(got["rgb"][names.index(j)]).all())
        assert bool(torch.isfinite(got["d_acc"][i]).all())


# ------------------------------------------------------------------------------------------------ the dropping rule
@pytest.mark.parametrize("name", ["hapke_bct_model_R130", "identity_R65", "microfacet_model_R130"])
def test_non_finite_rays_are_dropped_and_counted_only_when_asked(name):
    """NaN planted through acc and +Inf through extra_loss, among them ray 0, 63, 64 and the last.  Without `nonfinite` the loss is
    not finite, the NaN rays' gradients are not finite and the Inf rays' terms are +Inf (extra_loss reaches no gradient).  With it:
    counts == [n_nan, n_inf], those rays' ray_loss, d_acc, d_wsum and d_depth exactly 0, every other ray bitwise the clean run,
    loss_acc the clean per-slot sums without the dropped rays' terms."""
    c = T.case(name)
    R, slots = c["R"], c["slots"]
    assert c["use_extra"] and R >= 65
    nan_rays = [0, 64, 37]
    inf_rays = [r for r in (63, R - 1, 5) if r not in nan_rays]
    acc, extra = c["acc"].clone(), c["extra"].clone()
    acc[nan_rays, 0] = NAN
    extra[inf_rays] = float("inf")
    clean = _run(c)
    k0 = _run(c, acc=acc, extra=extra)
    assert not bool(torch.isfinite(k0["loss"])) and not bool(torch.isfinite(k0["ray_loss"][nan_rays + inf_rays]).any())
    assert bool((k0["ray_loss"][inf_rays] == float("inf")).all())
    # which rays' gradients that NaN reaches is the reference's to say (a clamp passes nothing on from a NaN colour: the Lambertian
    # kinds and the microfacet's albedo + glossy keep a finite gradient beside the NaN loss; Hapke does not).  Per ray, not per
    # entry: reverse mode multiplies the zero it sends back by the NaN local derivatives of the whole chain, forward mode only
    # where the dual itself is NaN
    bad = T.case_reference(c, torch.float64, acc=acc, extra_loss=extra)
    fin = lambda t: torch.isfinite(t).all(-1)
    assert torch.equal(fin(k0["d_acc"]), fin(bad["d_acc"])), f"{name}: the rays whose d_acc is not finite are not the reference's"
    assert not bool(torch.isfinite(bad["loss"])) and (T.kind_of(c["desc"]) != "hapke" or not bool(torch.isfinite(bad["d_acc"][nan_rays]).all(-1).any()))
    cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    k1 = _run(c, acc=acc, extra=extra, nonfinite=cnt)
    assert cnt.tolist() == [len(nan_rays), len(inf_rays)]
    dropped = torch.zeros(R, dtype=torch.bool)
    dropped[nan_rays + inf_rays] = True
    for q in ("ray_loss", "d_acc", "d_wsum", "d_depth"):
        assert bool((k1[q][dropped] == 0).all()), f"{name}: {q} of a dropped ray is not exactly 0"
        assert torch.equal(k1[q][~dropped], clean[q][~dropped]), f"{name}: {q} of a kept ray differs from the clean run"
    # (rgb is written before the ray is dropped: it is the clamped value, NaN where acc was)
    assert torch.equal(k1["rgb"][~dropped], clean["rgb"][~dropped])
    ref = T.reference(name)
    kept = torch.where(dropped, torch.zeros_like(ref["ray_loss"]), ref["ray_loss"])
    want = torch.zeros(slots, dtype=torch.float64).index_add_(0, torch.arange(R) % slots, kept)
    _hold(name + " kept", T.compare({"loss_acc": k1["loss_acc"], "loss": k1["loss"]}, {"loss_acc": want, "loss": want.sum()}, c["desc"]),
          T.kind_of(c["desc"]))
    # and with nothing to drop the counters stay 0 and nothing changes
    cnt.zero_()
    k2 = _run(c, nonfinite=cnt)
    assert cnt.tolist() == [0, 0] and all(torch.equal(k2[q], clean[q]) for q in OUTS)


# ------------------------------------------------------------------------------------------------ layout invariance
def _slot_sums_agree(name, c, a, b):
    """loss_acc of two launches on the same per-ray terms: bitwise where a slot holds one ray; where it holds several the atomic
    adds arrive in any order, and both launches are held to the reference instead."""
    if c["R"] <= c["slots"]:
        assert torch.equal(a["loss_acc"], b["loss_acc"]), f"{name}: loss_acc"
    else:
        for o in (a, b):
            _hold(name + " loss_acc", T.compare({"loss_acc": o["loss_acc"]}, T.reference(name), c["desc"]), T.kind_of(c["desc"]))


@pytest.mark.parametrize("name", ["rpv_ktr_model_R130", "hapke_bc_far_R64", "microfacet_far_R65", "lambert_irr_R130", "lambert_ncos_R63", "lambert_ncos_sunnone_R64"])
def test_strided_views_and_contiguous_copies_give_the_same_bits(name):
    c = T.case(name)
    has = lambda k: None if c[k] is None else "strided"
    a = _run(c, forms=dict(strided=True, prior="strided" if c["prior"] != "off" else "off", irr=has("irr_form")))
    b = _run(c, forms=dict(strided=False, prior="contiguous" if c["prior"] != "off" else "off", irr=None if c["irr_form"] is None else "contiguous"))
    for q in OUTS:
        assert torch.equal(a[q], b[q]), f"{name}: {q} depends on the operands' strides"
    _slot_sums_agree(name, c, a, b)


_PERMUTED = {   # case -> the same groups at other channels (group: new first channel); the channels left over keep their order
    "rpv_ktr_model_R130": dict(theta=4, rhoc=7, normal=10, k=13),
    "hapke_bct_model_R130": dict(theta=4, normal=5, c=8, b=11),
    "microfacet_model_R130": dict(rough=4, normal=5),
    "rpv_t_bothnormals_model_R65": dict(normal=4, theta=10),        # the winning field takes the losing field's place
}


@pytest.mark.parametrize("name", list(_PERMUTED))
def test_a_permuted_channel_layout_gives_the_permuted_gradient_bitwise(name):
    c = T.case(name)
    d0 = c["desc"]
    g0, new = T.groups_of(d0), _PERMUTED[name]
    perm = torch.full((d0.C,), -1, dtype=torch.long)              # perm[new channel] = old channel
    perm[:4] = torch.arange(4)
    for g, n0 in new.items():
        c0, w = g0[g]
        perm[n0:n0 + w] = torch.arange(c0, c0 + w)
    rest = [ch for ch in range(d0.C) if ch not in perm.tolist()]
    perm[perm < 0] = torch.tensor(rest, dtype=torch.long)
    assert sorted(perm.tolist()) == list(range(d0.C))
    d1 = T.copy_desc(d0)
    d1.ch_normal = new["normal"]
    heads = {"rpv": ("k", "theta", "rhoc"), "hapke": ("b", "c", "theta"), "microfacet": ("rough",)}[T.kind_of(d0)]
    for field, h in zip(("ch_p0", "ch_p1", "ch_p2"), heads):
        if h in new:
            setattr(d1, field, new[h])
    assert {g: w for g, (_, w) in T.groups_of(d1).items()} == {g: w for g, (_, w) in g0.items()}
    a, b = _run(c), _run(c, acc=c["acc"][:, perm], desc=d1)
    assert torch.equal(b["d_acc"], a["d_acc"][:, perm])
    for q in ("rgb", "ray_loss", "d_wsum", "d_depth"):
        assert torch.equal(a[q], b[q]), q
    _slot_sums_agree(name, c, a, b)


# ------------------------------------------------------------------------------------------------ bn_lambert_loss
@pytest.mark.parametrize("name", list(T.LL_CASES))
def test_lambert_loss(name):
    """The general step's Lambert tail (a wave per ray, lanes stride the samples) against the reference's Lambert arm on wsum and
    var formed from weights and z: rgb, the loss, d_acc[:3], d_depth; d_weights constant along a ray and the reference's d_wsum;
    d_acc[c >= 3] exactly 0."""
    from brdf_nerf_amd import functions as Fn
    c = T.ll_case(name)
    dv = lambda t: t.to(DEV).contiguous()
    p = c["ptab"]
    on = c["prior"] != "off"
    loss, rgb, d_acc, d_depth, d_w = Fn.lambert_loss(dv(c["acc"]), dv(c["weights"]), dv(c["z"]), dv(c["depth"]), dv(c["rgbs"]), T.PAD, T.LAM_RGB,
                                                     dv(p[:, 0]) if on else None, dv(p[:, 1]) if on else None, dv(p[:, 2]) if on else None,
                                                     dv(p[:, 3]) if on else None, T.LAM_DS if on else 0.0, c["prior"] == "all")
    torch.cuda.synchronize()
    assert d_w.shape == (c["R"], c["S"]) and d_acc.shape == (c["R"], c["C"])
    assert bool((d_w == d_w[:, :1]).all()), "d_weights varies along a ray"
    assert bool((d_acc[:, 3:] == 0).all()), "d_acc beyond the colour is not exactly 0"
    got = {"rgb": rgb.cpu(), "loss": loss.cpu(), "d_acc": d_acc.cpu(), "d_depth": d_depth.cpu(), "d_wsum": d_w[:, 0].cpu()}
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    _hold("lambert_loss " + name, T.compare(got, T.ll_reference64(name), T.ll_desc(c)), "lambert")
