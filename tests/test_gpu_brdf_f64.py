"""The closed-form BRDF code of csrc/brdf_eval.h, in both of its tested instantiations - the per-point kernels of brdf.hip
(bn_brdf_{rpv,hapke,microfacet}_{forward,backward}) and the per-sample launch of sample_brdf.hip (bn_sample_brdf_forward /
_backward) - against the float64 reference of tests/brdf_cases.py: oracle/brdf.py evaluated in float64 on the CPU from the same
float32 inputs, the full 3 x slots Jacobian of every row by autograd.  Tolerances: brdf_cases.TOL, fixed on the CPU from the
oracle's own float32 evaluation (tests/test_brdf_cpu.py); the on-branch (row, quantity) pairs listed in brdf_cases.ILL: their
derived bound."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import brdf_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL_ROWS = 64


@pytest.fixture(scope="module", autouse=True)
def _one_thread():
    """The oracle runs on a few hundred rows at a time: intra-op threads only wait for each other there, and on a busy machine
    that waiting is most of the run time.  One thread while this module runs, the caller's setting after it."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _unit(N, c):
    e = torch.zeros(N, 3, device=DEV)
    e[:, c] = 1
    return e


# ------------------------------------------------------------------------------------------------ the per-point kernels
def _point(variant, tab):
    """The per-point kernels through their autograd wrappers, in the layout of brdf_cases.evaluate."""
    from brdf_nerf_amd import functions as Fn
    s = K.VARIANTS[variant]
    fam, gs = s["family"], K.groups(variant)
    N = tab["l"].shape[0]
    x = {g: tab[g].to(DEV).clone().requires_grad_(True) for g in gs}
    l, v = tab["l"].to(DEV), tab["v"].to(DEV)
    if fam == "rpv":
        brdf, aux = Fn.RPVFunction.apply(l, v, x["n"], x["w"], x.get("k"), x.get("theta"), x.get("rhoc"))
    elif fam == "hapke":
        brdf, aux = Fn.HapkeFunction.apply(l, v, x["n"], x["w"], x.get("b"), x.get("c"), x.get("theta"), s["hpk_scl"], s["shell"])
    else:
        brdf, aux = Fn.MicrofacetFunction.apply(l, v, x["n"], x["albedo"], x["rough"], K.F0)
    leaves = [x[g] for g in gs]
    vjp = lambda d: [g_.reshape(N, -1) for g_ in torch.autograd.grad(brdf, leaves, grad_outputs=d, retain_graph=True)]
    rows = [vjp(_unit(N, c)) for c in range(3)]
    return {"brdf": brdf.detach(), "aux": {q: aux[:, c0:c0 + w] for q, (c0, w) in K.AUX_COLS[fam].items()},
            "jac": {g: torch.stack([rows[c][i] for c in range(3)], 1) for i, g in enumerate(gs)},
            "rnd": dict(zip(gs, vjp(tab["d_brdf"].to(DEV))))}


def _report(tag, e, fam):
    print(tag, {q: f"{v / K.TOL[(fam, q)]:.2f}" if K.TOL[(fam, q)] else f"{v:.0e}/0" for q, (v, _) in e.items()}, "(max error / TOL)")


def _check_well_posed(variant, got, kind="well_posed", rhoc_is_albedo=False):
    fam = K.VARIANTS[variant]["family"]
    tab = K.table(fam, kind)
    e, bad, _ = K.compare(variant, got, K.reference(variant, kind, rhoc_is_albedo), tab, None, rhoc_is_albedo)
    _report(f"{variant} {kind}:", e, fam)
    for q, (v, row) in e.items():
        assert v <= K.TOL[(fam, q)], f"{variant} {kind} row {row}: {q} error {v:.2e} > {K.TOL[(fam, q)]:.0e}"
    assert bad == 0, f"{variant} {kind}: {bad} Jacobian entries that are exactly 0 in the reference are not 0"


def _check_on_branch(variant, got, rhoc_is_albedo=False):
    """Values and aux: the reference's finite / NaN mask, within the bound.  Jacobian: the entries that are finite in float64
    within the bound, exact zeros exact; the others as they come (their count is printed).  The bound of every (row, quantity)
    is TOL, but for the triples of brdf_cases.ILL.  Where a NaN-replaced factor is a group's only path to the value
    (brdf_cases.REPLACED_ZERO) the gradient is exactly 0, whatever autograd says; on the rows of brdf_cases.SUBSTITUTED the
    reference's d / d theta is that of the function with the replacements put in."""
    fam = K.VARIANTS[variant]["family"]
    tab, names = K.on_branch(fam)
    ref = K.reference(variant, "on_branch", rhoc_is_albedo)
    m = K.finite_masks(ref)
    assert torch.equal(torch.isfinite(got["brdf"]).cpu(), m["brdf"]), f"{variant}: finite / NaN mask of the values"
    if got.get("aux") is not None:
        for q, a in got["aux"].items():
            assert torch.equal(torch.isfinite(a).cpu(), m["aux"][q]), f"{variant}: finite / NaN mask of aux {q}"
    skipped = sum(int((~mm).sum()) for mm in m["jac"].values())
    total = sum(int(mm.numel()) for mm in m["jac"].values())
    print(f"{variant} on-branch: {skipped} of {total} Jacobian entries are not finite in float64 and left uncompared")
    e, bad = K.compare_rows(variant, got, ref, tab, names, m, rhoc_is_albedo)
    worst = {}
    for (nm, q), v in e.items():
        bound = K.on_branch_bound(fam, nm, q, rhoc_is_albedo)
        key = q + (" (listed)" if (fam, nm, q) in K.ILL else "")
        worst[key] = max(worst.get(key, 0.0), v / bound if bound else (0.0 if v == 0 else float("inf")))
    print(f"{variant} on-branch:", {q: f"{v:.2f}" for q, v in sorted(worst.items())}, "(max error / bound)")
    for (nm, q), v in e.items():
        bound = K.on_branch_bound(fam, nm, q, rhoc_is_albedo)
        assert v <= bound, f"{variant} on-branch row {nm}: {q} error {v:.2e} > {bound:.0e}"
    assert bad == 0, f"{variant} on-branch: {bad} Jacobian entries that are exactly 0 in the reference are not 0"
    for nm, g in K.replaced_zero(variant):
        r = names.index(nm)
        for what in ("jac", "rnd"):
            t = got[what][g][r].cpu()
            assert bool((t == 0).all()), f"{variant} on-branch row {nm}: d_{g} through the replaced factor is {t.flatten().tolist()}, not 0"
    if "replaced_brdf" in ref:
        rows = ref["replaced_brdf"][0]
        assert bool(torch.isfinite(got["jac"]["theta"][rows]).all()) and bool(m["jac"]["theta"][rows].all())


@pytest.mark.parametrize("variant", list(K.VARIANTS))
def test_point_kernels_well_posed(variant):
    _check_well_posed(variant, _point(variant, K.table(K.VARIANTS[variant]["family"])))


@pytest.mark.parametrize("variant", list(K.VARIANTS))
def test_point_kernels_on_branch(variant):
    _check_on_branch(variant, _point(variant, K.table(K.VARIANTS[variant]["family"], "on_branch")))


# ------------------------------------------------------------------------------------------------ tail guard, optional outputs
def _raw_call(fam, tab, N, drop=None, spec=None):
    """Forward and backward through the C entry points on the first N rows, outputs SENTINEL_ROWS longer and NaN-filled.
    drop: the name of one d_* output passed as NULL.  -> {name: buffer}."""
    from brdf_nerf_amd import _lib as L
    lib = L.lib()
    names = {"rpv": ["n", "w", "k", "theta", "rhoc"], "hapke": ["n", "w", "b", "c", "theta"], "microfacet": ["n", "albedo", "rough"]}[fam]
    x = {g: tab[g][:N].to(DEV).contiguous() for g in names + ["l", "v", "d_brdf"]}
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    buf = lambda t: torch.full((N + SENTINEL_ROWS,) + tuple(t.shape[1:]), float("nan"), device=DEV)
    out = {"brdf": buf(x["d_brdf"]), "aux": torch.full((N + SENTINEL_ROWS, L.BN_BRDF_AUX), float("nan"), device=DEV)}
    out.update({"d_" + g: buf(x[g]) for g in names if g != drop})
    d = lambda g: vp(out.get("d_" + g))
    if fam == "rpv":
        a = [vp(x[g]) for g in ("l", "v", "n", "w", "k", "theta", "rhoc")]
        assert lib.bn_brdf_rpv_forward(*a, N, vp(out["brdf"]), vp(out["aux"]), None) == 0
        assert lib.bn_brdf_rpv_backward(*a, vp(x["d_brdf"]), N, d("n"), d("w"), d("k"), d("theta"), d("rhoc"), None) == 0
    elif fam == "hapke":
        a = [vp(x[g]) for g in ("l", "v", "n", "w", "b", "c", "theta")] + [4.0, 0]
        assert lib.bn_brdf_hapke_forward(*a, N, vp(out["brdf"]), vp(out["aux"]), None) == 0
        assert lib.bn_brdf_hapke_backward(*a, vp(x["d_brdf"]), N, d("n"), d("w"), d("b"), d("c"), d("theta"), None) == 0
    else:
        a = [vp(x[g]) for g in ("l", "v", "n", "albedo", "rough")] + [K.F0]
        assert lib.bn_brdf_microfacet_forward(*a, N, vp(out["brdf"]), vp(out["aux"]), None) == 0
        assert lib.bn_brdf_microfacet_backward(*a, vp(x["d_brdf"]), N, d("n"), d("albedo"), d("rough"), None) == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("family", K.FAMILIES)
def test_tail_guard_and_optional_outputs(family):
    """The block is 128 rows: N on either side of one and two blocks.  Rows at N and beyond keep the NaN sentinel; every d_*
    pointer NULL in turn leaves the others bit-equal; the first 129 rows of a 257-row call are bit-equal to the 129-row call."""
    tab = K.table(family)
    full = {}
    for N in (1, 127, 128, 129, 257):
        full[N] = o = _raw_call(family, tab, N)
        for nm, t in o.items():
            assert bool(torch.isfinite(t[:N]).all()), (N, nm)
            assert bool(torch.isnan(t[N:]).all()), f"{family} N={N}: {nm} was written at row N or beyond"
        for drop in [nm[2:] for nm in o if nm.startswith("d_")]:
            p = _raw_call(family, tab, N, drop)
            assert "d_" + drop not in p
            for nm, t in p.items():
                assert torch.equal(t[:N], o[nm][:N]) and bool(torch.isnan(t[N:]).all()), (N, drop, nm)
    for nm, t in full[129].items():
        assert torch.equal(t[:129], full[257][nm][:129]), nm
    # and the full call is the well-posed comparison's own numbers
    assert torch.equal(full[257]["brdf"][:257], _point({"rpv": "rpv/ktr", "hapke": "hapke/bct/4.0", "microfacet": "microfacet"}[family],
                                                        {k: a[:257] for k, a in tab.items()})["brdf"])


# ------------------------------------------------------------------------------------------------ the per-sample launch
_HEAD_ORDER = {"rpv": ("k", "theta", "rhoc"), "hapke": ("b", "c", "theta"), "microfacet": ("rough",)}
CH_N = 6                                     # row layout: [albedo 3, sigma, 2 spare channels, normal 3, heads ...]


def _sample(variant, tab, rhoc_is_albedo=False, two_block=False):
    """bn_sample_brdf_forward / _backward on the table laid out as field-output rows: one ray per row (S1 = 1, S2 = 0), or the
    two-block layout of brdf_cases.two_block.  rgb_padding = 0 and no irradiance: the launch's affine step b = (brdf (1 + 2 pad) -
    pad) irr is brdf * 1 - 0, exact.  -> the layout of brdf_cases.evaluate, without aux."""
    from brdf_nerf_amd import _lib as L, functions as Fn
    s = K.VARIANTS[variant]
    fam, gs = s["family"], K.groups(variant, rhoc_is_albedo)
    N = tab["n"].shape[0]
    alb = "albedo" if fam == "microfacet" else "w"
    cols, Cc = {"n": (CH_N, 3), alb: (0, 3)}, CH_N + 3
    for g in _HEAD_ORDER[fam]:
        if g in gs:
            w = tab[g].reshape(N, -1).shape[1]
            cols[g] = (Cc, w)
            Cc += w
    g0 = torch.Generator().manual_seed(11)
    X = torch.rand(N, Cc, generator=g0)                                # sigma and the spare channels: anything
    for g, (c0, w) in cols.items():
        X[:, c0:c0 + w] = tab[g].reshape(N, -1)
    if two_block:
        R, S1, S2 = K.TWO_BLOCK["R"], K.TWO_BLOCK["S1"], K.TWO_BLOCK["S2"]
        ray_l, ray_v = tab["ray_l"], tab["ray_v"]
    else:
        R, S1, S2 = N, 1, 0
        ray_l, ray_v = tab["l"], tab["v"]
    rays = torch.rand(R, 11, generator=g0)
    rays[:, 3:6], rays[:, 8:11] = -ray_v, ray_l
    X, rays = X.to(DEV).contiguous(), rays.to(DEV).contiguous()
    d = L.ShadeDesc()
    d.kind = {"rpv": L.BN_SHADE_RPV, "hapke": L.BN_SHADE_HAPKE, "microfacet": L.BN_SHADE_MICROFACET}[fam]
    d.C, d.ch_normal = Cc, CH_N
    p = [cols[g][0] if g in cols else -1 for g in _HEAD_ORDER[fam]] + [-1, -1]
    d.ch_p0, d.ch_p1, d.ch_p2 = p[0], p[1], p[2]
    d.rhoc_is_albedo, d.shell, d.cos_irradiance, d.usealldepth = int(rhoc_is_albedo), s.get("shell", 0), 0, 0
    d.hpk_scl, d.f0, d.rgb_padding = s.get("hpk_scl", 1.0), K.F0, 0.0
    d.lambda_rgb = d.lambda_ds = d.lambda_hs = 0.0
    d.irr, d.irr_stride = None, 0
    n1 = R * S1
    B = torch.full((N, 4), float("nan"), device=DEV)
    Fn.sample_brdf(d, X, rays, n1, S1, S2, B)
    assert torch.equal(B[:, 3], X[:, 3])

    def vjp(d_brdf):
        dB = torch.cat([d_brdf, torch.zeros(N, 1, device=DEV)], 1).contiguous()
        dX = torch.full((N, Cc), float("nan"), device=DEV)
        Fn.sample_brdf(d, X, rays, n1, S1, S2, dX, backward_of=dB)
        # sigma passes through, the spare channels (no head reads them) get an exact zero
        assert float(dX[:, 3:CH_N].abs().max()) == 0.0
        return [dX[:, cols[g][0]:cols[g][0] + cols[g][1]] for g in gs]

    rows = [vjp(_unit(N, c)) for c in range(3)]
    return {"brdf": B[:, :3], "jac": {g: torch.stack([rows[c][i] for c in range(3)], 1) for i, g in enumerate(gs)},
            "rnd": dict(zip(gs, vjp(tab["d_brdf"].to(DEV))))}


@pytest.mark.parametrize("variant", list(K.VARIANTS))
def test_sample_launch_well_posed_and_on_branch(variant):
    fam = K.VARIANTS[variant]["family"]
    _check_well_posed(variant, _sample(variant, K.table(fam)))
    _check_on_branch(variant, _sample(variant, K.table(fam, "on_branch")))


def test_sample_launch_rhoc_is_albedo():
    """funcH == 2: the albedo seeds its own slot and rhoc's; its gradient is the sum of both, the reference's w is both inputs."""
    _check_well_posed("rpv/kt", _sample("rpv/kt", K.table("rpv"), rhoc_is_albedo=True), rhoc_is_albedo=True)
    _check_on_branch("rpv/kt", _sample("rpv/kt", K.table("rpv", "on_branch"), rhoc_is_albedo=True), rhoc_is_albedo=True)
    # it is another function than rpv/kt without rhoc, and than rpv/ktr with the table's rhoc
    a, b = K.reference("rpv/kt", "well_posed", True), K.reference("rpv/kt", "well_posed")
    assert K.err_jac(a["jac"]["w"], b["jac"]["w"])[0] > 1e-2


@pytest.mark.parametrize("variant", ["rpv/ktr", "hapke/bct/4.0"])
def test_sample_launch_two_blocks(variant):
    """S1 = 3, S2 = 2, 37 rays: rows of block 1 take ray row / 3, rows of block 2 ray (row - 111) / 2; the reference is the
    float64 oracle on the gathered directions."""
    fam = K.VARIANTS[variant]["family"]
    _check_well_posed(variant, _sample(variant, K.table(fam, "two_block"), two_block=True), "two_block")
