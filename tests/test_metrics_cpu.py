"""CPU tests of the image and normal metrics (brdf_nerf_amd/metrics.py): the float64 statements of tests/metric_cases.py checked
against independent formulations before they measure the kernels, the two SSIM layouts, the refusals, image_psnr and the ABI."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metric_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _conv_ssim(pred, gt, mask, div, max_val, window):
    """SSIM by torch ops in float64: F.pad(mode='reflect') + F.conv2d with the outer product of the Gaussian weights."""
    C, H, W = pred.shape
    m = torch.ones(H, W, dtype=torch.float64) if mask is None else torch.from_numpy(mask.astype(np.float64))
    x = (torch.from_numpy(pred.astype(np.float64)) * m / div).reshape(C, 1, H, W)
    y = (torch.from_numpy(gt.astype(np.float64)) * m / div).reshape(C, 1, H, W)
    g = torch.from_numpy(M.gaussian(window))
    k = torch.outer(g, g).reshape(1, 1, window, window)
    pad = window // 2
    f = lambda t: F.conv2d(F.pad(t, (pad, pad, pad, pad), mode="reflect"), k)
    mx, my, exx, eyy, exy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    C1, C2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    v = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2) + 1e-12)
    return v.reshape(C, H, W).numpy()


@pytest.mark.parametrize("name", [n for n in M.SSIM_CASES if n not in M.MAX_VAL])
def test_ssim_statement_agrees_with_pad_and_conv2d(name):
    """The tap-loop statement against reflect padding + conv2d in float64, to 1e-12 (the two differ in the order of the sums
    only), NaN cells in the same places.  The ill-conditioned case is built to amplify exactly that difference and is left out."""
    c = M.ssim_case(name)
    P = lambda k: M.planes(c[k], c["layout"], c["C"], c["H"], c["W"])
    want = _conv_ssim(P("pred"), P("gt"), c["mask"], c["div"], c["max_val"], c["window"])
    got = M.ssim_expected(name)["v"]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    err = float(np.nanmax(np.abs(got - want))) if not np.isnan(got).all() else 0.0
    print(f"{name}: statement - conv2d max abs {err:.2e}")
    assert err <= 1e-12


def test_the_two_layouts_address_the_stated_elements():
    """'reference' is eval.py:471's .view(1, 3, H, W) of the (H W, 3) buffer - plane c = flat[c H W : (c + 1) H W], NOT channel c;
    'image' is the permuted true image.  The library's strides are the statement's."""
    from brdf_nerf_amd.metrics import layout_strides
    C, H, W = 3, 5, 7
    buf = torch.arange(H * W * C, dtype=torch.float32).reshape(H * W, C)
    flat = buf.numpy().reshape(-1)
    ref = M.planes(flat, "reference", C, H, W)
    img = M.planes(flat, "image", C, H, W)
    assert np.array_equal(ref, buf.view(1, C, H, W)[0].numpy())
    assert np.array_equal(ref, flat.reshape(C, H * W).reshape(C, H, W)) and ref[1, 0, 0] == H * W
    assert np.array_equal(img, buf.reshape(H, W, C).permute(2, 0, 1).numpy()) and img[1, 0, 0] == 1 and img[0, 0, 1] == C
    for layout in ("reference", "image"):
        assert layout_strides(layout, C, H, W) == M.strides(layout, C, H, W)
    assert layout_strides("reference", C, H, W) == (H * W, W, 1) and layout_strides("image", C, H, W) == (1, C * W, C)
    with pytest.raises(ValueError, match="layout"):
        layout_strides("planar", C, H, W)


def test_gaussian_weights():
    from brdf_nerf_amd.metrics import gaussian_window
    for w in (3, 5, 7, 9, 11):
        g = M.gaussian(w)
        assert g.shape == (w,) and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == w // 2
        assert gaussian_window(w) == g.tolist()
    assert M.gaussian(3)[1] / M.gaussian(3)[0] == pytest.approx(np.exp(1.0 / 4.5), rel=1e-15)


def test_the_ssim_cases_hold_what_they_promise():
    """The yardstick before it measures: reflect indices, the NaN pixel's window^2 skipped cells, the degenerate inputs, split
    invariance of the integer sums, and the two perturbations the GPU test must be able to see."""
    assert M.reflect_index(5, 2).tolist() == [2, 1, 0, 1, 2, 3, 4, 3, 2] and M.reflect_index(2, 1).tolist() == [1, 0, 1, 0]
    for name, w in (("nan_pixel_16x18_w3", 3), ("nan_pixel_16x18_w5", 5)):
        e = M.ssim_expected(name)
        assert e["sums"][2] == w * w and e["sums"][1] == 3 * 16 * 18 - w * w
        assert int(np.isnan(e["map"]).sum()) == w * w and np.isnan(e["map"][M.NAN_AT])
    e = M.ssim_expected("gt_zero_16x18")
    assert M.ssim_case("gt_zero_16x18")["max_val"] == 0.0 and e["sums"] == (0, 864, 0) and not e["v"].any()
    assert M.ssim_expected("gt_zero_16x18_scl")["sums"] == (0, 0, 864)          # div = 0: 0 / 0 everywhere
    e = M.ssim_expected("identical_16x18")
    assert abs(e["sums"][0] / (e["sums"][1] * M.SSIM_FIX) - 1.0) < 1e-9
    assert M.ssim_case("large_1e4_16x18")["max_val"] > 9.0e3
    for name in M.SSIM_CASES:
        c, e = M.ssim_case(name), M.ssim_expected(name)
        assert e["v"].shape == (c["C"], c["H"], c["W"]) and e["sums"][1] + e["sums"][2] == e["v"].size
    # any partition of the rows adds up to the whole, in integers
    v = M.ssim_expected("33x31_w11")["v"]
    for cuts in ([0, 1, 33], [0, 16, 33], list(range(34))):
        parts = [M.ssim_sums(v, (a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
        assert tuple(sum(p[k] for p in parts) for k in range(3)) == M.ssim_expected("33x31_w11")["sums"]
    # edge-repeat padding changes both perturbation cases; a column-major tap order the ill-conditioned one
    for name in M.PERTURBATION_CASES:
        c, e = M.ssim_case(name), M.ssim_expected(name)
        P = lambda k: M.planes(c[k], c["layout"], c["C"], c["H"], c["W"])
        edge = M.ssim_map(P("pred"), P("gt"), c["mask"], c["div"], c["max_val"], c["window"], c["g"], pad_index=M.edge_index)
        assert not np.array_equal(edge.astype(np.float32), e["map"]) and M.ssim_sums(edge) != e["sums"]
    c, e = M.ssim_case("3x5_w3_illcond"), M.ssim_expected("3x5_w3_illcond")
    P = lambda k: M.planes(c[k], c["layout"], c["C"], c["H"], c["W"])
    col = M.ssim_map(P("pred"), P("gt"), c["mask"], c["div"], c["max_val"], c["window"], c["g"], column_major=True)
    assert not np.array_equal(col.astype(np.float32), e["map"]) and M.ssim_sums(col) != e["sums"]


def test_a_tilted_plane_has_its_closed_form_normal():
    """z = a x + b y + d: every interior normal is (a, b, -1) / sqrt(1 + a^2 + b^2) to 1e-12 - with the reference's axes (y grows
    with the row) flat ground gives n_z = -1 - and the border is zero."""
    a, b, res = M.PLANE
    n = M.normals(M.normal_case("plane_6x7")[1], res, as_float32=False)
    want = M.plane_normal(a, b)
    assert np.abs(n[1:-1, 1:-1] - want).max() <= 1e-12
    assert not n[0].any() and not n[-1].any() and not n[:, 0].any() and not n[:, -1].any()
    flat = M.normals(M.normal_case("flat_5x5")[1], 0.5, as_float32=False)
    assert np.array_equal(flat[1:-1, 1:-1], np.broadcast_to([0.0, 0.0, -1.0], (3, 3, 3)))
    # a NaN altitude reaches its own normal and its four neighbours', nothing else; a grid without an interior is all zero
    nan = M.normals_expected("nan_9x8")
    assert int(np.isnan(nan).any(-1).sum()) == 5 and np.isnan(nan[4, 3]).all() and np.isnan(nan[3, 3]).all()
    assert not M.normals_expected("2x5").any()
    # equal grids: 90 on the reference's border (zero normals), NaN there with border = 1; inside the angle is 0 up to the float32
    # rounding of the normals (|n|^2 = 1 +- 1.2e-7 and arccos is steep at 1: at most sqrt(2.4e-7) rad = 0.03 degrees), as upstream
    n33 = M.normals_expected("3x3")
    ang = M.angle_map(n33, n33, 0)
    assert 0.0 <= ang[1, 1] < 0.03 and np.all(np.delete(ang.ravel(), 4) == 90.0)
    q = int(np.rint(ang[1, 1] * 2 ** 20))
    assert M.angle_sums(ang, None) == [8 * 90 * 2 ** 20 + q, 9, 8 * 90 * 2 ** 20 + q, 9, 0, 0]
    ang1 = M.angle_map(n33, n33, 1)
    assert M.angle_sums(ang1, None) == [q, 1, q, 1, 0, 0] and int(np.isnan(ang1).sum()) == 8
    flat = M.normals_expected("flat_5x5")
    assert M.angle_sums(M.angle_map(flat, flat, 1), None) == [0, 9, 0, 9, 0, 0]          # (0, 0, -1) is exact: angle 0
    m = M.angle_mask("33x31_mask")
    s = M.angle_sums(M.angle_map(M.normals_expected("33x31"), M.normals_expected("33x31_other"), 0), m)
    assert s[0] == s[2] + s[4] and s[1] == s[3] + s[5] == 33 * 31 and s[3] == int(m.sum()) and 0 < s[3] < s[1]


def test_header_and_binding_carry_the_three_entries():
    from brdf_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    declared = set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", header))
    for name in ("bn_ssim_map", "bn_grid_normals", "bn_normal_angle"):
        assert name in declared and name in _lib._SIGS, name
        assert hasattr(_lib.lib(), name), name
    assert int(re.search(r"#define BN_SSIM_MAX_WINDOW (\d+)", header).group(1)) == _lib.BN_SSIM_MAX_WINDOW == 11
    assert _lib.BN_ABI_VERSION == 7 and _lib.lib().bn_abi_version() == 7
    assert [len(_lib._SIGS[n][1]) for n in ("bn_ssim_map", "bn_grid_normals", "bn_normal_angle")] == [18, 6, 9]
    import brdf_nerf_amd
    for name in ("image_psnr", "image_ssim", "dsm_normals", "normal_angle_mae", "score_view"):
        assert name in brdf_nerf_amd.__all__ and callable(getattr(brdf_nerf_amd, name))
    from brdf_nerf_amd.build import FILE_FLAGS
    assert "-ffp-contract=off" in FILE_FLAGS["metrics.hip"]
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "brdf_nerf_amd", "csrc", "metrics.hip")).read()


def test_refusals_raise_before_any_library_call(monkeypatch):
    """An even window, one outside 3 to 11, an image too small for the reflect padding, a max_val that is not finite, grids that
    are not on one shape: ValueError by name, from host tensors, with the three bindings replaced by a trap."""
    from brdf_nerf_amd import functions as Fn
    from brdf_nerf_amd import image_ssim, normal_angle_mae, dsm_normals, score_view

    def trap(*a, **k):
        raise AssertionError("the library was called")

    for name in ("ssim_map", "grid_normals", "normal_angle"):
        monkeypatch.setattr(Fn, name, trap)
    img = torch.rand(6 * 8, 3)
    for w in (4, 2, 1, 13, 3.0):
        with pytest.raises(ValueError, match="window"):
            image_ssim(img, img, 6, 8, window=w)
    with pytest.raises(ValueError, match="too small"):
        image_ssim(torch.rand(2 * 9, 3), torch.rand(2 * 9, 3), 2, 9, window=5)
    with pytest.raises(ValueError, match="too small"):
        image_ssim(torch.rand(9 * 5, 3), torch.rand(9 * 5, 3), 9, 5, window=11)
    for bad in (float("nan"), float("inf")):
        t = img.clone()
        t[7, 1] = bad
        with pytest.raises(ValueError, match="max_val"):
            image_ssim(img, t, 6, 8)
    with pytest.raises(ValueError, match="layout"):
        image_ssim(img, img, 6, 8, layout="planar")
    with pytest.raises(ValueError, match="rows"):
        image_ssim(img, img, 6, 8, rows=(3, 7))
    with pytest.raises(ValueError, match="not both"):
        image_ssim(img, torch.rand(6 * 8, 1), 6, 8)
    with pytest.raises(ValueError, match="one grid"):
        normal_angle_mae(torch.zeros(4, 5), torch.zeros(5, 4), 0.5)
    with pytest.raises(ValueError, match="border"):
        normal_angle_mae(torch.zeros(4, 5), torch.zeros(4, 5), 0.5, border="zero")
    with pytest.raises(ValueError, match="mask"):
        normal_angle_mae(torch.zeros(4, 5), torch.zeros(4, 5), 0.5, mask=torch.ones(5, 5))
    with pytest.raises(ValueError, match="resolution"):
        dsm_normals(torch.zeros(4, 5), 0.0)
    with pytest.raises(ValueError, match="rays"):
        score_view(None, None, torch.zeros(10, 11), torch.zeros(10, 3), 3, 4)
    with pytest.raises(ValueError, match="window"):
        score_view(None, None, torch.zeros(12, 11), torch.zeros(12, 3), 3, 4, window=6)


def test_image_psnr_is_the_reference_formula():
    """metrics.py:292-325: without a mask losses.psnr's value; with one the mean over the kept elements of (rgb - gt)^2 /
    max(gt)^2 - the maximum over the WHOLE target - in float64; scl divides both images by max(gt) first."""
    from brdf_nerf_amd import image_psnr
    from brdf_nerf_amd.losses import psnr
    g = torch.Generator().manual_seed(3)
    gt = torch.rand(7 * 9, 3, generator=g) * 0.8
    rgb = (gt + 0.05 * torch.randn(7 * 9, 3, generator=g)).clamp(0, 1)
    p, p_scl = image_psnr(rgb, gt)
    assert torch.equal(p, psnr(rgb, gt)) and p_scl == -1
    mask = torch.rand(7, 9, generator=g) < 0.6
    mask[0, 0] = False
    gt[0, 0] = 0.95                                       # the largest target value lies OUTSIDE the mask and still normalises
    a, b = rgb.double().numpy(), gt.double().numpy()
    keep = np.tile(mask.reshape(-1, 1).numpy(), (1, 3))
    want = -10.0 * np.log10(np.mean(((a - b) ** 2 / b.max() ** 2)[keep]))
    a_s, b_s = a / b.max(), b / b.max()
    want_scl = -10.0 * np.log10(np.mean(((a_s - b_s) ** 2 / b_s.max() ** 2)[keep]))
    p, p_scl = image_psnr(rgb.double(), gt.double(), mask=mask, scl=True)
    assert float(p) == pytest.approx(want, rel=1e-12) and float(p_scl) == pytest.approx(want_scl, rel=1e-12)
    # (the normaliser makes the PSNR scale-free, so upstream's psnr_scl repeats psnr up to rounding)
    assert abs(float(p_scl) - float(p)) < 1e-9 and float(p) != pytest.approx(float(image_psnr(rgb.double(), gt.double())[0]))
    # the same mask flat, per element, and in float32
    assert float(image_psnr(rgb.double(), gt.double(), mask=mask.reshape(-1))[0]) == float(p)
    assert float(image_psnr(rgb.double(), gt.double(), mask=torch.from_numpy(keep))[0]) == float(p)
    assert float(image_psnr(rgb, gt, mask=mask)[0]) == pytest.approx(want, rel=1e-5)
    with pytest.raises(ValueError, match="mask"):
        image_psnr(rgb, gt, mask=torch.ones(5))
