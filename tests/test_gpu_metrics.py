"""GPU tests of the image and normal metrics (brdf_nerf_amd/metrics.py; bn_ssim_map, bn_grid_normals, bn_normal_angle).  Run on
the MI355X box with `pytest -m gpu`.  Cases and the float64 statements they are held to: tests/metric_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metric_cases as M
from test_gpu_parity import DEV, _free_port

pytestmark = pytest.mark.gpu

# bn_normal_angle against the statement on the float32 normals the kernel was given (arccos is not bit-specified).  Measured on
# an MI355X over every case of M.ANGLE_CASES: the float32 angle map differed from (float) of the statement's in 0 of 4325
# cells (largest error 0.0 degrees) and every integer sum was the statement's (error 0 units of 2^-20 degree per cell): a
# last-place difference of the device's float64 arccos does not reach a float32 rounding or an llrint boundary on these cases.
# The gates are 4 x the largest measured error, the project's convention (tests/test_gpu_ray_kernels_f64.py): 4 x 0 = 0.
ANGLE_MEASURED = {"map_abs_deg": 0.0, "sum_units_per_cell": 0.0}
ANGLE_GATE = {k: 4.0 * v for k, v in ANGLE_MEASURED.items()}


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C")).to(DEV)          # a writable copy: the cases are read-only
    return t if dtype is None else t.to(dtype)


def bits(a):
    """float32 compared bitwise, NaN cells included: a NaN compares as NaN (one canonical pattern).  IEEE 754 leaves the sign and
    payload of a propagated NaN open - a - b with a NaN b keeps b's sign on the host and flips it on the device, whose subtraction
    is an addition with a negated operand - so which NaN a cell holds is no property of the rule; THAT it is NaN is."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.int32(0x7FC00000), a.view(np.int32))


def run_ssim(name, parts=None, want_map=True):
    """A case through bn_ssim_map with the statement's own weights, whole or as the row ranges `parts` accumulated into one
    triple and one map.  -> (map (C, H, W) float32 numpy, prefilled with a sentinel, sums as 3 Python ints)."""
    from brdf_nerf_amd import functions as Fn
    c = M.ssim_case(name)
    pred, gt = dev(c["pred"]), dev(c["gt"])
    mask = None if c["mask"] is None else dev(c["mask"])
    sums = torch.zeros(3, dtype=torch.int64, device=DEV)
    out = torch.full((c["C"], c["H"], c["W"]), -7.0, dtype=torch.float32, device=DEV) if want_map else None
    for rows in (parts or [None]):
        Fn.ssim_map(pred, gt, c["C"], c["H"], c["W"], c["strides"], mask, c["div"], c["max_val"], c["window"], c["g"].tolist(), sums,
                    rows=rows, out=out)
    return (out.cpu().numpy() if want_map else None), tuple(int(v) for v in sums.cpu())


@pytest.mark.parametrize("name", list(M.SSIM_CASES))
def test_ssim_bit_equal_to_the_float64_statement(name):
    """The three integers equal the statement exactly and the float32 map equals (float) of the statement's float64 map bit for
    bit in every cell, NaN pattern included: the rule is a float64 chain rounded operation by operation.  A difference means a
    contracted multiply-add, a wrong reflect index or a wrong tap order.  Nothing is excluded."""
    want = M.ssim_expected(name)
    got, sums = run_ssim(name)
    print(f"{name}: sums {sums} (statement {want['sums']}); map cells with other bits "
          f"{int((bits(got) != bits(want['map'])).sum())} of {got.size}")
    assert sums == want["sums"]
    assert got.dtype == np.float32 and got.shape == want["map"].shape
    assert np.array_equal(np.isnan(got), np.isnan(want["map"]))
    assert np.array_equal(bits(got), bits(want["map"]))
    # without a map the integers are the same
    assert run_ssim(name, want_map=False)[1] == want["sums"]


@pytest.mark.parametrize("name", ["33x31_w11", "64x96_mask_image_scl", "nan_pixel_16x18_w5"])
def test_ssim_split_invariance_is_bitwise(name):
    """Any partition of the output rows into ranges gives the same integers and the same map as one launch: single rows, one row
    against the rest (both ends), even halves, bands that cut a tile; a range leaves the rows outside it untouched."""
    H = M.ssim_case(name)["H"]
    whole_map, whole = run_ssim(name)
    assert whole == M.ssim_expected(name)["sums"]
    cuts = {"single rows": list(range(H + 1)), "first row | rest": [0, 1, H], "rest | last row": [0, H - 1, H],
            "halves": [0, H // 2, H], "bands of 5": list(range(0, H, 5)) + [H], "an empty range too": [0, 7, 7, H]}
    for what, c in cuts.items():
        got_map, got = run_ssim(name, parts=list(zip(c[:-1], c[1:])))
        assert got == whole, what
        assert np.array_equal(bits(got_map), bits(whole_map)), what
    band_map, band = run_ssim(name, parts=[(3, 9)])
    assert band == M.ssim_sums(M.ssim_expected(name)["v"], (3, 9))
    assert np.all(band_map[:, :3] == -7.0) and np.all(band_map[:, 9:] == -7.0)
    assert np.array_equal(bits(band_map[:, 3:9]), bits(whole_map[:, 3:9]))


def test_ssim_refusals():
    """BN_EINVAL, not a launch: an even window, one outside 3 to 11, an image too small for the reflect padding, a max_val or div
    that is not finite, rows outside the image, C H W over 2^30, NULL pointers."""
    import ctypes as C
    from brdf_nerf_amd import _lib as L
    lib = L.lib()
    img = torch.rand(3 * 6 * 8, device=DEV)
    sums = torch.zeros(3, dtype=torch.int64, device=DEV)
    g = (C.c_double * 11)(*([1.0 / 11] * 11))
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(C_=3, H=6, W=8, window=3, div=1.0, max_val=1.0, row0=0, row1=6, pred=p(img), gw=g, sm=p(sums), sp=48):
        return lib.bn_ssim_map(pred, p(img), C_, H, W, sp, W, 1, None, div, max_val, window, gw, row0, row1, None, sm, None)

    assert call() == 0
    torch.cuda.synchronize()
    before = sums.clone()
    for kw in (dict(window=4), dict(window=1), dict(window=13), dict(window=0), dict(H=2, W=9, window=5, row1=2), dict(H=9, W=5, window=11),
               dict(max_val=float("nan")), dict(max_val=float("inf")), dict(div=float("nan")), dict(row0=-1), dict(row1=7),
               dict(row0=4, row1=3), dict(C_=1 << 10, H=1 << 10, W=(1 << 10) + 1, row1=1), dict(pred=None), dict(gw=None), dict(sm=None),
               dict(sp=-1), dict(H=0, row1=0)):
        assert call(**kw) == -1, kw
        assert b"ssim_map" in lib.bn_last_error(), kw
    assert b"reflect" in (call(H=2, W=9, window=5, row1=2), lib.bn_last_error())[1]
    z = torch.zeros(4, 5, device=DEV)
    n = torch.zeros(4, 5, 3, device=DEV)
    s6 = torch.zeros(6, dtype=torch.int64, device=DEV)
    assert lib.bn_grid_normals(p(z), 4, 5, 0.5, p(n), None) == 0
    for args in ((None, 4, 5, 0.5, p(n), None), (p(z), 4, 5, 0.0, p(n), None), (p(z), 0, 5, 0.5, p(n), None), (p(z), 4, 5, 0.5, None, None)):
        assert lib.bn_grid_normals(*args) == -1 and b"grid_normals" in lib.bn_last_error()
    assert lib.bn_normal_angle(p(n), p(n), 4, 5, None, 0, None, p(s6), None) == 0
    for args in ((None, p(n), 4, 5, None, 0, None, p(s6), None), (p(n), p(n), 4, 5, None, 2, None, p(s6), None),
                 (p(n), p(n), 4, 5, None, 0, None, None, None)):
        assert lib.bn_normal_angle(*args) == -1 and b"normal_angle" in lib.bn_last_error()
    torch.cuda.synchronize()
    assert torch.equal(sums, before)


@pytest.mark.parametrize("layout", ["reference", "image"])
def test_image_ssim_is_the_statement_of_its_layout(layout):
    """image_ssim on the masked 64 x 96 view, both layouts, with scl: max_val = max(target * mask) under that layout, the second
    launch divides by it with max_val = 1; every number is sum / (count 2^30) of the statement's integers, exactly."""
    from brdf_nerf_amd import image_ssim
    plain, scl = M.ssim_case(f"64x96_mask_{layout}"), M.ssim_case(f"64x96_mask_{layout}_scl")
    C, H, W = plain["C"], plain["H"], plain["W"]
    rgb, gt = dev(plain["pred"]).reshape(H * W, C), dev(plain["gt"]).reshape(H * W, C)
    ssim, ssim_scl, info = image_ssim(rgb, gt, H, W, mask=dev(plain["mask"]).bool(), window=scl["window"], layout=layout, scl=True,
                                      want_map=True)
    want_scl = M.ssim_expected(f"64x96_mask_{layout}_scl")
    assert info["max_val"] == plain["top"] == scl["div"]
    assert tuple(int(v) for v in info["sums"][1]) == want_scl["sums"]
    assert ssim_scl == want_scl["sums"][0] / (want_scl["sums"][1] * 2.0 ** 30) and 0.9 < ssim_scl < 1.0
    assert np.array_equal(bits(info["map_scl"].cpu().numpy()), bits(want_scl["map"]))
    ssim3, none, info3 = image_ssim(rgb, gt, H, W, mask=dev(plain["mask"]).reshape(-1), layout=layout)
    want = M.ssim_expected(f"64x96_mask_{layout}")
    assert none == -1 and info3["map"] is None and info3["skipped"] == 0
    assert tuple(int(v) for v in info3["sums"][0]) == want["sums"] and ssim3 == want["sums"][0] / (want["sums"][1] * 2.0 ** 30)
    # row bands of two calls add up to the whole
    a = image_ssim(rgb, gt, H, W, mask=dev(plain["mask"]), layout=layout, rows=(0, 29))[2]["sums"]
    b = image_ssim(rgb, gt, H, W, mask=dev(plain["mask"]), layout=layout, rows=(29, H))[2]["sums"]
    assert torch.equal(a + b, info3["sums"])


@pytest.mark.parametrize("name", list(M.NORMAL_CASES))
def test_grid_normals_bit_equal_to_the_float64_statement(name):
    """The chain is float64 + - * / sqrt, all correctly rounded, so the float32 normals equal the statement's bit for bit, NaN
    cells and the zero border included."""
    from brdf_nerf_amd import dsm_normals
    res, z = M.normal_case(name)
    want = M.normals_expected(name)
    got = dsm_normals(dev(z), res).cpu().numpy()
    other = bits(got) != bits(want)
    with np.errstate(invalid="ignore"):
        far = float(np.nanmax(np.abs(got.astype(np.float64) - want.astype(np.float64)))) if other.any() else 0.0
    print(f"{name}: components with other bits {int(other.sum())} of {got.size}, max abs difference {far:.3e}")
    assert got.shape == z.shape + (3,) and got.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(bits(got), bits(want))


def test_plane_normals_on_the_device():
    from brdf_nerf_amd import dsm_normals
    a, b, res = M.PLANE
    got = dsm_normals(dev(M.normal_case("plane_6x7")[1]), res).cpu().numpy()
    assert np.abs(got[1:-1, 1:-1] - M.plane_normal(a, b)).max() < 1e-7
    assert np.all(dsm_normals(dev(M.normal_case("flat_5x5")[1]), 0.5)[1:-1, 1:-1].cpu().numpy() == np.float32([0, 0, -1]))


def run_angle(name):
    """-> (angle (H, W) float32 numpy, sums (6 ints), the statement's float64 angle map, its sums) on the kernel's own normals."""
    from brdf_nerf_amd import dsm_normals
    from brdf_nerf_amd import functions as Fn
    first, second, _, border = M.ANGLE_CASES[name]
    n1 = dsm_normals(dev(M.normal_case(first)[1]), M.normal_case(first)[0])
    n2 = dsm_normals(dev(M.normal_case(second)[1]), M.normal_case(second)[0])
    mask = M.angle_mask(name)
    angle, sums = Fn.normal_angle(n1, n2, None if mask is None else dev(mask), border)
    want = M.angle_map(n1.cpu().numpy(), n2.cpu().numpy(), border)
    return angle.cpu().numpy(), [int(v) for v in sums.cpu()], want, M.angle_sums(want, mask)


@pytest.mark.parametrize("name", list(M.ANGLE_CASES))
def test_normal_angle_against_the_statement(name):
    """Per cell against the statement on the float32 normals the kernel was given.  The counts and the NaN pattern are exact; the
    float32 angle and the integer sums are gated at 4 x the largest error measured over all cases (ANGLE_MEASURED)."""
    got, sums, want, want_sums = run_angle(name)
    with np.errstate(invalid="ignore"):
        want32 = want.astype(np.float32)
        err = float(np.nanmax(np.abs(got.astype(np.float64) - want32.astype(np.float64)))) if not np.isnan(want).all() else 0.0
    per_cell = [abs(sums[k] - want_sums[k]) / max(want_sums[k + 1], 1) for k in (0, 2, 4)]
    print(f"ANGLE {name}: map max abs error {err:.3e} deg, cells with other bits {int((bits(got) != bits(want32)).sum())} of {got.size}; "
          f"sums {sums} statement {want_sums}; sum error per cell (units of 2^-20 deg) {max(per_cell):.3e}")
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert [sums[1], sums[3], sums[5]] == [want_sums[1], want_sums[3], want_sums[5]]
    assert err <= ANGLE_GATE["map_abs_deg"]
    assert max(per_cell) <= ANGLE_GATE["sum_units_per_cell"]
    if "equal" in name:
        inner = got[1:-1, 1:-1]
        assert np.all(inner < 0.03) and (M.ANGLE_CASES[name][3] == 1 or np.all(got[0] == 90.0))
    # two runs give bit-equal sums and maps
    again, sums2, _, _ = run_angle(name)
    assert sums2 == sums and np.array_equal(bits(again), bits(got))


EDGE_GRIDS = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 255), (16, 16), (1, 257), (3, 171)]      # one cell; a wave, a block +- one cell
EDGE_MASKS = ("none", "zero", "one", "odd")


def edge_mask(kind, H, W):
    """(H, W) uint8 numpy or None: no mask, all zero, all one, or the cells of odd index."""
    odd = (np.arange(H * W).reshape(H, W) & 1).astype(np.uint8)
    return {"none": None, "zero": odd * 0, "one": odd * 0 + 1, "odd": odd}[kind]


@pytest.mark.parametrize("mask_kind", EDGE_MASKS)
@pytest.mark.parametrize("H,W,border", [g + (0,) for g in EDGE_GRIDS] + [(3, 171, 1)])
def test_normal_angle_sums_at_lane_wave_and_block_edges(H, W, border, mask_kind):
    """The six block sums where the other cases never go: one cell, a last wave and a last block that are full, one short or one
    over.  n1 cycles through (0,0,1), (1,0,0), (0,0,-1), (0,1,0) by cell index against n2 = (0,0,1): every angle is 0, 90 or 180
    degrees, arccos is exact there, so the sums equal the statement's AND the closed form (90 n90 + 180 n180) 2^20 exactly."""
    from brdf_nerf_amd import functions as Fn
    cell = np.arange(H * W).reshape(H, W)
    n1 = np.float32([(0, 0, 1), (1, 0, 0), (0, 0, -1), (0, 1, 0)])[cell % 4]
    n2 = np.broadcast_to(np.float32([0, 0, 1]), (H, W, 3))
    mask = edge_mask(mask_kind, H, W)
    _, sums = Fn.normal_angle(dev(n1), dev(n2), None if mask is None else dev(mask), border, want_map=False)
    sums = [int(v) for v in sums.cpu()]
    want = M.angle_map(n1, n2, border)
    counted = ~np.isnan(want)
    inside = np.ones((H, W), bool) if mask is None else mask != 0
    closed = []
    for sel in (counted, counted & inside, counted & ~inside):
        n90, n180 = int((sel & (cell % 2 == 1)).sum()), int((sel & (cell % 4 == 2)).sum())
        closed += [(90 * n90 + 180 * n180) << 20, int(sel.sum())]
    print(f"ANGLE EDGE {H}x{W} border {border} mask {mask_kind}: sums {sums} statement {M.angle_sums(want, mask)} closed form {closed}")
    assert sums == M.angle_sums(want, mask)
    assert sums == closed
    if border:
        assert sums[1] == 169


def test_normal_angle_mae_is_its_sums():
    from brdf_nerf_amd import normal_angle_mae
    (res, z1), (_, z2) = M.normal_case("33x31"), M.normal_case("33x31_other")
    mask = M.angle_mask("33x31_mask")
    got = normal_angle_mae(dev(z1), dev(z2), res, mask=dev(mask))
    _, sums, _, _ = run_angle("33x31_mask")
    assert [int(v) for v in got["sums"]] == sums and got["diff_nr"].shape == (33, 31)
    assert got["mae_nr"] == sums[0] / (sums[1] * 2.0 ** 20) and got["mae_nr_in"] == sums[2] / (sums[3] * 2.0 ** 20)
    assert got["mae_nr_out"] == sums[4] / (sums[5] * 2.0 ** 20) and 0.0 < got["mae_nr"] < 180.0
    # the float32 angle map's nanmean is the same number to float32 accuracy
    assert got["mae_nr"] == pytest.approx(float(torch.nanmean(got["diff_nr"].double())), rel=1e-6)
    plain = normal_angle_mae(dev(z1), z2, res, border="nan")                    # a host ground truth; the border left out
    _, sums_b, _, _ = run_angle("33x31_mask_b1")
    assert plain["mae_nr_in"] == -1 and plain["mae_nr_out"] == -1 and int(plain["sums"][1]) == 31 * 29 == sums_b[1]
    assert int(torch.isnan(plain["diff_nr"]).sum()) == 33 * 31 - 31 * 29


@pytest.mark.parametrize("name", ["lambert", "rpv111"])
def test_score_view_against_its_parts(name):
    """score_view's depth and dsm are bitwise dsm_image's after the same torch.manual_seed (and its rgb render_image's), and
    its numbers are image_psnr, image_ssim, altitude_mae and normal_angle_mae on those outputs."""
    import dsm_cases as D
    from brdf_nerf_amd import SceneFrame, altitude_mae, dsm_image, image_psnr, image_ssim, normal_angle_mae, score_view
    from brdf_nerf_amd.evaluate import render_image
    from test_gpu_relight import R_TEST, build, flags
    cfg, args, models, rays = build(name)
    fl, cosi = flags(name)
    H, W = 15, 20
    assert R_TEST == H * W
    frame = SceneFrame(D.CENTER, D.RANGE)
    kw = dict(chunk=128, cos_irra_on=cosi, **fl)
    g = torch.Generator().manual_seed(5)
    rgbs = torch.rand(H * W, 3, generator=g).to(DEV)
    mask = (torch.rand(H, W, generator=g) < 0.8).to(DEV)
    torch.manual_seed(29)
    ref = dsm_image(models, args, rays, frame, **kw)
    torch.manual_seed(29)
    img = render_image(models, args, rays, **kw)
    grid = ref["grid"]
    gt_dsm = (ref["dsm"] + 0.5 + 0.2 * torch.randn(ref["dsm"].shape, generator=g).to(DEV)).float()
    gt_dsm[0, 0] = float("nan")
    dsm_mask = (torch.rand(ref["dsm"].shape, generator=g) < 0.5).to(DEV)
    torch.manual_seed(29)
    got = score_view(models, args, rays, rgbs, H, W, mask=mask, frame=frame, gt_dsm=gt_dsm, dsm_mask=dsm_mask, **kw)
    assert torch.equal(got["depth"], ref["depth"]) and torch.equal(got["rgb"], img["rgb"]) and got["grid"] == grid
    assert torch.equal(got["dsm"].view(torch.int32), ref["dsm"].view(torch.int32)) and torch.equal(got["count"], ref["count"])
    assert got["skipped"] == ref["skipped"]
    p, p_scl = image_psnr(got["rgb"], rgbs, mask=mask, scl=True)
    s, s_scl, info = image_ssim(got["rgb"], rgbs, H, W, mask=mask, scl=True)
    alt = altitude_mae(got["dsm"], gt_dsm, mask=dsm_mask)
    nr = normal_angle_mae(got["dsm"], gt_dsm, grid.resolution, mask=dsm_mask)
    assert (got["psnr"], got["psnr_scl"]) == (float(p), float(p_scl))
    assert (got["ssim"], got["ssim_scl"], got["ssim_skipped"]) == (s, s_scl, info["skipped"]) and torch.equal(got["ssim_sums"], info["sums"])
    assert (got["mae"], got["mae_in"], got["mae_out"]) == (alt["mae"], alt["mae_in"], alt["mae_out"])
    assert (got["mae_nr"], got["mae_nr_in"], got["mae_nr_out"]) == (nr["mae_nr"], nr["mae_nr_in"], nr["mae_nr_out"])
    for k in ("psnr", "psnr_scl", "ssim", "ssim_scl", "mae", "mae_in", "mae_out"):
        assert np.isfinite(got[k]), k
    # without a frame: the image numbers alone, the same ones; with the grid passed in: the same DSM
    torch.manual_seed(29)
    plain = score_view(models, args, rays, rgbs, H, W, mask=mask, **kw)
    assert "dsm" not in plain and "mae" not in plain and (plain["psnr"], plain["ssim"], plain["ssim_scl"]) == (got["psnr"], got["ssim"], got["ssim_scl"])
    assert torch.equal(plain["depth"], ref["depth"])
    torch.manual_seed(29)
    again = score_view(models, args, rays, rgbs, H, W, mask=mask, frame=frame, grid=grid, **kw)
    assert torch.equal(again["dsm"].view(torch.int32), ref["dsm"].view(torch.int32)) and "mae" not in again


def test_two_rank_scores_match_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_metrics_worker.py), each child under its own time limit and started
    once: the row bands merged by one SUM all-reduce give the integer triples of the single process, and the same numbers."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_metrics_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=_free_port(), WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, worker], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=300)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append("TIMEOUT\n" + p.communicate()[0])
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert all("RESULT" in o and "ok" in o for o in outs), "\n".join(outs)
