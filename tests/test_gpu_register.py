"""GPU tests of the xy registration (brdf_nerf_amd/register.py; bn_grid_halve, bn_ncc_moments, bn_dsm_shift_diff).  Run on the
MI355X box with `pytest -m gpu`.  Cases and the float64 / Python-integer statements they are held to: tests/register_cases.py;
the reference's own results: tests/golden/dsmr_*.npz."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import register_cases as R
from test_gpu_metrics import EDGE_GRIDS, EDGE_MASKS, edge_mask
from test_gpu_parity import DEV, _free_port
from test_register_cpu import bits32, bits64

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C")).to(DEV)          # a writable copy: the cases are read-only
    return t if dtype is None else t.to(dtype)


@pytest.mark.parametrize("name", R.HALVE_CASES)
def test_grid_halve_bit_equal_to_the_statement(name):
    """float64 + and / only, so every cell equals the statement's bit for bit: NaN and infinite cells, all-missing boxes, odd
    edges, one row, one column."""
    from brdf_nerf_amd import functions as Fn
    a = R.halve_case(name)
    want = R.halve(a)
    got = Fn.grid_halve(dev(a)).cpu().numpy()
    print(f"{name}: {a.shape} -> {got.shape}, NaN cells {int(np.isnan(want).sum())}, cells with other bits {int((bits64(got) != bits64(want)).sum())}")
    assert got.shape == want.shape == ((a.shape[0] + 1) // 2, (a.shape[1] + 1) // 2) and got.dtype == np.float64
    assert np.array_equal(bits64(got), bits64(want))


def run_moments(name, parts=None):
    from brdf_nerf_amd import functions as Fn
    c = R.moment_case(name)
    u, v = dev(c["u"]), dev(c["v"])
    sums = skipped = None
    for rows in (parts or [None]):
        sums, skipped = Fn.ncc_moments(u, v, c["pivot"], c["k"], c["dx0"], c["dy0"], c["r"], sums=sums, skipped=skipped, rows=rows)
    return [tuple(int(x) for x in row) for row in sums.cpu().tolist()], int(skipped.item())


@pytest.mark.parametrize("name", list(R.MOMENT_CASES))
def test_ncc_moments_equal_the_statement(name):
    """All (2r + 1)^2 x 6 integers and the skipped count equal the statement's: nothing is excluded and nothing is approximate."""
    want, want_skipped = R.moments_expected(name)
    got, skipped = run_moments(name)
    wrong = [s for s, (a, b) in enumerate(zip(got, want)) if a != b]
    print(f"{name} ({R.MOMENT_CASES[name][5]}): shifts {len(want)}, with N = 0 {sum(1 for m in want if m[0] == 0)}, largest Suu "
          f"{max(m[3] for m in want)}, skipped {skipped} (statement {want_skipped}), shifts that differ {wrong[:5]}")
    assert got == want
    assert skipped == want_skipped
    assert run_moments(name) == (got, skipped)                     # a second run: the same integers


@pytest.mark.parametrize("name", ["33x31_r5", "64x96_nan_r5", "35x66_r8", "33x40_wrong_pivot"])
def test_ncc_moments_split_invariance(name):
    """Two and three row bands - and bands that cut a tile, single rows, an empty band - added into one `sums` give the
    integers of the single launch."""
    H = R.MOMENT_CASES[name][0]
    whole = run_moments(name)
    assert whole == R.moments_expected(name)
    for what, cuts in {"two bands": [0, H // 2, H], "three bands": [0, 7, H - 1, H], "bands of 5": list(range(0, H, 5)) + [H],
                       "an empty band too": [0, 9, 9, H]}.items():
        assert run_moments(name, parts=list(zip(cuts[:-1], cuts[1:]))) == whole, what
    band = run_moments(name, parts=[(3, 9)])
    assert band == R.moments_expected(name, (3, 9))


@pytest.mark.parametrize("name", list(R.SHIFT_CASES))
def test_dsm_shift_diff_bit_equal_to_the_statement(name):
    """rdsm and diff equal the statement's float32 bit for bit (a float64 addition, a float64 subtraction, two roundings) and
    the six integers are equal, with and without a mask; a shift beyond the grid gives all NaN and count 0."""
    from brdf_nerf_amd import functions as Fn
    c = R.shift_case(name)
    rdsm_w, diff_w, sums_w = R.shift_expected(name)
    mask = None if c["mask"] is None else dev(c["mask"])
    rdsm, diff, sums = Fn.dsm_shift_diff(dev(c["pred"]), dev(c["gt"]), c["dx"], c["dy"], c["b"], mask)
    sums = [int(x) for x in sums.cpu()]
    print(f"{name}: sums {sums} (statement {sums_w}), NaN cells {int(np.isnan(diff_w).sum())} of {diff_w.size}")
    assert np.array_equal(bits32(rdsm.cpu().numpy()), bits32(rdsm_w))
    assert np.array_equal(bits32(diff.cpu().numpy()), bits32(diff_w))
    assert sums == sums_w
    if "beyond" in name:
        assert sums == [0] * 6 and bool(torch.isnan(rdsm).all())
    none, none2, again = Fn.dsm_shift_diff(dev(c["pred"]), dev(c["gt"]), c["dx"], c["dy"], c["b"], mask, want_maps=False)
    assert none is None and none2 is None and [int(x) for x in again.cpu()] == sums_w


@pytest.mark.parametrize("mask_kind", EDGE_MASKS)
@pytest.mark.parametrize("H,W", EDGE_GRIDS)
def test_dsm_shift_diff_at_lane_wave_and_block_edges(H, W, mask_kind):
    """The six block sums where R.SHIFT_CASES never go (one cell; a last wave and a last block that are full, one short or one
    over; a mask that is all zero, all one or every other cell): rdsm, diff and the sums equal the statement's bit for bit."""
    from brdf_nerf_amd import functions as Fn
    pred, gt = R._grid(H, W, 5 + W, nan=0.1).astype(np.float32), R._grid(H, W, 6 + W, nan=0.1).astype(np.float32)
    mask = edge_mask(mask_kind, H, W)
    rdsm_w, diff_w, sums_w = R.shift_diff(pred, gt, 0, 0, 0.5, mask)
    rdsm, diff, sums = Fn.dsm_shift_diff(dev(pred), dev(gt), 0, 0, 0.5, None if mask is None else dev(mask))
    sums = [int(x) for x in sums.cpu()]
    print(f"SHIFT EDGE {H}x{W} mask {mask_kind}: sums {sums} (statement {sums_w}), NaN cells {int(np.isnan(diff_w).sum())} of {diff_w.size}")
    assert np.array_equal(bits32(rdsm.cpu().numpy()), bits32(rdsm_w))
    assert np.array_equal(bits32(diff.cpu().numpy()), bits32(diff_w))
    assert sums == sums_w


@pytest.mark.parametrize("name", R.GOLDENS)
def test_register_xy_finds_the_reference_shift(name):
    """register_xy on the reference's inputs: its (dx, dy) at every level, b within 2^-k + 1e-9 of its b; every integer of every
    level and the pyramid equal the statement's."""
    from brdf_nerf_amd import register_xy
    g = R.golden(name)
    s = R.golden_registration(name)
    got = register_xy(dev(g["v"]), dev(g["u"]))
    print(f"{name}: levels {got['levels']}, k {got['k']} pivot {got['pivot']}, b {got['b']!r} (reference {float(g['b'])!r}, "
          f"|difference| {abs(got['b'] - float(g['b'])):.3e})")
    assert got["levels"] == [tuple(int(x) for x in row) for row in g["levels"]]
    assert (got["dx"], got["dy"]) == tuple(int(x) for x in g["levels"][-1][2:])
    assert abs(got["b"] - float(g["b"])) <= 2.0 ** -got["k"] + 1e-9
    assert (got["k"], got["pivot"], got["skipped"]) == (s["k"], s["pivot"], 0)
    assert [[tuple(row) for row in m.tolist()] for m in got["moments"]] == s["moments"]
    assert got["b"] == s["b"]


def test_altitude_mae_xy_is_its_parts_and_a_known_shift_registers_to_zero():
    from brdf_nerf_amd import altitude_mae_xy, apply_registration, register_xy
    g = R.golden("one_level")
    pred, gt = dev(g["v"]), dev(g["u"])
    mask = torch.from_numpy(np.random.default_rng(3).random(g["u"].shape) < 0.7).to(DEV)
    got = altitude_mae_xy(pred, gt, mask=mask)
    masked = torch.where(mask, pred, torch.full_like(pred, float("nan")))
    reg = register_xy(masked, gt)
    out = apply_registration(masked, gt, reg["dx"], reg["dy"], reg["b"], mask=mask)
    assert (got["dx"], got["dy"], got["shift"]) == (reg["dx"], reg["dy"], reg["b"]) == (8, -4, reg["b"])
    assert (got["mae"], got["mae_in"], got["mae_out"]) == (out["mae"], out["mae_in"], out["mae_out"])
    assert torch.equal(got["rdsm"].view(torch.int32), out["rdsm"].view(torch.int32))
    assert torch.equal(got["diff"].view(torch.int32), out["diff"].view(torch.int32))
    s = [int(x) for x in out["sums"]]
    assert out["mae"] == s[0] / (s[1] * 2.0 ** 20) and out["mae_in"] == s[2] / (s[3] * 2.0 ** 20) and 0 < out["mae"] < 0.2
    assert s[1] == s[3] + s[5] and out["mae"] == pytest.approx(float(torch.nanmean(out["diff"].double().abs())), rel=1e-6)
    plain = altitude_mae_xy(pred, gt)
    assert "mae_in" not in plain and (plain["dx"], plain["dy"]) == (8, -4)
    # a DSM that IS its ground truth moved by (dx, dy) cells and a constant: diff is exactly zero wherever it exists.  Altitudes
    # are multiples of 2^-6 m and the constant of 2^-2, so the quanta, their means and every float32 sum are exact.
    base = np.round(R._grid(70, 90, 9) * 64.0) / 64.0
    dx, dy, c = 3, -2, 2.75
    moved = np.full_like(base, np.nan)
    moved[max(0, dy):70 + min(0, dy), max(0, dx):90 + min(0, dx)] = base[max(0, -dy):70 - max(0, dy), max(0, -dx):90 - max(0, dx)] - c
    z = altitude_mae_xy(dev(moved.astype(np.float32)), dev(base.astype(np.float32)))
    assert (z["dx"], z["dy"], z["shift"]) == (dx, dy, c)
    d = z["diff"]
    assert int(torch.isfinite(d).sum()) == (70 - abs(dy)) * (90 - abs(dx)) and bool((d[torch.isfinite(d)] == 0).all())
    assert z["mae"] == 0.0


@pytest.mark.parametrize("name", ["lambert", "rpv111"])
def test_score_view_register(name):
    """register='z' is bitwise today's dict (the default's); register='xy' is altitude_mae_xy + normal_angle_mae on the
    returned dsm, its other entries unchanged."""
    import dsm_cases as D
    from brdf_nerf_amd import SceneFrame, altitude_mae_xy, normal_angle_mae, score_view
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
    first = score_view(models, args, rays, rgbs, H, W, mask=mask, frame=frame, **kw)
    gt_dsm = (torch.roll(torch.nan_to_num(first["dsm"], nan=12.0), (1, -1), (0, 1)) + 0.5).float()
    gt_dsm[0, 0] = float("nan")
    dsm_mask = (torch.rand(first["dsm"].shape, generator=g) < 0.7).to(DEV)
    kw.update(mask=mask, frame=frame, grid=first["grid"], gt_dsm=gt_dsm, dsm_mask=dsm_mask)
    torch.manual_seed(29)
    today = score_view(models, args, rays, rgbs, H, W, **kw)
    torch.manual_seed(29)
    z = score_view(models, args, rays, rgbs, H, W, register="z", **kw)
    assert set(z) == set(today) and "dx" not in z
    for k, a in today.items():
        b = z[k]
        if torch.is_tensor(a):
            assert a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), k
        else:
            assert (a == b or (a != a and b != b)) and type(a) is type(b), k
    torch.manual_seed(29)
    xy = score_view(models, args, rays, rgbs, H, W, register="xy", **kw)
    assert torch.equal(xy["dsm"].view(torch.int32), today["dsm"].view(torch.int32))
    for k in ("psnr", "psnr_scl", "ssim", "ssim_scl", "skipped"):
        assert xy[k] == today[k], k
    alt = altitude_mae_xy(xy["dsm"], gt_dsm, mask=dsm_mask)
    nr = normal_angle_mae(alt["rdsm"], gt_dsm, first["grid"].resolution, mask=dsm_mask)
    assert (xy["mae"], xy["mae_in"], xy["mae_out"], xy["shift"], xy["dx"], xy["dy"]) == \
        (alt["mae"], alt["mae_in"], alt["mae_out"], alt["shift"], alt["dx"], alt["dy"])
    assert (xy["mae_nr"], xy["mae_nr_in"], xy["mae_nr_out"]) == (nr["mae_nr"], nr["mae_nr_in"], nr["mae_nr_out"])
    assert torch.equal(xy["rdsm"].view(torch.int32), alt["rdsm"].view(torch.int32)) and np.isfinite(xy["mae"])
    with pytest.raises(ValueError, match="register"):
        score_view(models, args, rays, rgbs, H, W, register="bogus", **kw)


def test_refusals():
    """BN_EINVAL with its message, not a launch: null pointers, H or W < 1, more than 2^22 cells, r outside [0, 8], k outside
    [0, 16], rows outside [0, H], a pivot or b that is not finite, |dx| or |dy| above 2^20; and the ValueErrors of the Python
    surface on device tensors."""
    from brdf_nerf_amd import _lib as L
    from brdf_nerf_amd import apply_registration, register_xy
    lib = L.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    u = torch.rand(6, 8, dtype=torch.float64, device=DEV)
    out = torch.zeros(3, 4, dtype=torch.float64, device=DEV)
    sums = torch.zeros(121 * 6, dtype=torch.int64, device=DEV)
    skipped = torch.zeros(1, dtype=torch.int64, device=DEV)
    f = torch.rand(6, 8, device=DEV)
    s6 = torch.zeros(6, dtype=torch.int64, device=DEV)
    nan, inf, far = float("nan"), float("inf"), (1 << 20) + 1

    assert lib.bn_grid_halve(p(u), 6, 8, p(out), None) == 0
    for args in ((None, 6, 8, p(out), None), (p(u), 6, 8, None, None), (p(u), 0, 8, p(out), None), (p(u), 6, 0, p(out), None),
                 (p(u), 2048, 2049, p(out), None)):
        assert lib.bn_grid_halve(*args) == -1 and b"grid_halve" in lib.bn_last_error(), args

    def mom(u_=p(u), v_=p(u), H=6, W=8, pivot=0.0, k=4, dx0=0, dy0=0, r=5, row0=0, row1=6, sm=p(sums), sk=p(skipped)):
        return lib.bn_ncc_moments(u_, v_, H, W, pivot, k, dx0, dy0, r, row0, row1, sm, sk, None)

    assert mom() == 0
    torch.cuda.synchronize()
    before = sums.clone()
    for kw, word in ((dict(u_=None), b"null"), (dict(v_=None), b"null"), (dict(sm=None), b"null"), (dict(sk=None), b"null"),
                     (dict(H=0, row1=0), b"grid"), (dict(W=0), b"grid"), (dict(H=2049, W=2048, row1=1), b"2^22"), (dict(r=-1), b"r="),
                     (dict(r=9), b"r="), (dict(k=-1), b"k="), (dict(k=17), b"k="), (dict(row0=-1), b"rows"), (dict(row1=7), b"rows"),
                     (dict(row0=4, row1=3), b"rows"), (dict(pivot=nan), b"pivot"), (dict(pivot=inf), b"pivot"), (dict(dx0=far), b"2^20"),
                     (dict(dy0=-far), b"2^20")):
        assert mom(**kw) == -1, kw
        assert b"ncc_moments" in lib.bn_last_error() and word in lib.bn_last_error(), (kw, lib.bn_last_error())
    assert mom(dx0=1 << 20, dy0=-(1 << 20), row0=2, row1=2) == 0            # the bound itself, and an empty band

    def shd(pr=p(f), g_=p(f), H=6, W=8, dx=0, dy=0, b=0.0, sm=p(s6)):
        return lib.bn_dsm_shift_diff(pr, g_, H, W, dx, dy, b, None, None, None, sm, None)

    assert shd() == 0
    for kw, word in ((dict(pr=None), b"null"), (dict(g_=None), b"null"), (dict(sm=None), b"null"), (dict(H=0), b"grid"), (dict(W=-1), b"grid"),
                     (dict(H=2048, W=2049), b"2^22"), (dict(b=nan), b"b="), (dict(b=-inf), b"b="), (dict(dx=far), b"2^20"), (dict(dy=-far), b"2^20")):
        assert shd(**kw) == -1, kw
        assert b"dsm_shift_diff" in lib.bn_last_error() and word in lib.bn_last_error(), (kw, lib.bn_last_error())
    torch.cuda.synchronize()
    assert torch.equal(sums, before) and int(s6[1]) == 48 and int(s6[0]) == 0

    z = torch.zeros(4, 5, device=DEV)
    with pytest.raises(ValueError, match="2\\^20"):
        register_xy(torch.tensor([[0.0, 2.0 ** 20 + 1.0]], device=DEV), torch.zeros(1, 2, device=DEV))
    with pytest.raises(ValueError, match="finite cell"):
        register_xy(z * nan, z * nan)
    with pytest.raises(ValueError, match="rows"):
        register_xy(z, z, rows=(2, 5))
    with pytest.raises(ValueError, match="irange"):
        register_xy(z, z, irange=9)
    with pytest.raises(ValueError, match="not finite"):
        apply_registration(z, z, 0, 0, nan)
    with pytest.raises(ValueError, match="2\\^20"):
        apply_registration(z, z, far, 0, 0.0)
    with pytest.raises(ValueError, match="mask"):
        apply_registration(z, z, 0, 0, 0.0, mask=torch.ones(5, 5))
    flat = register_xy(z, z)                                                # constant grids: no shift can win, the start is returned
    assert (flat["dx"], flat["dy"], flat["b"]) == (0, 0, 0.0)


def test_two_rank_registration_matches_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_register_worker.py), each child under its own time limit and started
    once: the row bands merged by one SUM all-reduce per level give the moments, (dx, dy) and b of the single process, bitwise."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_register_worker.py")
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
