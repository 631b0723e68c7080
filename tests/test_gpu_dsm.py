"""GPU tests of the DSM rasteriser (brdf_nerf_amd/dsm.py, bn_dsm_splat / bn_dsm_resolve).  Run on the MI355X box with
`pytest -m gpu`.  Cases and the float64 statement they are held to: tests/dsm_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dsm_cases as D
from test_gpu_parity import DEV, _free_port

pytestmark = pytest.mark.gpu


def frame():
    from brdf_nerf_amd import SceneFrame
    return SceneFrame(D.CENTER, D.RANGE)


def accumulate(name, order=None, chunk=None):
    """A case's rows (in `order`, `chunk` rows per add) in a fresh accumulator."""
    from brdf_nerf_amd import DsmAccumulator, Grid
    grid, radius, footprint, rays, depth = D.case(name)
    rays, depth = torch.from_numpy(rays.copy()).to(DEV), torch.from_numpy(depth.copy()).to(DEV)
    if order is not None:
        rays, depth = rays[order].contiguous(), depth[order].contiguous()
    acc = DsmAccumulator(Grid(*grid), DEV, radius=radius, footprint=footprint)
    R = rays.shape[0]
    for i in range(0, R, chunk or R):
        acc.add(rays[i:i + (chunk or R)], depth[i:i + (chunk or R)], frame())
    return acc


def bits(t):
    return t.contiguous().view(torch.int32)         # float32 compared bitwise: NaN cells included


@pytest.mark.parametrize("name", list(D.CASES))
def test_bit_equal_to_the_float64_statement(name):
    """acc (sums and counts), skipped, dsm (its NaN pattern included) and count equal the numpy statement exactly, in every cell:
    the rule is integer after a float64 chain rounded operation by operation.  A difference means a contracted multiply-add or a
    wrong index rule."""
    want = D.expected(name)
    acc = accumulate(name)
    got = acc.acc.cpu().numpy()
    dsm, count = acc.result()
    dsm, count = dsm.cpu().numpy(), count.cpu().numpy()
    print(f"{name}: cells with another sum {int((got[..., 0] != want['sums']).sum())}, another count "
          f"{int((got[..., 1] != want['counts']).sum())} of {want['sums'].size}; skipped {acc.skipped} (statement {want['skipped']}); "
          f"dsm cells with other bits {int((dsm.view(np.int32) != want['dsm'].view(np.int32)).sum())}")
    assert got.shape == want["sums"].shape + (2,) and got.dtype == np.int64
    assert np.array_equal(got[..., 0], want["sums"])
    assert np.array_equal(got[..., 1], want["counts"])
    assert acc.skipped == want["skipped"]
    assert dsm.dtype == np.float32 and np.array_equal(np.isnan(dsm), np.isnan(want["dsm"]))
    assert np.array_equal(dsm.view(np.int32), want["dsm"].view(np.int32))
    assert count.dtype == np.int32 and np.array_equal(count, want["count"])


def test_split_invariance_is_bitwise():
    """The same points in one add, shuffled, and in chunks of 1, 64 and 100: one accumulator, bit for bit."""
    name = "large_R300_r2_disc"
    whole = accumulate(name)
    R = D.case(name)[3].shape[0]
    perm = torch.from_numpy(np.random.RandomState(9).permutation(R)).to(DEV)
    runs = {"shuffled": accumulate(name, order=perm), "chunks of 1": accumulate(name, chunk=1), "chunks of 64": accumulate(name, chunk=64),
            "chunks of 100": accumulate(name, chunk=100), "shuffled, chunks of 64": accumulate(name, order=perm, chunk=64)}
    assert int(whole.acc[..., 1].sum()) > 0
    for what, a in runs.items():
        assert torch.equal(a.acc, whole.acc) and a.skipped == whole.skipped, what
    # two views in one accumulator: the sums of the two on their own
    both = accumulate(name)
    _, _, _, rays, depth = D.case("large_R300_r1_disc")
    both.add(torch.from_numpy(rays.copy()).to(DEV), torch.from_numpy(depth.copy()).to(DEV), frame())
    two = D.splat(rays, depth, *D.case(name)[:3], acc=D.splat(*D.case(name)[3:], *D.case(name)[:3]))
    assert np.array_equal(both.acc[..., 0].cpu().numpy(), D.as_int64(two[0])) and np.array_equal(both.acc[..., 1].cpu().numpy(), D.as_int64(two[1]))
    assert both.skipped == two[2]


def test_fp32_positions_would_be_caught():
    """The guard on the yardstick: the statement evaluated with positions rounded to fp32 differs from the product's result (and
    from the float64 statement) on the guarded case, so the bit-equality test above would catch a float32 implementation."""
    name = D.FP32_GUARD_CASE
    acc = accumulate(name).acc.cpu().numpy()
    f64, f32 = D.expected(name), D.expected(name, True)
    assert np.array_equal(acc[..., 1], f64["counts"])
    n = int((acc[..., 1] != f32["counts"]).sum())
    print(f"{name}: {n} of {f32['counts'].size} cells change their count with fp32 positions")
    assert n >= 1


def test_refusals():
    """BN_EINVAL, not a launch: radius outside [0, 4], resolution <= 0, another footprint, a grid over 2^31 cells, NULL pointers."""
    import ctypes as C
    from brdf_nerf_amd import _lib as L
    lib = L.lib()
    rays, depth = torch.zeros(4, 8, device=DEV), torch.ones(4, device=DEV)
    rays[:, 0] = -1000.0                            # 6 km west of every grid below: no call deposits anything, accepted or not
    acc, skipped = torch.zeros(5, 7, 2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    c = (C.c_double * 3)(*D.CENTER)
    p = lambda t: C.c_void_p(t.data_ptr())

    def splat(radius=1, res=0.5, W=7, H=5, fp=0, rays_p=p(rays), acc_p=p(acc), sk=p(skipped)):
        return lib.bn_dsm_splat(rays_p, 8, p(depth), 4, c, 6.0, D.SMALL[0], D.SMALL[1], res, W, H, radius, fp, acc_p, sk, None)

    assert splat() == 0
    for kw in (dict(radius=-1), dict(radius=5), dict(res=0.0), dict(res=-0.5), dict(fp=2), dict(W=1 << 16, H=(1 << 15) + 1),
               dict(rays_p=None), dict(acc_p=None), dict(sk=None), dict(W=0)):
        assert splat(**kw) == -1, kw
        assert b"dsm_splat" in lib.bn_last_error()
    dsm = torch.empty(5, 7, device=DEV)
    assert lib.bn_dsm_resolve(p(acc), 7, 5, p(dsm), None, None) == 0
    assert lib.bn_dsm_resolve(None, 7, 5, p(dsm), None, None) == -1 and lib.bn_dsm_resolve(p(acc), 7, 5, None, None, None) == -1
    torch.cuda.synchronize()
    assert int(acc.abs().sum()) == 0 and int(skipped) == 0


@pytest.mark.parametrize("name", ["lambert", "rpv111"])
def test_dsm_image_against_the_product_path(name):
    """After the same torch.manual_seed dsm_image's depth is render_image's, bit for bit, and its dsm is what a DsmAccumulator fed
    that depth gives - with a chunk smaller than R that does not divide it, with the grid taken from the cloud and with the same
    grid passed in (splatted chunk by chunk)."""
    from brdf_nerf_amd import DsmAccumulator, altitude_image, dsm_image
    from brdf_nerf_amd.evaluate import render_image
    from test_gpu_relight import R_TEST, build, flags
    cfg, args, models, rays = build(name)
    fl, cosi = flags(name)
    assert R_TEST == 300
    kw = dict(chunk=128, cos_irra_on=cosi, **fl)
    torch.manual_seed(29)
    ref = render_image(models, args, rays, **kw)
    torch.manual_seed(29)
    got = dsm_image(models, args, rays, frame(), **kw)
    assert torch.equal(got["depth"], ref["depth"])
    grid = got["grid"]
    assert 1 < grid.width < 200 and 1 < grid.height < 200 and grid.resolution == 0.5
    acc = DsmAccumulator(grid, DEV).add(rays, ref["depth"], frame())
    dsm, count = acc.result()
    assert int((count > 0).sum()) > 0 and got["skipped"] == acc.skipped
    assert torch.equal(bits(got["dsm"]), bits(dsm)) and torch.equal(got["count"], count)
    assert torch.equal(got["altitude"], altitude_image(rays, ref["depth"], frame())) and got["altitude"].dtype == torch.float64
    torch.manual_seed(29)
    again = dsm_image(models, args, rays, frame(), grid=grid, **kw)
    assert torch.equal(again["depth"], ref["depth"]) and torch.equal(bits(again["dsm"]), bits(dsm)) and torch.equal(again["count"], count)
    assert again["grid"] is grid


def test_two_rank_dsm_matches_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_dsm_worker.py), each child under its own time limit and started once:
    every rank's dsm_image(group=...) result equals the single-process one bitwise."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_dsm_worker.py")
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


def _block_edge_rows():
    """257 rows on SMALL (radius 1, disc): rows 0, 63, 64, 255 and 256 - the first and last lane of a wave, the first lane of the
    next, the last lane of a block and a block of one lane - must be skipped; every other row lands on the grid."""
    k = np.arange(257)
    rays, depth = D._nadir(-2.8125 + 0.1875 * (k % 17), -1.3125 + 0.1875 * (k % 13), -3.0 + 0.75 * (k % 7), 0.5)
    depth[0] = np.nan                                            # NaN depth
    rays[63, 0] = np.inf                                         # inf origin
    rays[64, 2], rays[64, 5], depth[64] = 0.25, 1.0, 1398099.0   # altitude == 2^23 exactly (dsm_cases._bad_rows)
    rays[255, 5], depth[255] = -1.0, 2.0e6                       # altitude about -1.2e7 m
    rays[256, 1], depth[256] = -np.inf, np.nan                   # both
    return rays, depth


def test_block_edges_of_the_shared_kernel():
    """bn_dsm_splat runs the kernel of bn_dsm_splat_world, which counts its skipped rows per block (no lane leaves early): bad rows
    at a wave edge, a block edge and alone in a last block of one lane, then a bad row on its own (R = 1) and a whole block
    (R = 256).  acc and skipped are the statement's integers exactly."""
    from brdf_nerf_amd import _lib as L
    from brdf_nerf_amd import functions as Fn
    rays, depth = _block_edge_rows()
    xoff, yoff, res, W, H = D.SMALL
    for R, bad in ((257, 5), (1, 1), (256, 4)):
        sums, counts, skipped = D.splat(rays[:R], depth[:R], D.SMALL, 1, "disc")
        assert skipped == bad and int(D.splat(rays[:R], depth[:R], D.SMALL, 0, "disc")[1].sum()) == R - bad      # all others land
        acc, sk = torch.zeros((H, W, 2), dtype=torch.int64, device=DEV), torch.zeros((1,), dtype=torch.int64, device=DEV)
        Fn.dsm_splat(torch.from_numpy(rays[:R].copy()).to(DEV), torch.from_numpy(depth[:R].copy()).to(DEV), D.CENTER, D.RANGE, xoff, yoff,
                     res, 1, L.BN_DSM_DISC, acc, sk)
        got = acc.cpu().numpy()
        print(f"R = {R}: cells with another sum {int((got[..., 0] != D.as_int64(sums)).sum())}, another count "
              f"{int((got[..., 1] != D.as_int64(counts)).sum())}; skipped {int(sk)} (statement {skipped})")
        assert np.array_equal(got[..., 0], D.as_int64(sums)) and np.array_equal(got[..., 1], D.as_int64(counts)), R
        assert int(sk) == skipped, R


def test_one_row_of_a_narrow_view():
    """One row of a (1, 8) tensor expanded to (4, 8) has row stride 0, which is never read: rays[2:3] gives the accumulator of its
    contiguous copy through bn_dsm_splat as through bn_dsm_splat_world."""
    from brdf_nerf_amd import _lib as L
    from brdf_nerf_amd import functions as Fn
    row, t = D._one_point()
    rays = torch.from_numpy(row.copy()).to(DEV).expand(4, 8)
    depth = torch.from_numpy(t.copy()).to(DEV).expand(4).contiguous()
    assert rays.stride(0) == 0 and rays[2:3].shape == (1, 8)
    xoff, yoff, res, W, H = D.SMALL
    grid = (D.CENTER, D.RANGE, xoff, yoff, res, 1, L.BN_DSM_DISC)
    for name, splat in (("dsm_splat", lambda r, d, a, s: Fn.dsm_splat(r, d, *grid, a, s)),
                        ("dsm_splat_world", lambda r, d, a, s: Fn.dsm_splat_world(r, d, *grid, L.BN_CS_UTM, 1, 0, a, s))):
        got, want = (torch.zeros((H, W, 2), dtype=torch.int64, device=DEV) for _ in range(2))
        sk = torch.zeros((1,), dtype=torch.int64, device=DEV)
        splat(rays[2:3], depth[2:3], got, sk)
        splat(rays[2:3].contiguous(), depth[2:3], want, sk)
        assert int(want[..., 1].sum()) == 5 and int(sk) == 0, name
        assert torch.equal(got, want), name


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second device")
def test_a_device_that_is_not_the_current_one():
    """bn_dsm_splat and bn_dsm_resolve launch on the stream of the tensors' device, whichever device is current."""
    from brdf_nerf_amd import DsmAccumulator, Grid
    name = "small_R65_r1_disc"
    grid, radius, footprint, rays, depth = D.case(name)
    want = D.expected(name)
    other = torch.device("cuda", 1)
    with torch.cuda.device(0):
        acc = DsmAccumulator(Grid(*grid), other, radius=radius, footprint=footprint)
        acc.add(torch.from_numpy(rays.copy()).to(other), torch.from_numpy(depth.copy()).to(other), frame())
        dsm, count = acc.result()
        torch.cuda.synchronize(other)
    got = acc.acc.cpu().numpy()
    assert np.array_equal(got[..., 0], want["sums"]) and np.array_equal(got[..., 1], want["counts"]) and acc.skipped == want["skipped"]
    assert np.array_equal(dsm.cpu().numpy().view(np.int32), want["dsm"].view(np.int32)) and np.array_equal(count.cpu().numpy(), want["count"])
