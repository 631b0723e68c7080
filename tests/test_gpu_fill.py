"""GPU tests of the hole filling (brdf_nerf_amd/fill.py, bn_grid_nearest_col / bn_grid_fill).  Run on the MI355X box with
`pytest -m gpu`.  Cases and the integer statement they are held to: tests/fill_cases.py."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fill_cases as F
from test_gpu_parity import DEV, _free_port

pytestmark = pytest.mark.gpu


def dev(u):
    return torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32).copy()).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()          # float32 compared bitwise: NaN payloads included


def run(u, rows=None):
    """Both launches on a numpy grid -> near_row, dst bits, source, dist2, counts as numpy."""
    from brdf_nerf_amd import functions as Fn
    src = dev(u)
    near = Fn.grid_nearest_col(src)
    dst, source, dist2, counts = Fn.grid_fill(src, near, rows=rows, want_source=True, want_dist2=True)
    return near.cpu().numpy(), bits(dst), source.cpu().numpy(), dist2.cpu().numpy(), counts.cpu().numpy()


def check(u, what):
    near, dst, source, dist2, counts = run(u)
    filled, wsource, wdist2 = F.statement(u)
    assert near.dtype == np.int32 and np.array_equal(near, F.near_rows(u)), what
    assert np.array_equal(dst, F.bits(filled)), what
    assert source.dtype == np.int32 and np.array_equal(source, wsource), what
    assert dist2.dtype == np.int32 and np.array_equal(dist2, wdist2), what
    assert counts.tolist() == list(F.counts(u)), what


@pytest.mark.parametrize("name", list(F.CASES))
def test_bit_equal_to_the_statement(name):
    """near_row equals the restatement of the column pass; dst, source and dist2 equal the brute force bit for bit in every
    cell; counts = (holes, largest d2).  The 40 x 600 case scans a whole row, the tie cases catch a wrong order or a side
    dropped at dx^2 >= best."""
    check(F.CASES[name], name)


def test_every_3x3_pattern():
    """All 511 non-empty known / hole patterns of a 3 x 3 grid: exhaustive over the tie orientations."""
    for n, u in enumerate(F.patterns_3x3()):
        check(u, n + 1)
    _, _, source, _, _ = run(F.tie_pair())
    assert source[1, 1] == 1 * 3 + 2


def test_random_4x5_patterns():
    for n, u in enumerate(F.patterns_4x5()):
        check(u, n)


@pytest.mark.parametrize("name,a,b", [("33x65", 7, 20), ("31x257", 1, 30), ("33x65", 0, 33)])
def test_row_bands_concatenate_to_the_whole(name, a, b):
    """Rows [0, a), [a, b), [b, H) filled on their own: the bands concatenate to the whole bit for bit, the hole counts add and
    the largest d2 is the maximum of the bands'."""
    u = F.CASES[name]
    H = u.shape[0]
    _, dst, source, dist2, counts = run(u)
    parts = [run(u, rows=r) + (r,) for r in ((0, a), (a, b), (b, H))]
    for k, whole in ((1, dst), (2, source), (3, dist2)):
        assert np.array_equal(np.concatenate([p[k][p[5][0]:p[5][1]] for p in parts]), whole)
    assert sum(int(p[4][0]) for p in parts) == counts[0] and max(int(p[4][1]) for p in parts) == counts[1]
    from brdf_nerf_amd import fill_holes
    whole = fill_holes(dev(u), want_source=True)
    band = fill_holes(dev(u), rows=(a, b), want_source=True)
    assert np.array_equal(bits(band["filled"])[a:b], bits(whole["filled"])[a:b])
    assert np.array_equal(bits(band["filled"])[:a], F.bits(u)[:a]) and (band["source"][b:] == -1).all()
    assert band["holes"] == int(np.isnan(u[a:b]).sum())


@pytest.mark.parametrize("name", F.GOLDENS)
def test_fill_holes_against_the_reference(name):
    """fill_holes on a golden: the two assertions of the CPU test against the reference's output, and the statement bitwise in
    every cell; apply_fill(dsm, source) is `filled`."""
    from brdf_nerf_amd import apply_fill, fill_holes
    g = F.golden(name)
    out = fill_holes(dev(g["u"]), want_source=True)
    filled, wsource, wdist2 = F.statement(g["u"])
    assert out["filled"].dtype == torch.float32 and np.array_equal(bits(out["filled"]), F.bits(filled))
    assert out["source"].dtype == torch.int32 and np.array_equal(out["source"].cpu().numpy(), wsource)
    assert out["holes"] == int(np.isnan(g["u"]).sum()) and out["max_dist"] == math.sqrt(int(wdist2.max()))
    unique, ties = F.against_reference(g["u"], out["filled"].cpu().numpy(), wdist2, g["ref"])
    assert unique >= 400 and ties >= 200
    assert np.array_equal(bits(apply_fill(dev(g["u"]), out["source"])), bits(out["filled"]))
    count = torch.arange(g["u"].size, dtype=torch.int32, device=DEV).reshape(g["u"].shape)
    assert torch.equal(apply_fill(count, out["source"]), out["source"])
    assert "source" not in fill_holes(dev(g["u"]))


def test_dsm_image_with_fill():
    """dsm_image(fill=True) on the small Lambertian model of test_gpu_dsm.py: dsm, count, depth and skipped are bitwise those of
    fill=False after the same seed; dsm_grid is fill_holes(dsm)'s, has no NaN and equals dsm wherever dsm is not NaN."""
    from brdf_nerf_amd import dsm_image, fill_holes
    from test_gpu_dsm import frame
    from test_gpu_relight import build, flags
    cfg, args, models, rays = build("lambert")
    fl, cosi = flags("lambert")
    kw = dict(chunk=128, cos_irra_on=cosi, **fl)
    torch.manual_seed(29)
    plain = dsm_image(models, args, rays, frame(), **kw)
    torch.manual_seed(29)
    got = dsm_image(models, args, rays, frame(), fill=True, **kw)
    assert set(got) == set(plain) | {"dsm_grid", "holes", "max_dist"}
    assert np.array_equal(bits(got["dsm"]), bits(plain["dsm"])) and torch.equal(got["count"], plain["count"])
    assert torch.equal(got["depth"], plain["depth"]) and got["skipped"] == plain["skipped"] and got["grid"] == plain["grid"]
    want = fill_holes(plain["dsm"])
    assert np.array_equal(bits(got["dsm_grid"]), bits(want["filled"]))
    assert got["holes"] == want["holes"] == int(torch.isnan(plain["dsm"]).sum()) > 0 and got["max_dist"] == want["max_dist"] >= 1.0
    assert not torch.isnan(got["dsm_grid"]).any()
    known = ~torch.isnan(plain["dsm"])
    assert np.array_equal(bits(got["dsm_grid"][known]), bits(plain["dsm"][known]))


def test_refusals():
    """BN_EINVAL, not a launch, through the raw ABI: null src, near_row or dst, H or W < 1 or > 8192, rows outside [0, H] or
    row0 > row1.  ValueError from fill_holes on a grid without a known cell."""
    from brdf_nerf_amd import _lib as L
    from brdf_nerf_amd import fill_holes
    lib = L.lib()
    src = dev(F.CASES["12x14_empty_columns"])
    near = torch.full((12, 14), -7, dtype=torch.int32, device=DEV)
    dst = torch.full((12, 14), -7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())

    def col(s=p(src), H=12, W=14, n=p(near)):
        return lib.bn_grid_nearest_col(s, H, W, n, None)

    for kw in (dict(s=None), dict(n=None), dict(H=0), dict(W=0), dict(H=-3), dict(H=8193), dict(W=8193)):
        assert col(**kw) == -1, kw
        assert b"grid_nearest_col" in lib.bn_last_error()

    def fill(s=p(src), n=p(near), H=12, W=14, row0=0, row1=12, d=p(dst)):
        return lib.bn_grid_fill(s, n, H, W, row0, row1, d, None, None, None, None)

    for kw in (dict(s=None), dict(n=None), dict(d=None), dict(H=0), dict(W=0), dict(W=-1), dict(H=8193), dict(W=8193), dict(row0=-1),
               dict(row1=13), dict(row0=5, row1=4), dict(row0=13, row1=13)):
        assert fill(**kw) == -1, kw
        assert b"grid_fill" in lib.bn_last_error()
    assert fill(row0=6, row1=6) == 0                             # an empty band is accepted and launches nothing
    torch.cuda.synchronize()
    assert (near == -7).all() and (dst == -7.0).all()            # nothing was written by any refused call
    assert col() == 0 and fill() == 0                            # the same arguments, accepted (source, dist2, counts NULL)
    torch.cuda.synchronize()
    assert np.array_equal(bits(dst), F.bits(F.statement(F.CASES["12x14_empty_columns"])[0]))
    with pytest.raises(ValueError, match="no known cell"):
        fill_holes(dev(F.ALL_NAN))
    for bad, what in ((dev(F.ALL_NAN).double(), "float32"), (dev(F.ALL_NAN)[:, ::2], "contiguous"), (dev(F.ALL_NAN)[0], "2-D"),
                      (torch.from_numpy(F.ALL_NAN), "device")):
        with pytest.raises(ValueError, match=what):
            fill_holes(bad)


def test_two_rank_fill_matches_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_fill_worker.py), each child under its own time limit and started once:
    the gathered row bands and the merged counts are the single process's filled grid, source map, holes and max_dist, bitwise."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_fill_worker.py")
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
