"""GPU tests of the orthorectified maps (brdf_nerf_amd/ortho.py; bn_ortho_top / bn_ortho_splat / bn_ortho_resolve).  Run on the
MI355X box with `pytest -m gpu`.  Everything is held to the Python-integer statement of tests/ortho_cases.py BIT FOR BIT: top,
acc, the three counters, maps, dsm and count, NaN pattern included - the rule is integer after a float64 chain rounded operation
by operation, and there is no upstream counterpart to compare the feature channels with."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dsm_cases as D
import ortho_cases as O
from test_gpu_parity import DEV, _free_port

pytestmark = pytest.mark.gpu

I64 = dict(dtype=torch.int64, device=DEV)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # a copy: the shared inputs are read-only


def frame():
    from brdf_nerf_amd import SceneFrame
    return SceneFrame(D.CENTER, D.RANGE)


def bits(t):
    return t.contiguous().view(torch.int32)


def accumulate(rays, depth, feats, grid, radius, footprint, mode, band, order=None, chunk=None, fr=None, into=None):
    """Both passes over the rows (in `order`, `chunk` rows per call) in a fresh accumulator, or `into` one whose pass 1 is done."""
    from brdf_nerf_amd import Grid, OrthoAccumulator
    rays, depth, feats = (t if torch.is_tensor(t) else dev(t) for t in (rays, depth, feats))
    if order is not None:
        rays, depth, feats = rays[order].contiguous(), depth[order].contiguous(), feats[order].contiguous()
    fr = fr or frame()
    R, E = feats.shape
    acc = into or OrthoAccumulator(Grid(*grid), DEV, E, radius=radius, footprint=footprint, mode=mode, band=band)
    step = chunk or max(R, 1)
    if mode == "top" and into is None:
        for i in range(0, R, step):
            acc.add_top(rays[i:i + step], depth[i:i + step], fr)
    for i in range(0, R, step):
        acc.add(rays[i:i + step], depth[i:i + step], fr, feats[i:i + step] if E else None)
    return acc


def check(acc, want, what=""):
    got = acc.acc.cpu().numpy()
    maps, dsm, count = (t.cpu().numpy() for t in acc.result())
    counters = [acc.skipped, acc.bad_features, acc.culled]
    print(f"{what}: acc cells with other bits {int((got != want['acc']).any(-1).sum())} of {got.shape[0] * got.shape[1]}, counters {counters} "
          f"(statement {want['counters']}), map values with other bits {int((maps.view(np.int32) != want['maps'].view(np.int32)).sum())}, "
          f"dsm {int((dsm.view(np.int32) != want['dsm'].view(np.int32)).sum())}, deposits {int(want['acc'][..., 1].sum())}")
    assert got.shape == want["acc"].shape and got.dtype == np.int64
    if want["top"] is not None:
        assert np.array_equal(acc.top.cpu().numpy(), want["top"]), what
        assert int(acc._top_skipped) == want["top_skipped"], what
    else:
        assert acc.top is None
    assert np.array_equal(got, want["acc"]), what
    assert counters == want["counters"], what
    assert maps.dtype == np.float32 and maps.shape == want["maps"].shape and np.array_equal(np.isnan(maps), np.isnan(want["maps"])), what
    assert np.array_equal(maps.view(np.int32), want["maps"].view(np.int32)), what
    assert np.array_equal(dsm.view(np.int32), want["dsm"].view(np.int32)), what
    assert count.dtype == np.int32 and np.array_equal(count, want["count"]), what


# ----------------------------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("c", O.SWEEP, ids=O.sweep_id)
def test_bit_equal_to_the_statement(c):
    R, E, gname, radius, footprint, mode = c
    grid, rays, depth, feats = O.sweep_case(c)
    check(accumulate(rays, depth, feats, grid, radius, footprint, mode, O.SWEEP_BAND), O.sweep_expected(c), O.sweep_id(c))


def test_features_as_a_strided_column_slice():
    """The features as columns 2:19 of a (R, 24) tensor: read in place (no copy is made: the slice's own storage is passed)."""
    c = (257, 17, "33x65", 4, "disc", "top")
    grid, rays, depth, feats = O.sweep_case(c)
    wide = torch.full((257, 24), float("nan"), device=DEV)
    wide[:, 2:19] = dev(feats)
    view = wide[:, 2:19]
    assert view.stride() == (24, 1) and not view.is_contiguous()
    check(accumulate(rays, depth, view, grid, 4, "disc", "top", O.SWEEP_BAND), O.sweep_expected(c), "strided features")
    rays11 = torch.full((257, 11), float("nan"), device=DEV)           # and the rays as rows of 11 floats
    rays11[:, :8] = dev(rays)
    check(accumulate(rays11[:, :8], depth, view, grid, 4, "disc", "top", O.SWEEP_BAND), O.sweep_expected(c), "strided rays and features")


def test_contention_and_outside_centres():
    """300 rays on a 3 x 3 grid (every cell takes most of them, 7 sums each); centre cells outside the grid whose footprint
    reaches in; negative altitudes and features, -0.0, denormals, +-(2^16 - ulp)."""
    grid, rays, depth, feats = O.contention_case()
    assert (O.statement(rays, depth, feats, grid, 1, "disc")["count"] > 60).all()
    for mode in ("mean", "top"):
        check(accumulate(rays, depth, feats, grid, 1, "disc", mode, 2.0), O.statement(rays, depth, feats, grid, 1, "disc", mode, 2.0),
              "contention " + mode)
    grid, rays, depth, feats = O.outside_case()
    want = O.statement(rays, depth, feats, grid, 2, "square", "top", 0.75)
    cells = O._cells(rays, depth, grid, 2, O.CENTER, O.RANGE)
    outside = [c for c in cells if c and not (0 <= c[0] < grid[3] and 0 <= c[1] < grid[4])]
    assert len(outside) >= 10 and (D.points(rays, depth)[:, 2] < 0).any() and (np.signbit(feats) & (feats == 0)).any()
    check(accumulate(rays, depth, feats, grid, 2, "square", "top", 0.75), want, "centres outside")


def test_bad_features_and_bad_points():
    """A NaN, an inf, a -inf, a 2^16 and a -2^16 feature: each ray counted in bad_features, nothing deposited, and the other rays'
    bits unchanged.  A bad point together with a bad feature is counted once, as a bad point."""
    c = (257, 3, "7x9", 2, "disc", "mean")
    grid, rays, depth, feats = O.sweep_case(c)
    cells = O._cells(rays, depth, grid, 2, O.CENTER, O.RANGE)
    good = [k for k, cell in enumerate(cells) if cell][:5]
    badp = [k for k, cell in enumerate(cells) if cell is None][:2]
    far = [k for k, cell in enumerate(cells) if cell == ()][:1]
    assert len(good) == 5 and len(badp) == 2
    f = feats.copy()
    for k, v in zip(good, (np.nan, np.inf, -np.inf, 65536.0, -65536.0)):
        f[k, k % 3] = v
    f[badp[0], 1] = np.nan                                                # a bad point AND a bad feature
    for k in far:
        f[k, 0] = np.inf                                                  # out of reach of the grid, still a bad feature
    for mode in ("mean", "top"):
        want = O.statement(rays, depth, f, grid, 2, "disc", mode, O.SWEEP_BAND)
        clean = O.sweep_expected(c) if mode == "mean" else O.statement(rays, depth, feats, grid, 2, "disc", mode, O.SWEEP_BAND)
        assert want["counters"][0] == clean["counters"][0] == 5 and want["counters"][1] == 5 + len(far)
        check(accumulate(rays, depth, f, grid, 2, "disc", mode, O.SWEEP_BAND), want, "bad features " + mode)
    # the other rays' bits: the same rows without the bad ones
    keep = np.array([k for k in range(len(rays)) if k not in good and k not in far])
    rest = accumulate(rays[keep], depth[keep], f[keep], grid, 2, "disc", "mean", 0.0)
    whole = accumulate(rays, depth, f, grid, 2, "disc", "mean", 0.0)
    assert torch.equal(rest.acc, whole.acc) and rest.skipped == whole.skipped and rest.bad_features == 0


# --------------------------------------------------------------------------------------------------- the altitude part is the DSM's
@pytest.mark.parametrize("name", ["small_R65_r1_disc", "large_R300_r2_square", "contention_R4096_r1_disc"])
def test_without_channels_the_accumulator_is_the_dsm_accumulator(name):
    from brdf_nerf_amd import DsmAccumulator, Grid
    grid, radius, footprint, rays, depth = D.case(name)
    rays, depth = dev(rays), dev(depth)
    ours = accumulate(rays, depth, torch.zeros((len(rays), 0), device=DEV), grid, radius, footprint, "mean", 0.0)
    dsm = DsmAccumulator(Grid(*grid), DEV, radius=radius, footprint=footprint).add(rays, depth, frame())
    assert int(dsm.acc[..., 1].sum()) > 0 and torch.equal(ours.acc, dsm.acc) and ours.skipped == dsm.skipped == D.expected(name)["skipped"]
    maps, d, count = ours.result()
    assert tuple(maps.shape) == (0,) + tuple(d.shape)
    assert torch.equal(bits(d), bits(dsm.result()[0])) and torch.equal(count, dsm.result()[1])


def test_without_channels_on_an_ecef_frame():
    """cs = ecef: bn_dsm_splat_world's accumulator bit for bit (the same device functions), refused rows included; and with three
    channels the (sum_z, count) columns are still that accumulator."""
    import ecef_cases as E
    from brdf_nerf_amd import DsmAccumulator, Grid
    from test_gpu_ecef import ecef_frame, site_inputs
    name = "z21s"
    fr = ecef_frame(name)
    rays, depth = site_inputs(name)
    depth = depth.clone()
    depth[5], depth[70] = float("nan"), float("inf")
    grid = E.cloud_grid(E.site_statement(name)["enz"])
    dsm = DsmAccumulator(Grid(*grid), DEV).add(rays, depth, fr)
    ours = accumulate(rays, depth, torch.zeros((len(rays), 0), device=DEV), grid, 1, "disc", "mean", 0.0, fr=fr)
    assert dsm.skipped == 2 and torch.equal(ours.acc, dsm.acc) and ours.skipped == 2
    feats = dev(O.features_for(len(rays), 3, 41))
    three = accumulate(rays, depth, feats, grid, 1, "disc", "mean", 0.0, fr=fr, chunk=100)
    assert torch.equal(three.acc[..., :2], dsm.acc) and three.skipped == 2
    wide = accumulate(rays, depth, feats, grid, 1, "disc", "top", 1.0e4, fr=fr)           # a band above any relief: nothing culled
    assert torch.equal(wide.acc, three.acc) and wide.culled == 0 and int(wide.top.max()) > O.EMPTY


# ------------------------------------------------------------------------------------------------------------------ top mode
def block(mode, band, **kw):
    s = O.block_scene()
    return accumulate(s["rays"], s["depth"], s["features"], s["grid"], 1, "disc", mode, band, **kw)


def test_top_mode_on_the_block_scene():
    """The block seen 30 degrees off nadir: mean mode, top mode at the scene's band of 1 m, band 0, and a top grid left at EMPTY."""
    from brdf_nerf_amd import Grid, OrthoAccumulator
    s = O.block_scene()
    check(block("mean", 0.0), s["mean"], "block, mean")
    top = block("top", O.BLOCK_BAND)
    check(top, s["top"], "block, top, band 1 m")
    assert top.culled == O.BLOCK_CONDITIONS["culled"] > 0
    roof = torch.tensor(O.BLOCK_COLOURS["roof"], device=DEV)
    maps = top.result()[0]
    for j in O.ROOF_ROWS:
        for i in O.ROOF_COLS:
            assert torch.equal(maps[:, j, i], roof), (j, i)
    check(block("top", 0.0), O.statement(s["rays"], s["depth"], s["features"], s["grid"], 1, "disc", "top", 0.0), "block, top, band 0")
    empty = OrthoAccumulator(Grid(*s["grid"]), DEV, 3, mode="top", band=0.0)              # pass 1 never run: EMPTY passes everything
    accumulate(s["rays"], s["depth"], s["features"], s["grid"], 1, "disc", "top", 0.0, into=empty)
    assert int(empty.top.max()) == O.EMPTY and empty.culled == 0 and torch.equal(empty.acc, block("mean", 0.0).acc)


def test_the_band_boundary_is_kept():
    """q + band_q == top exactly: kept.  Two points of equal q at the top: both kept, at band 0 too."""
    grid, rays, depth, feats, band = O.boundary_case()
    cells = O._cells(rays, depth, grid, 0, O.CENTER, O.RANGE)
    qs = [c[2] for c in cells]
    assert len({c[:2] for c in cells}) == 1 and qs[0] == qs[1] == qs[2] + O.band_q(band) and qs[3] + O.band_q(band) < qs[0]
    for radius in (0, 1):
        want = O.statement(rays, depth, feats, grid, radius, "disc", "top", band)
        j, i = cells[0][1], cells[0][0]
        assert want["count"][j, i] == 3 and want["counters"][2] == (1 if radius == 0 else 5)
        check(accumulate(rays, depth, feats, grid, radius, "disc", "top", band), want, f"boundary, radius {radius}")
        zero = O.statement(rays, depth, feats, grid, radius, "disc", "top", 0.0)
        assert zero["count"][j, i] == 2
        check(accumulate(rays, depth, feats, grid, radius, "disc", "top", 0.0), zero, f"band 0, radius {radius}")


# ------------------------------------------------------------------------------------------- order, chunks, views and ranks
def test_split_invariance_is_bitwise():
    """Shuffled rays and chunks of 1, 64 and 100 in both passes: one result.  Two views in one accumulator: their concatenation."""
    s = O.block_scene()
    R = len(s["rays"])
    whole = block("top", O.BLOCK_BAND)
    perm = torch.from_numpy(np.random.RandomState(9).permutation(R)).to(DEV)
    runs = {"shuffled": block("top", O.BLOCK_BAND, order=perm), "chunks of 1": block("top", O.BLOCK_BAND, chunk=1),
            "chunks of 64": block("top", O.BLOCK_BAND, chunk=64), "chunks of 100": block("top", O.BLOCK_BAND, chunk=100),
            "shuffled, chunks of 64": block("top", O.BLOCK_BAND, order=perm, chunk=64)}
    for what, a in runs.items():
        assert torch.equal(a.top, whole.top) and torch.equal(a.acc, whole.acc), what
        assert (a.skipped, a.bad_features, a.culled) == (whole.skipped, whole.bad_features, whole.culled), what
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a.result(), whole.result())), what
    # a second view: the rays of the contention case moved over the block's grid, with colours of their own
    from brdf_nerf_amd import Grid, OrthoAccumulator
    _, r2, d2, f2 = O.contention_case()
    r2 = r2.copy()
    r2[:, 0] += np.float32(-4.0 / O.RANGE)                     # over the ground west of the block, some of it higher
    f2 = f2[:, :3]
    both = OrthoAccumulator(Grid(*s["grid"]), DEV, 3, mode="top", band=O.BLOCK_BAND)
    fr = frame()
    both.add_top(dev(s["rays"]), dev(s["depth"]), fr).add_top(dev(r2), dev(d2), fr)
    both.add(dev(s["rays"]), dev(s["depth"]), fr, dev(s["features"])).add(dev(r2), dev(d2), fr, dev(f2))
    cat = (np.concatenate([s["rays"], r2]), np.concatenate([s["depth"], d2]), np.concatenate([s["features"], f2]))
    want = O.statement(*cat, s["grid"], 1, "disc", "top", O.BLOCK_BAND)
    assert int((want["acc"] != s["top"]["acc"]).any(-1).sum()) > 5
    check(both, want, "two views")


def test_two_rank_ortho_matches_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_ortho_worker.py), each child under its own time limit and started once."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_ortho_worker.py")
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


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    """BN_EINVAL, nothing launched: the buffers are as they were."""
    from brdf_nerf_amd import _lib as L
    lib = L.lib()
    R, E, W, H = 4, 3, 7, 5
    rays, depth = torch.zeros(R, 8, device=DEV), torch.ones(R, device=DEV)
    rays[:, 5] = -1.0                                          # every ray's point is 1 m west of the centre, inside SMALL: an accepted call deposits
    feats = torch.ones(R, 4, device=DEV)
    acc, top, counters = torch.zeros(H, W, 2 + E, **I64), torch.full((H, W), O.EMPTY, **I64), torch.zeros(3, **I64)
    c = (C.c_double * 3)(D.CENTER[0] - 1.0, D.CENTER[1], D.CENTER[2] + D.RANGE)
    p = lambda t: C.c_void_p(t.data_ptr())
    odd = C.c_void_p(acc.data_ptr() + 8)

    def splat(radius=1, res=0.5, W=W, H=H, fp=0, cs=L.BN_CS_UTM, zone=17, south=0, stride=8, rays_p=p(rays), depth_p=p(depth), center=c,
              feats_p=p(feats), fs=4, E=E, top_p=p(top), band=0, acc_p=p(acc), cnt=p(counters), R=R, rng=D.RANGE):
        return lib.bn_ortho_splat(rays_p, stride, depth_p, R, center, rng, D.SMALL[0], D.SMALL[1], res, W, H, radius, fp, cs, zone, south,
                                  feats_p, fs, E, top_p, band, acc_p, cnt, None)

    def first(radius=1, res=0.5, W=W, H=H, fp=0, cs=L.BN_CS_UTM, zone=17, south=0, stride=8, rays_p=p(rays), top_p=p(top), sk=p(counters), R=R):
        return lib.bn_ortho_top(rays_p, stride, p(depth), R, c, D.RANGE, D.SMALL[0], D.SMALL[1], res, W, H, radius, fp, cs, zone, south,
                                top_p, sk, None)

    for kw in (dict(rays_p=None), dict(depth_p=None), dict(center=None), dict(acc_p=None), dict(cnt=None), dict(E=-1), dict(E=33),
               dict(fs=2), dict(band=-1), dict(feats_p=None), dict(acc_p=odd), dict(radius=-1), dict(radius=5), dict(res=0.0),
               dict(res=float("nan")), dict(fp=2), dict(W=0), dict(W=1 << 16, H=(1 << 15) + 1), dict(cs=2), dict(zone=0), dict(zone=61),
               dict(south=2), dict(stride=5), dict(R=-1), dict(rng=float("inf"))):
        assert splat(**kw) == -1 and b"ortho_splat" in lib.bn_last_error(), kw
    for kw in (dict(rays_p=None), dict(top_p=None), dict(sk=None), dict(radius=5), dict(res=-0.5), dict(fp=-1), dict(H=0), dict(cs=-1),
               dict(zone=61), dict(south=-1), dict(stride=3), dict(R=-2)):
        assert first(**kw) == -1 and b"ortho_top" in lib.bn_last_error(), kw
    maps, dsm = torch.full((E, H, W), 7.0, device=DEV), torch.full((H, W), 7.0, device=DEV)
    for args in ((None, W, H, E, p(maps), p(dsm)), (p(acc), W, H, E, None, p(dsm)), (p(acc), W, H, E, p(maps), None),
                 (p(acc), W, H, 33, p(maps), p(dsm)), (p(acc), W, H, -1, p(maps), p(dsm)), (p(acc), 0, H, E, p(maps), p(dsm)),
                 (odd, W, H, E, p(maps), p(dsm))):
        assert lib.bn_ortho_resolve(*args, None, None) == -1 and b"ortho_resolve" in lib.bn_last_error(), args
    torch.cuda.synchronize()
    assert int(acc.abs().sum()) == 0 and int(counters.abs().sum()) == 0 and int(top.max()) == O.EMPTY
    assert bool((maps == 7.0).all()) and bool((dsm == 7.0).all())
    # and the accepted calls do write: E == 0 takes no features, a band beyond 2^62 is a band
    assert first() == 0 and splat() == 0 and splat(band=(1 << 63) - 1) == 0
    assert lib.bn_ortho_splat(p(rays), 8, p(depth), R, c, D.RANGE, D.SMALL[0], D.SMALL[1], 0.5, W, H, 1, 0, L.BN_CS_UTM, 17, 0, None, 0, 0,
                              None, 0, p(torch.zeros(H, W, 2, **I64)), p(counters), None) == 0
    assert lib.bn_ortho_resolve(p(acc), W, H, E, p(maps), p(dsm), None, None) == 0
    torch.cuda.synchronize()
    assert int(acc[..., 1].sum()) == 2 * R * 5 and int(top.max()) > O.EMPTY and int(counters.sum()) == 0
    assert bool(torch.isnan(dsm).any()) and int(torch.isfinite(maps[0]).sum()) == 5


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_ortho_image_end_to_end():
    """The 12 x 10 view of test_gpu_maps.py, an RPV model with analytic normals.  After the same seed: ortho_image's dsm in mean
    mode is bitwise dsm_image's; rgb and depth are bitwise view_maps'; the maps equal the statement applied to view_maps'
    outputs, in mean and in top mode; fill=True gives every layer through ONE source map with no NaN left."""
    from brdf_nerf_amd import apply_fill, dsm_image, ortho_image, view_maps
    from test_gpu_maps import CHUNK, VIEW_H, VIEW_W, view_case
    args, models, rays, fl = view_case("rpv_an")
    H, W, seed = VIEW_H, VIEW_W, 23
    keys = ("rgb", "albedo", "normal_an", "rpv_k", "rpv_theta", "rpv_rhoc", "depth_std")
    torch.manual_seed(seed)
    vm = view_maps(models, args, rays, H, W, chunk=CHUNK, **fl)["maps"]
    torch.manual_seed(seed)
    ref = dsm_image(models, args, rays, frame(), chunk=CHUNK, **fl)
    torch.manual_seed(seed)
    mean = ortho_image(models, args, rays, H, W, frame(), keys=keys, mode="mean", chunk=CHUNK, **fl)
    assert mean["grid"] == ref["grid"] and torch.equal(bits(mean["dsm"]), bits(ref["dsm"])) and torch.equal(mean["count"], ref["count"])
    assert mean["skipped"] == ref["skipped"] and mean["culled"] == 0 and mean["bad_features"] == 0
    assert torch.equal(mean["rgb"], vm["rgb"]) and torch.equal(mean["depth"], vm["depth"]) and torch.equal(mean["depth"], ref["depth"])
    feats = torch.cat([vm[k].reshape(H * W, -1) for k in keys], 1)
    E = feats.shape[1]
    assert 13 <= E == sum(d for _, d in mean["channels"].values()) and list(mean["channels"]) == list(keys)
    assert mean["channels"]["rgb"] == (0, 3) and mean["channels"]["depth_std"] == (E - 1, 1)
    g = mean["grid"]
    grid = (g.xoff, g.yoff, g.resolution, g.width, g.height)
    npy = lambda t: t.detach().cpu().numpy()
    torch.manual_seed(seed)
    top = ortho_image(models, args, rays, H, W, frame(), grid=g, keys=keys, mode="top", band=0.25, fill=True, chunk=CHUNK, **fl)
    for res, mode, band in ((mean, "mean", 0.0), (top, "top", 0.25)):
        want = O.statement(npy(rays), npy(vm["depth"]), npy(feats), grid, 1, "disc", mode, band)
        got = torch.cat([res["maps"][k] for k in keys], 0)
        assert tuple(got.shape) == (E, g.height, g.width) and int(want["count"].sum()) > H * W
        assert np.array_equal(npy(got).view(np.int32), want["maps"].view(np.int32)), mode
        assert np.array_equal(npy(res["dsm"]).view(np.int32), want["dsm"].view(np.int32)) and np.array_equal(npy(res["count"]), want["count"])
        assert [res["skipped"], res["bad_features"], res["culled"]] == want["counters"], mode
    assert top["culled"] > 0 and top["grid"] is g
    # the fill: one source map for the dsm and every channel
    src = top["source"]
    assert top["holes"] == int(torch.isnan(top["dsm"]).sum()) > 0 and bool(torch.isfinite(top["dsm_grid"]).all())
    assert torch.equal(bits(top["dsm_grid"]), bits(apply_fill(top["dsm"], src)))
    for k in keys:
        layer, filled = top["maps"][k], top["maps_grid"][k]
        assert filled.shape == layer.shape and bool(torch.isfinite(filled).all()), k
        for d in range(layer.shape[0]):
            assert torch.equal(bits(filled[d]), bits(apply_fill(layer[d], src))), k
    # refused by name
    with pytest.raises(ValueError, match="hpk_b"):
        ortho_image(models, args, rays, H, W, frame(), keys=("rgb", "hpk_b"), chunk=CHUNK, **fl)
    with pytest.raises(ValueError, match="no_such_map"):
        ortho_image(models, args, rays, H, W, frame(), keys=("no_such_map",), chunk=CHUNK, **fl)
    with pytest.raises(ValueError, match="32"):
        ortho_image(models, args, rays, H, W, frame(), keys=("rgb",) * 11, chunk=CHUNK, **fl)
    with pytest.raises(NotImplementedError, match="gsam_only"):
        ortho_image(models, args, rays, H, W, frame(), gsam_only=True, chunk=CHUNK, **fl)
