"""GPU tests of the altitude sweep of a surface model (brdf_nerf_amd/sweep.py; bn_grid_sweep).  Run on the MI355X box with
`pytest -m gpu`.  Cases and the numpy float64 statement they are held to: tests/sweep_cases.py.

Fed the STATEMENT's pixels (colrow_in), no transcendental lies between the kernel's inputs and its outputs, and every output must
equal the statement bit for bit.  With the projection inside, the kernel is held to the statement's Welford and argmin applied to
the DEVICE's own per-level pixels and bn_image_gather outputs: the fused launch is the Z K-launch chain's bits.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import camera_cases as K
import mosaic_cases as M
import orthophoto_cases as O
import sweep_cases as S
import visibility_cases as V
from test_gpu_parity import DEV, _free_port

pytestmark = pytest.mark.gpu

MODES = ("bilinear", "nearest")
MAPS = ("cost_min", "altitude")


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).copy()).to(DEV)


def npy(t):
    return t.detach().cpu().numpy()


def rpc_of(d):
    from brdf_nerf_amd import Rpc
    return Rpc.from_dict(d)


def view_table(planes, ds, vis, layout):
    """The K tuples functions.grid_sweep takes: planes K arrays (C, Hi, Wi), ds K descriptors, vis K arrays (H, W) or None."""
    strides = lambda Cn, Hi, Wi: (Wi * Cn, Cn, 1) if layout == "image" else (Wi, 1, Hi * Wi)
    return [(dev(O.to_layout(p, layout)), p.shape[1], p.shape[2], strides(*p.shape), None if v is None else dev(v), 0, rpc_of(d))
            for p, d, v in zip(planes, ds, vis)]


def check(out, want, where, cost=True):
    """Every output of the launch against pick's dictionary: the integers equal, the float maps bit-equal with every NaN as one."""
    n = want["level"].size
    assert np.array_equal(npy(out["level"]).reshape(-1), want["level"].reshape(-1)), where
    assert np.array_equal(npy(out["count"]).reshape(-1), want["count"].reshape(-1)), where
    assert npy(out["valid"]).tolist() == list(want["valid"]), where
    assert npy(out["wins"]).tolist() == list(want["wins"]), where
    assert npy(out["sums"]).tolist() == list(want["sums"]), where
    for key in MAPS:
        assert O.same_f32(npy(out[key]).reshape(-1), want[key].reshape(-1)), f"{where} {key}"
    if cost:
        assert O.same_f32(npy(out["cost"]).reshape(-1, n), want["cost"].reshape(-1, n)), f"{where} cost"


def statement_case(H, W, views, Cn, Z, seed=0):
    """Views of different image sizes over an H x W grid; per level the pixels from random_colrow and edge_colrow; images with NaN,
    payload-NaN, -0.0, denormal and infinite pixels; a mask for every second view; a DSM with NaN cells; offsets that are neither
    sorted nor dyadic, and from Z = 4 on a quarter of the levels repeat an earlier one - pixels and offset: a tie."""
    n = H * W
    rng = np.random.default_rng(seed + 7 * views + Cn + n + 13 * Z)
    distinct = Z - Z // 4
    src = np.concatenate([rng.permutation(distinct), rng.integers(0, distinct, Z - distinct)])
    offsets = (rng.permutation(distinct) * 0.3 - 1.7)[src]
    planes, colrow, vis = [], [], []
    for k in range(views):
        Hi, Wi = M.IMAGE_SIZES[(k + seed) % len(M.IMAGE_SIZES)]
        planes.append(O.random_image(Cn, Hi, Wi, seed=k + seed))
        edge = O.edge_colrow(Hi, Wi)
        per_level = []
        for l in range(distinct):
            cr = O.random_colrow(Hi, Wi, n, seed=k + seed + 50 * l)
            at = rng.permutation(n)[:min(n, len(edge))]
            cr[at] = edge[rng.permutation(len(edge))[:len(at)]]
            per_level.append(cr.reshape(H, W, 2))
        colrow.append(np.stack(per_level))
        vis.append(rng.integers(0, 3, (H, W)).astype(np.uint8) if k % 2 else None)
    colrow = np.ascontiguousarray(np.stack(colrow, 1)[src])                  # (Z, K, H, W, 2)
    dsm = rng.uniform(90.0, 110.0, (H, W)).astype(np.float32)
    dsm[rng.random((H, W)) < 0.05] = np.nan
    ds = [K.make_rpc("z17", k) for k in range(views)]
    return planes, colrow, vis, dsm, offsets, ds


# ------------------------------------------------------------------------------------------------ statement pixels in
@pytest.mark.parametrize("views,Cn,Z,min_views", S.STATEMENT_CASES)
@pytest.mark.parametrize("shape", M.GRIDS)
def test_sweep_bit_equal_to_the_statement(shape, views, Cn, Z, min_views):
    from brdf_nerf_amd import functions as Fn
    H, W = shape
    planes, colrow, vis, dsm, offsets, ds = statement_case(H, W, views, Cn, Z)
    ddsm, dcolrow = dev(dsm), dev(colrow)
    layout = "image" if (views + Z) % 2 else "planes"
    for mode in MODES if Z <= 17 else MODES[views % 2:][:1]:          # Z = 256: one mode per case, bilinear at K = 2, nearest at K = 3
        want = S.pick(S.gathered(planes, colrow, vis, mode), dsm, offsets, min_views)
        out = Fn.grid_sweep(view_table(planes, ds, vis, layout), Cn, ddsm, 0.0, 0.0, 0.5, 17, 0, offsets, min_views=min_views, mode=mode,
                            colrow=dcolrow, want_cost=True)
        check(out, want, f"{H} x {W} K={views} C={Cn} Z={Z} min_views={min_views} {mode} {layout}")
        if Z >= 17 and H * W >= 255 and min_views <= 2:
            later = np.flatnonzero(np.arange(Z) >= Z - Z // 4)               # the repeated levels never win: their first copy does
            assert sum(want["wins"]) > 0 and all(want["wins"][l] == 0 for l in later)


def test_constant_images_tie_at_every_level():
    """Planted constant images: whatever the pixels, every level's cost is the same, and level 0 keeps it."""
    from brdf_nerf_amd import functions as Fn
    H, W, views, Cn, Z = 3, 5, 5, 3, 17
    _, colrow, _, dsm, offsets, ds = statement_case(H, W, views, Cn, Z, seed=2)
    colrow[:] = (2.25, 3.5)                                                  # every view sees every cell at every level
    planes = [M.planted_image(Cn, 5, 7, k) for k in range(views)]
    for mode in MODES:
        want = S.pick(S.gathered(planes, colrow, [None] * views, mode), dsm, offsets, 2)
        assert want["wins"] == [H * W] + [0] * (Z - 1) and (want["cost_min"] > 0).all()
        out = Fn.grid_sweep(view_table(planes, ds, [None] * views, "planes"), Cn, dev(dsm), 0.0, 0.0, 0.5, 17, 0, offsets, mode=mode,
                            colrow=dev(colrow), want_cost=True)
        check(out, want, f"planted {mode}")


# ------------------------------------------------------------------------------------------------ projection inside
def device_levels(table, Cn, dsm64, e, n, offsets, zone, mode, f32_grid=None):
    """The levels of pick from the device's own launches: per level and view the pixels of (e, n, dsm + off) by world_pixels - or, with
    f32_grid = (ddsm_of_level, xoff, yoff, res), by bn_grid_pixels on the float32 grid of that level - and bn_image_gather on them."""
    from brdf_nerf_amd import functions as Fn
    from brdf_nerf_amd import world_pixels
    for l, off in enumerate(offsets):
        values, states = [], []
        pts = torch.stack([e, n, dsm64 + float(off)], -1).reshape(-1, 3).contiguous()
        for img, Hi, Wi, strides, v, _, rpc in table:
            if f32_grid is None:
                colrow, _ = world_pixels(rpc, pts, zone)
            else:
                grids, xoff, yoff, res = f32_grid
                colrow, _ = Fn.grid_pixels(rpc, grids[l], xoff, yoff, res, zone, 0)
            out, state, _ = Fn.image_gather(img, Hi, Wi, Cn, strides, colrow.reshape(-1, 2), v, mode=mode)
            values.append(npy(out))
            states.append(npy(state))
        yield np.stack(values), np.stack(states)


@pytest.mark.parametrize("dyadic", (True, False))
@pytest.mark.parametrize("site", sorted(K.SITES))
@pytest.mark.parametrize("shape", ((3, 5), (33, 65)))
def test_fused_launch_is_the_chain_of_launches(shape, site, dyadic):
    """colrow_in NULL.  dyadic: DSM and offsets are multiples of 2^-4 m below 4096 m, so (float)(dsm + off) is exact and bn_grid_pixels
    on that float32 grid sees the rule's a_l.  Otherwise the offsets are multiples of 0.1 m and the pixels are bn_utm_geodetic +
    bn_rpc_project on the float64 altitudes dsm + off - what bn_grid_pixels equals bit for bit on its own cells."""
    from brdf_nerf_amd import functions as Fn
    H, W = shape
    zone, res, Cn = K.SITES[site][2], 0.5, 3
    dsm = V.relief(H, W, seed=H + W, nan=0.1, low=K.SITES[site][3] - 20.0)
    finite = np.isfinite(dsm)
    dsm[finite] = np.round(dsm[finite] * 16.0) / 16.0
    assert np.isnan(dsm).any() and np.nanmax(np.abs(dsm[finite])) < 4000.0
    offsets = np.array([0.5, -3.0, 0.0, 2.0625, -0.25, 0.5, 7.0]) if dyadic else np.array([0.1, -3.3, 0.0, 2.1, -0.3, 0.1, 7.7])
    xoff, yoff = O.site_grid(site, H, W, res, shift=(137.0, -61.0))
    ds = [K.make_rpc(site, 30 + k) for k in range(3)]
    planes = [O.random_image(Cn, Hi, Wi, seed=k) for k, (Hi, Wi) in enumerate(((640, 640), (600, 550), (528, 720)))]
    vis = [None, np.random.default_rng(H).integers(0, 3, (H, W)).astype(np.uint8), None]
    ddsm = dev(dsm)
    dsm64 = ddsm.double()
    jj, ii = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float64), torch.arange(W, device=DEV, dtype=torch.float64), indexing="ij")
    e, n = xoff + (ii + 0.5) * res, yoff - (jj + 0.5) * res
    f32_grid = None
    if dyadic:
        grids = [(dsm64 + float(o)).float() for o in offsets]
        assert all(torch.equal(g.double()[torch.isfinite(g)], (dsm64 + float(o))[torch.isfinite(g)]) for g, o in zip(grids, offsets))
        f32_grid = (grids, xoff, yoff, res)
    for mode in MODES:
        table = view_table(planes, ds, vis, "image")
        want = S.pick(device_levels(table, Cn, dsm64, e, n, offsets, zone, mode, f32_grid), dsm, offsets, 2)
        out = Fn.grid_sweep(table, Cn, ddsm, xoff, yoff, res, zone, 0, offsets, mode=mode, want_cost=True)
        check(out, want, f"{site} {H} x {W} {mode} dyadic={dyadic}")
        print(f"{site} {H} x {W} {mode} dyadic={dyadic}: valid {want['valid']} wins {want['wins']}")
        assert want["wins"][5] == 0                                          # offsets[5] repeats offsets[0]
        if H * W > 15:
            assert sum(want["wins"]) > 100 and sum(w > 0 for w in want["wins"]) >= 4


def test_one_level_agrees_with_the_mosaic():
    """offsets = [0]: count is bn_grid_mosaic's where that is at least min_views and 0 elsewhere; valid[0] is its sums[0] at 2."""
    from brdf_nerf_amd import functions as Fn
    site, H, W, Cn = "z17", 33, 65, 3
    zone, res = K.SITES[site][2], 0.5
    dsm = dev(V.relief(H, W, seed=5, nan=0.1, low=K.SITES[site][3] - 20.0))
    xoff, yoff = O.site_grid(site, H, W, res)
    ds = [K.make_rpc(site, 30 + k) for k in range(3)]
    planes = [O.random_image(Cn, Hi, Wi, seed=k) for k, (Hi, Wi) in enumerate(((640, 640), (600, 550), (528, 720)))]
    vis = [None, np.random.default_rng(H).integers(0, 3, (H, W)).astype(np.uint8), None]
    table = view_table(planes, ds, vis, "image")
    mosaic = Fn.grid_mosaic(table, Cn, dsm, xoff, yoff, res, zone, 0)
    for min_views in (1, 2, 3):
        got = Fn.grid_sweep(table, Cn, dsm, xoff, yoff, res, zone, 0, [0.0], min_views=min_views)
        enough = mosaic["count"] >= min_views
        assert int(enough.sum()) > 100 and torch.equal(got["count"], torch.where(enough, mosaic["count"], torch.zeros_like(mosaic["count"])))
        assert torch.equal(got["level"], enough.to(torch.int32) - 1) and int(got["valid"][0]) == int(enough.sum()) == int(got["wins"][0])
        if min_views == 2:
            assert int(got["valid"][0]) == int(mosaic["sums"][0])
        variance = (mosaic["std"].double() ** 2).sum(0)                       # the float32 std, squared: the cost up to that rounding
        assert torch.allclose(got["cost_min"].double()[enough], variance[enough], rtol=1e-6, atol=1e-12)
        assert torch.equal(got["altitude"][enough], dsm[enough])


# ------------------------------------------------------------------------------------------------ row bands, want_cost
def test_row_bands_into_one_set_of_buffers():
    from brdf_nerf_amd import functions as Fn
    H, W, views, Cn, Z = 33, 65, 3, 3, 17
    planes, colrow, vis, dsm, offsets, ds = statement_case(H, W, views, Cn, Z, seed=3)
    ddsm, dcolrow = dev(dsm), dev(colrow)
    table = view_table(planes, ds, vis, "image")
    call = lambda **kw: Fn.grid_sweep(table, Cn, ddsm, 0.0, 0.0, 0.5, 17, 0, offsets, colrow=dcolrow, **kw)
    whole = call(want_cost=True)
    check(whole, S.pick(S.gathered(planes, colrow, vis, "bilinear"), dsm, offsets, 2), "whole")
    plain = call()                                                           # want_cost off: the same other outputs
    assert plain["cost"] is None
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    for key in ("level", "count", "valid", "wins", "sums") + MAPS:
        assert torch.equal(bits(plain[key]), bits(whole[key])), key
    for cuts in ((0, 1, H), (0, 13, H)):
        bufs = dict(level=torch.full((H, W), -9, dtype=torch.int32, device=DEV), count=torch.full((H, W), 0xAB, dtype=torch.uint8, device=DEV),
                    cost_min=torch.full((H, W), -3.0, device=DEV), altitude=torch.full((H, W), -3.0, device=DEV),
                    cost=torch.full((Z, H, W), -3.0, device=DEV), valid=torch.zeros(Z, dtype=torch.int64, device=DEV),
                    wins=torch.zeros(Z, dtype=torch.int64, device=DEV), sums=torch.zeros(3, dtype=torch.int64, device=DEV))
        untouched = lambda rows: (bufs["level"][rows] == -9).all() and (bufs["count"][rows] == 0xAB).all() and \
            (bufs["cost"][:, rows] == -3.0).all() and all((bufs[k][rows] == -3.0).all() for k in MAPS)
        call(rows=(5, 5), **bufs)                                            # an empty band writes nothing
        assert untouched(slice(0, H)) and all(int(bufs[k].sum()) == 0 for k in ("valid", "wins", "sums"))
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            assert untouched(slice(r0, H))
            call(rows=(r0, r1), **bufs)
            assert untouched(slice(r1, H))
        for key in ("level", "count", "valid", "wins", "sums", "cost") + MAPS:
            assert torch.equal(bits(bufs[key]), bits(whole[key])), (cuts, key)


# ------------------------------------------------------------------------------------------------ the wrapper
def scene_on_the_device():
    from brdf_nerf_amd import Grid
    ds, planes, dsm, xoff, yoff, res, zone = S.scene()
    views = [(dev(p), p.shape[1], p.shape[2], rpc_of(d)) for p, d in zip(planes, ds)]
    return views, dsm, Grid(xoff, yoff, res, dsm.shape[1], dsm.shape[0]), zone


def test_altitude_sweep_finds_the_planted_error():
    """The box of the scene 6 m too high: the wrapper meets the conditions and the recorded counts of test_sweep_cpu.py, with and
    without occlusion, on dyadic and on non-dyadic offsets; on the true DSM it stays; the refined model is more photo-consistent."""
    from brdf_nerf_amd import altitude_sweep, orthomosaic
    views, dsm, grid, zone = scene_on_the_device()
    raised = dev(M.raised(dsm))
    results = {}
    for which, base, offsets, kw in (("raised", raised, S.SCENE_OFFSETS, {}), ("true", dev(dsm), S.SCENE_OFFSETS, {}),
                                     ("raised_tenth", raised, S.SCENE_OFFSETS + 0.1, {}),
                                     ("raised_unoccluded", raised, S.SCENE_OFFSETS, dict(occlusion=False))):
        got = results[which] = altitude_sweep(views, base, grid, zone, offsets, layout="planes", want_cost=which == "raised", **kw)
        roof, ground, astray, none = S.scene_counts({"level": npy(got["level"])}, dsm, 8 if which == "true" else 2)
        print(f"{which}: roof {roof}, ground {ground}, astray {astray}, none {none}, wins {got['wins']}, mean cost {got['mean_cost']:.6g}")
        want = S.SCENE_RECORD[which]
        assert roof >= 80 and roof + ground >= 1500 and (astray == 0 or which == "raised_unoccluded")
        assert (roof, ground, none) == (want["roof"], want["ground"], want["none"])
        assert got["valid"] == want["valid"] and got["wins"] == want["wins"] and got["cells"] == sum(want["wins"]) and got["skipped"] == 0
        level = got["level"]
        has = level >= 0
        assert torch.equal(got["offset"][has], torch.from_numpy(offsets).to(DEV)[level[has].long()]) and torch.isnan(got["offset"][~has]).all()
        assert torch.equal(got["altitude"][has], (base.double()[has] + got["offset"][has]).float()) and torch.isnan(got["altitude"][~has]).all()
        assert (got["count"][has] >= 2).all() and (got["count"][~has] == 0).all() and torch.isnan(got["cost_min"][~has]).all()
        assert (got["visible"] is None) == (which == "raised_unoccluded")
    got = results["raised"]
    picked = torch.gather(got["cost"], 0, got["level"].clamp(min=0).long()[None])[0]
    has = got["level"] >= 0
    assert torch.equal(picked[has], got["cost_min"][has]) and not (got["cost"][:, has] < got["cost_min"][has]).any()
    part = altitude_sweep(views, raised, grid, zone, S.SCENE_OFFSETS, layout="planes", rows=(10, 31))          # a band without a group
    assert torch.equal(part["level"][10:31], got["level"][10:31]) and (part["level"][:10] == -1).all() and (part["count"][31:] == 0).all()
    assert torch.isnan(part["altitude"][:10]).all() and torch.isnan(part["cost_min"][31:]).all()
    before = orthomosaic(views, raised, grid, zone, layout="planes")
    after = orthomosaic(views, got["altitude"], grid, zone, layout="planes")
    print(f"consistency of the raised DSM {before['consistency']:.6g} over {before['cells']} cells, of the sweep's altitude "
          f"{after['consistency']:.6g} over {after['cells']} cells")
    assert after["cells"] >= 1000 and after["consistency"] < before["consistency"]


def test_two_rank_sweep_matches_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_sweep_worker.py), each child under its own time limit and started once."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_sweep_worker.py")
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


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    """BN_EINVAL through the raw ABI, nothing launched, every buffer as it was."""
    from brdf_nerf_amd import _lib as L
    lib = L.lib()
    H, W, Hi, Wi, Cn, views, Z = 7, 9, 5, 6, 3, 2, 3
    site, zone = "z17", 17
    xoff, yoff = O.site_grid(site, H, W)
    dsm = dev(V.relief(H, W, low=K.SITES[site][3] - 20.0))
    img = dev(O.random_image(Cn, Hi, Wi))
    vis = torch.ones(H, W, dtype=torch.uint8, device=DEV)
    level = torch.full((H, W), -9, dtype=torch.int32, device=DEV)
    count = torch.full((H, W), 0xAB, dtype=torch.uint8, device=DEV)
    maps = [torch.full((H, W), -3.0, device=DEV) for _ in range(2)]
    cost = torch.full((Z, H, W), -3.0, device=DEV)
    valid, wins = (torch.full((Z,), -5, dtype=torch.int64, device=DEV) for _ in range(2))
    sums = torch.full((3,), -5, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    nan, inf = float("nan"), float("inf")

    def table(**kw):
        t = (L.MosaicView * views)()
        for k in range(views):
            t[k].img, t[k].vis, t[k].Hi, t[k].Wi = img.data_ptr(), vis.data_ptr() if k else None, Hi, Wi
            t[k].s_row, t[k].s_col, t[k].s_chan, t[k].rank = Wi, 1, Hi * Wi, k
            t[k].rpc = rpc_of(K.make_rpc(site, 2 + k)).struct
        for key, value in kw.items():
            if key == "rpc":
                getattr(t[1].rpc, value[0])[7] = value[1]
            else:
                setattr(t[1], key, value)
        return t

    good = table()
    good_dev = torch.frombuffer(bytearray(bytes(good)), dtype=torch.uint8).to(DEV)
    offs = lambda *v: (C.c_double * len(v))(*v)
    good_off = offs(-1.0, 0.0, 1.5)
    off_dev = torch.tensor([-1.0, 0.0, 1.5], dtype=torch.float64, device=DEV)

    def sweep(t=good, td=p(good_dev), views=views, Cn=Cn, s=p(dsm), H=H, W=W, xoff=xoff, yoff=yoff, res=0.5, row0=0, row1=H, zone=zone, south=0,
              mode=0, oh=good_off, od=p(off_dev), Z=Z, mv=2, cr=None, lv=p(level), cm=p(maps[0]), n=p(count), alt=p(maps[1]), cv=p(cost),
              v=p(valid), w=p(wins), q=p(sums)):
        return lib.bn_grid_sweep(t, td, views, Cn, s, H, W, xoff, yoff, res, row0, row1, zone, south, mode, oh, od, Z, mv, cr, lv, cm, n, alt, cv,
                                 v, w, q, None)

    flat = table()
    flat[1].rpc.col_scale = 0.0
    for kw in [dict(t=None), dict(td=None), dict(s=None), dict(views=0), dict(views=33), dict(views=-1),
               dict(Cn=0), dict(Cn=5), dict(Cn=-1), dict(zone=0), dict(zone=61), dict(zone=-1), dict(south=2), dict(south=-1), dict(H=0), dict(W=0),
               dict(H=-2), dict(H=1 << 15, W=(1 << 15) + 1), dict(row0=-1), dict(row1=H + 1), dict(row0=5, row1=4), dict(res=0.0),
               dict(res=-0.5), dict(res=inf), dict(res=nan), dict(xoff=nan), dict(yoff=inf), dict(mode=2), dict(mode=-1),
               dict(t=table(img=None)), dict(t=table(Hi=0)), dict(t=table(Wi=-3)), dict(t=table(s_row=-1)), dict(t=table(s_col=-1)),
               dict(t=table(s_chan=-1)), dict(t=flat), dict(t=table(rpc=("row_num", nan))), dict(t=table(rpc=("col_den", inf))),
               dict(oh=None), dict(od=None), dict(lv=None), dict(v=None), dict(w=None), dict(q=None), dict(Z=0), dict(Z=257), dict(Z=-1),
               dict(oh=offs(0.0, nan, 1.0)), dict(oh=offs(inf, 0.0, 1.0)), dict(oh=offs(0.0, 1.0, -inf)), dict(mv=0), dict(mv=33), dict(mv=-1)]:
        assert sweep(**kw) == -1, kw
        assert b"grid_sweep" in lib.bn_last_error()
    assert sweep(row0=3, row1=3) == 0                                          # accepted, nothing launched
    torch.cuda.synchronize()
    assert (level == -9).all() and (count == 0xAB).all() and all((m == -3.0).all() for m in maps) and (cost == -3.0).all()
    assert (valid == -5).all() and (wins == -5).all() and (sums == -5).all()
    for t in (valid, wins, sums):
        t.zero_()
    assert sweep(mv=1) == 0 and sweep(mv=1, cm=None, n=None, alt=None, cv=None) == 0          # accepted; the nullable outputs
    torch.cuda.synchronize()
    assert not (level == -9).any() and not (count == 0xAB).any() and not (cost == -3.0).any() and all(not (m == -3.0).any() for m in maps)
    assert int(sums[0]) == int(wins.sum()) == 2 * int((level >= 0).sum()) and int(valid.max()) <= 2 * H * W


def test_wrapper_refusals_on_the_device():
    from brdf_nerf_amd import Grid, altitude_sweep
    from brdf_nerf_amd import functions as Fn
    rpc = rpc_of(K.make_rpc("z17", 1))
    grid = Grid(0.0, 0.0, 0.5, 5, 4)
    dsm, img = torch.zeros(4, 5, device=DEV), torch.zeros(6 * 7, 3, device=DEV)
    view, off = (img, 6, 7, rpc), [0.0, 1.0]
    row = (img, 6, 7, (21, 3, 1), None, 0, rpc)
    for call in (lambda: altitude_sweep([view, (img.cpu(), 6, 7, rpc)], dsm, grid, 17, off), lambda: altitude_sweep([view], dsm.cpu(), grid, 17, off),
                 lambda: altitude_sweep([view], dsm, grid, 17, off, colrow=torch.zeros(2, 1, 4, 5, 2, dtype=torch.float64)),
                 lambda: Fn.grid_sweep([row[:4] + (torch.ones(4, 5, dtype=torch.uint8),) + row[5:]], 3, dsm, 0.0, 0.0, 0.5, 17, 0, off)):
        with pytest.raises(ValueError, match="device"):
            call()
    with pytest.raises(ValueError, match="no finite cell"):
        altitude_sweep([view], torch.full((4, 5), float("nan"), device=DEV), grid, 17, off)
    with pytest.raises(ValueError, match="strides"):
        Fn.grid_sweep([row[:3] + ((21, 3, 2),) + row[4:]], 3, dsm, 0.0, 0.0, 0.5, 17, 0, off)
    with pytest.raises(ValueError, match="level"):
        Fn.grid_sweep([row], 3, dsm, 0.0, 0.0, 0.5, 17, 0, off, level=torch.zeros(4, 4, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="cost"):
        Fn.grid_sweep([row], 3, dsm, 0.0, 0.0, 0.5, 17, 0, off, cost=torch.zeros(3, 4, 5, device=DEV))
    with pytest.raises(ValueError, match="offsets"):
        Fn.grid_sweep([row], 3, dsm, 0.0, 0.0, 0.5, 17, 0, [])
    with pytest.raises(ValueError, match="min_views"):
        Fn.grid_sweep([row], 3, dsm, 0.0, 0.0, 0.5, 17, 0, off, min_views=0)
