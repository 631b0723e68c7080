"""GPU tests of the orthomosaic of several observed images (brdf_nerf_amd/mosaic.py; bn_grid_mosaic).  Run on the MI355X box with
`pytest -m gpu`.  Cases and the numpy float64 statement they are held to: tests/mosaic_cases.py.

Fed the STATEMENT's pixels (colrow_in), no transcendental lies between the kernel's inputs and its outputs, and every output must
equal the statement bit for bit.  With the projection inside, the kernel is held to the statement's fuse applied to the DEVICE's
own per-view bn_grid_pixels + bn_image_gather outputs: the fused launch is the K-launch chain's bits.
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
import visibility_cases as V
from test_gpu_parity import DEV, _free_port

pytestmark = pytest.mark.gpu

LAYOUTS = ("image", "planes")
MODES = ("bilinear", "nearest")
MAPS = ("best_val", "mean", "std")


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).copy()).to(DEV)


def npy(t):
    return t.detach().cpu().numpy()


def rpc_of(d):
    from brdf_nerf_amd import Rpc
    return Rpc.from_dict(d)


def strides_of(Cn, Hi, Wi, layout):
    return (Wi * Cn, Cn, 1) if layout == "image" else (Wi, 1, Hi * Wi)


def view_table(planes, ds, vis, rank, layout):
    """The K tuples functions.grid_mosaic takes: planes K arrays (C, Hi, Wi), ds K descriptors, vis K arrays (H, W) or None."""
    return [(dev(O.to_layout(p, layout)), p.shape[1], p.shape[2], strides_of(*p.shape, layout), None if v is None else dev(v), int(r),
             rpc_of(d)) for p, d, v, r in zip(planes, ds, vis, rank)]


def check(out, want, mode, where, shape=None):
    """Every output of the launch against fuse's dictionary: integers equal, best_val on all 32 bits in nearest mode, mean, std and
    the bilinear best_val bit-equal with every NaN as one value."""
    n = want["count"].size
    assert np.array_equal(npy(out["count"]).reshape(-1), want["count"].reshape(-1)), where
    assert np.array_equal(npy(out["best"]).reshape(-1), want["best"].reshape(-1)), where
    assert npy(out["counts"]).tolist() == want["counts"].tolist(), where
    assert npy(out["sums"]).tolist() == list(want["sums"]), where
    for key in MAPS:
        got = npy(out[key]).reshape(-1, n)
        assert O.same_f32(got, want[key].reshape(-1, n), exact_nan=key == "best_val" and mode == "nearest"), f"{where} {key}"


def statement_case(H, W, views, Cn, seed=0):
    """Views of different image sizes over an H x W grid, their pixels from random_colrow and edge_colrow, images with NaN,
    payload-NaN, -0.0, denormal and infinite pixels, a mask for every second view, ranks with ties."""
    n = H * W
    rng = np.random.default_rng(seed + 7 * views + Cn + n)
    planes, colrow, vis = [], [], []
    for k in range(views):
        Hi, Wi = M.IMAGE_SIZES[(k + seed) % len(M.IMAGE_SIZES)]
        planes.append(O.random_image(Cn, Hi, Wi, seed=k + seed))
        cr = O.random_colrow(Hi, Wi, n, seed=k + seed)
        edge = O.edge_colrow(Hi, Wi)
        at = rng.permutation(n)[:min(n, len(edge))]
        cr[at] = edge[rng.permutation(len(edge))[:len(at)]]
        colrow.append(cr.reshape(H, W, 2))
        vis.append(rng.integers(0, 3, (H, W)).astype(np.uint8) if k % 2 else None)
    rank = rng.integers(0, max(2, views // 2), views).tolist()
    ds = [K.make_rpc("z17", k) for k in range(views)]
    return planes, np.stack(colrow), vis, rank, ds


def fuse_of_the_statement(planes, colrow, vis, rank, mode):
    per_view = [O.gather(p, cr, v, mode) for p, cr, v in zip(planes, colrow, vis)]
    return M.fuse(np.stack([p[0] for p in per_view]), np.stack([p[1] for p in per_view]), rank)


# ------------------------------------------------------------------------------------------------ statement pixels in
@pytest.mark.parametrize("views,Cn", ((1, 1), (2, 3), (3, 4), (5, 3), (32, 1), (32, 4)))
@pytest.mark.parametrize("shape", M.GRIDS)
def test_mosaic_bit_equal_to_the_statement(shape, views, Cn):
    from brdf_nerf_amd import functions as Fn
    H, W = shape
    planes, colrow, vis, rank, ds = statement_case(H, W, views, Cn)
    dsm = torch.zeros(H, W, device=DEV)
    seen = set()
    for mode in MODES:
        want = fuse_of_the_statement(planes, colrow, vis, rank, mode)
        seen |= set(np.unique(want["states"]).tolist())
        for layout in LAYOUTS:
            out = Fn.grid_mosaic(view_table(planes, ds, vis, rank, layout), Cn, dsm, 0.0, 0.0, 0.5, 17, 0, mode=mode, colrow=dev(colrow))
            check(out, want, mode, f"{H} x {W} K={views} C={Cn} {mode} {layout}")
    if H * W >= 255 and views >= 5:
        assert seen == {0, 1, 2, 3, 4}                                       # every state occurs, NONFINITE included


def test_planted_stack_keeps_its_spread():
    """Five constant images 4096 + {0.001, 0.002, 0.0005, 0.0017, 0.0011}: the std is the two-pass value as float32, which the
    sum-of-squares form misses (asserted on the inputs), in every channel and both modes."""
    from brdf_nerf_amd import functions as Fn
    H, W, Cn = 3, 5, 3
    planes = [M.planted_image(Cn, 5, 7, k) for k in range(5)]
    colrow = np.stack([O.random_colrow(5, 7, H * W, seed=k).reshape(H, W, 2) for k in range(5)])
    colrow[:, 1, 2] = (2.25, 3.5)                                            # one cell that all five views see
    values = M.planted_values(Cn)[:, :, 0]
    two_pass = values.astype(np.float64).std(0).astype(np.float32)
    assert all(np.float32(M.sum_of_squares_std(values[:, ch])) != two_pass[ch] for ch in range(Cn))
    ds = [K.make_rpc("z17", k) for k in range(5)]
    for mode in MODES:
        want = fuse_of_the_statement(planes, colrow, [None] * 5, range(5), mode)
        out = Fn.grid_mosaic(view_table(planes, ds, [None] * 5, range(5), "planes"), Cn, torch.zeros(H, W, device=DEV), 0.0, 0.0, 0.5, 17, 0,
                             mode=mode, colrow=dev(colrow))
        check(out, want, mode, f"planted {mode}")
        assert npy(out["count"])[1, 2] == 5 and np.array_equal(npy(out["std"])[:, 1, 2], two_pass)


# ------------------------------------------------------------------------------------------------ projection inside
def site_relief(site, H, W, seed=0):
    return V.relief(H, W, seed=seed, nan=0.1, low=K.SITES[site][3] - 20.0)


@pytest.mark.parametrize("site", sorted(K.SITES))
@pytest.mark.parametrize("shape", ((3, 5), (33, 65)))
def test_fused_launch_is_the_chain_of_launches(shape, site):
    """colrow_in NULL: every output equals fuse applied to the device's own bn_grid_pixels + bn_image_gather outputs per view;
    counts[k][0..2] are that gather's, counts[k][3] + counts[k][4] its kept count."""
    from brdf_nerf_amd import functions as Fn
    H, W = shape
    zone, res, Cn = K.SITES[site][2], 0.5, 3
    dsm = site_relief(site, H, W, seed=H + W)
    assert np.isnan(dsm).any() and np.isinf(dsm).any()
    xoff, yoff = O.site_grid(site, H, W, res, shift=(137.0, -61.0))
    ds = [K.make_rpc(site, 30 + k) for k in range(3)]
    planes = [O.random_image(Cn, Hi, Wi, seed=k) for k, (Hi, Wi) in enumerate(((640, 640), (600, 550), (528, 720)))]          # some cells outside the two smaller ones
    vis = [None, np.random.default_rng(H).integers(0, 3, (H, W)).astype(np.uint8), None]
    rank = [1, 0, 1]
    ddsm = dev(dsm)
    for mode in MODES:
        table = view_table(planes, ds, vis, rank, "image")
        values, states, gathered = [], [], []
        for img, Hi, Wi, strides, v, _, rpc in table:
            colrow, _ = Fn.grid_pixels(rpc, ddsm, xoff, yoff, res, zone, 0)
            out, state, counts = Fn.image_gather(img, Hi, Wi, Cn, strides, colrow, v, mode=mode)
            values.append(npy(out))
            states.append(npy(state))
            gathered.append(npy(counts).tolist())
        want = M.fuse(np.stack(values), np.stack(states), rank)
        out = Fn.grid_mosaic(table, Cn, ddsm, xoff, yoff, res, zone, 0, mode=mode)
        check(out, want, mode, f"{site} {H} x {W} {mode}")
        got = npy(out["counts"]).tolist()
        for k in range(3):
            assert got[k][:3] == gathered[k][:3] and got[k][3] + got[k][4] == gathered[k][3]
        print(f"{site} {H} x {W} {mode}: counts {got}")
        assert sum(row[3] for row in got) > 0                                # the views do see the grid
        if H * W > 15:
            assert all(sum(row[s] for row in got) > 0 for s in range(5))      # and every state occurs


# ------------------------------------------------------------------------------------------------ row bands
def test_row_bands_into_one_set_of_buffers():
    from brdf_nerf_amd import functions as Fn
    H, W, views, Cn = 33, 65, 3, 3
    planes, colrow, vis, rank, ds = statement_case(H, W, views, Cn, seed=3)
    dsm = torch.zeros(H, W, device=DEV)
    table = view_table(planes, ds, vis, rank, "image")
    whole = Fn.grid_mosaic(table, Cn, dsm, 0.0, 0.0, 0.5, 17, 0, colrow=dev(colrow))
    check(whole, fuse_of_the_statement(planes, colrow, vis, rank, "bilinear"), "bilinear", "whole")
    bufs = dict(count=torch.full((H, W), 0xAB, dtype=torch.uint8, device=DEV), best=torch.full((H, W), -9, dtype=torch.int32, device=DEV),
                **{k: torch.full((Cn, H, W), -3.0, device=DEV) for k in MAPS},
                counts=torch.zeros((views, 5), dtype=torch.int64, device=DEV), sums=torch.zeros(3, dtype=torch.int64, device=DEV))
    untouched = lambda rows: (bufs["count"][rows] == 0xAB).all() and (bufs["best"][rows] == -9).all() and \
        all((bufs[k][:, rows] == -3.0).all() for k in MAPS)
    Fn.grid_mosaic(table, Cn, dsm, 0.0, 0.0, 0.5, 17, 0, colrow=dev(colrow), rows=(5, 5), **bufs)          # an empty band writes nothing
    assert untouched(slice(0, H)) and int(bufs["counts"].sum()) == 0 and int(bufs["sums"].sum()) == 0
    cuts = list(M.ROW_SPLITS) + [H]
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        assert untouched(slice(r0, H))
        Fn.grid_mosaic(table, Cn, dsm, 0.0, 0.0, 0.5, 17, 0, colrow=dev(colrow), rows=(r0, r1), **bufs)
        assert untouched(slice(r1, H))
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    for key in ("count", "best", "counts", "sums") + MAPS:
        assert torch.equal(bits(bufs[key]), bits(whole[key])), key


# ------------------------------------------------------------------------------------------------ the wrapper
def box_scene_on_the_device(ds, planes, layout="image"):
    from brdf_nerf_amd import Grid
    _, dsm, xoff, yoff, res, zone = M.box_views()
    H, W = dsm.shape
    views = [(dev(O.to_layout(p, layout)), p.shape[1], p.shape[2], rpc_of(d)) for p, d in zip(planes, ds)]
    return views, dsm, Grid(xoff, yoff, res, W, H), zone


def test_one_view_is_the_orthophoto():
    from brdf_nerf_amd import orthomosaic, orthophoto
    ds = M.box_views()[0][:1]
    planes = [O.random_image(3, *O.SCENE_IMAGE, seed=4, specials=False)]
    views, dsm, grid, zone = box_scene_on_the_device(ds, planes)
    for mode in MODES:
        one = orthophoto(*views[0], dev(dsm), grid, zone, mode=mode)
        got = orthomosaic(views, dev(dsm), grid, zone, mode=mode)
        kept = one["state"] == O.KEPT
        assert 200 <= int(kept.sum()) < dsm.size
        assert torch.equal(got["best_rgb"].view(torch.int32), one["ortho"].view(torch.int32))
        assert torch.equal(got["mean"][:, kept], one["ortho"][:, kept]) and torch.isnan(got["mean"][:, ~kept]).all()
        assert (got["std"][:, kept] == 0).all() and torch.isnan(got["std"][:, ~kept]).all()
        assert torch.equal(got["count"], kept.to(torch.uint8)) and torch.equal(got["best"], kept.to(torch.int32) - 1)
        assert torch.equal(got["visible"][0], one["visible"]) and got["rank"] == [0] and got["cells"] == 0 and np.isnan(got["consistency"])
        assert got["counts"] == {"nodata": [one["counts"]["nodata"]], "outside": [one["counts"]["outside"]],
                                 "occluded": [one["counts"]["occluded"]], "used": [one["counts"]["kept"]], "nonfinite": [0]}


@pytest.mark.parametrize("image", ("linear", "random"))
def test_orthomosaic_of_the_box_scene(image):
    """Three views of the box scene: orthomosaic equals fuse applied to three device orthophoto results, whose per-cell values and
    states orthophoto's own tests hold; the histogram of n is the statement's; the ranks order the views by elevation; an explicit
    permuted rank moves `best` only; consistency is the integer quotient."""
    from brdf_nerf_amd import orthomosaic, orthophoto, ortho_psnr
    ds = M.box_views()[0]
    Hi, Wi = O.SCENE_IMAGE
    planes = [O.linear_image(Hi, Wi, 3) + np.float32(k) if image == "linear" else O.random_image(3, Hi, Wi, seed=k) for k in range(3)]
    views, dsm, grid, zone = box_scene_on_the_device(ds, planes)
    H, W = dsm.shape
    ddsm = dev(dsm)
    got = orthomosaic(views, ddsm, grid, zone)
    singles = [orthophoto(*v, ddsm, grid, zone) for v in views]
    dirs = np.stack([npy(s["view_dir"]) for s in singles])
    assert np.array_equal(npy(got["view_dirs"]), dirs) and got["rank"] == M.nadir_ranks(dirs) and sorted(got["rank"]) == [0, 1, 2]
    want = M.fuse(np.stack([npy(s["ortho"]).reshape(3, -1) for s in singles]), np.stack([npy(s["state"]).reshape(-1) for s in singles]),
                  got["rank"])
    out = dict(count=got["count"], best=got["best"], best_val=got["best_rgb"], mean=got["mean"], std=got["std"],
               counts=torch.tensor([[got["counts"][s][k] for s in M.STATES] for k in range(3)]),
               sums=torch.tensor([got["cells"], want["sums"][1], got["skipped"]]))
    check(out, want, "bilinear", f"box scene {image}")
    for k in range(3):
        assert torch.equal(got["visible"][k], singles[k]["visible"])
    statement = M.mosaic(ds, planes, dsm, grid.xoff, grid.yoff, grid.resolution, zone)
    hist = np.bincount(npy(got["count"]).ravel(), minlength=4).tolist()
    assert hist == np.bincount(statement["count"].ravel(), minlength=4).tolist() and min(hist) >= 10
    assert got["rank"] == statement["rank"]
    assert got["consistency"] == want["sums"][1] / (want["sums"][0] * 3 * (1 << 20)) and got["cells"] == hist[2] + hist[3]
    assert (got["counts"]["nonfinite"] == [0, 0, 0]) == (image == "linear")
    other = orthomosaic(views, ddsm, grid, zone, rank=[got["rank"][1], got["rank"][2], got["rank"][0]])
    assert not torch.equal(other["best"], got["best"]) and not torch.equal(other["best_rgb"].view(torch.int32), got["best_rgb"].view(torch.int32))
    for key in ("mean", "std"):
        assert torch.equal(other[key].view(torch.int32), got[key].view(torch.int32)), key
    assert torch.equal(other["count"], got["count"]) and other["counts"] == got["counts"] and other["consistency"] == got["consistency"]
    # a band without a group: the other rows are unseen and uncounted; the pixels given instead of the projection: the same bits
    part = orthomosaic(views, ddsm, grid, zone, rows=(10, 31))
    assert torch.equal(part["mean"][:, 10:31].view(torch.int32), got["mean"][:, 10:31].view(torch.int32))
    assert (part["count"][:10] == 0).all() and (part["best"][31:] == -1).all() and torch.isnan(part["std"][:, :10]).all()
    assert sum(part["counts"][s][0] for s in M.STATES) == 21 * W
    given = orthomosaic(views, ddsm, grid, zone, colrow=torch.stack([s["colrow"] for s in singles]))
    for key in ("best_rgb", "mean", "std"):
        assert torch.equal(given[key].view(torch.int32), got[key].view(torch.int32)), key
    psnr, n = ortho_psnr(got["mean"], got["mean"])
    assert n == int((npy(got["count"]) > 0).sum()) and n > 0


def test_a_wrong_altitude_raises_the_consistency():
    """Three cameras that all see ONE texture painted on the box scene: on the true DSM the views agree but for the box's
    silhouette; with the box 6 m too high every roof cell lands on different ground in every image.  The direction only."""
    from brdf_nerf_amd import Grid, orthomosaic
    ds, dsm, xoff, yoff, res, zone = M.fine_views()
    planes = M.textured_images(ds, dsm, xoff, yoff, res, zone)
    H, W = dsm.shape
    views = [(dev(p), p.shape[1], p.shape[2], rpc_of(d)) for p, d in zip(planes, ds)]
    grid = Grid(xoff, yoff, res, W, H)
    true = orthomosaic(views, dev(dsm), grid, zone, layout="planes")
    wrong = orthomosaic(views, dev(M.raised(dsm)), grid, zone, layout="planes")
    print(f"consistency of the true DSM {true['consistency']:.6g} over {true['cells']} cells, of the box 6 m too high "
          f"{wrong['consistency']:.6g} over {wrong['cells']} cells")
    assert true["cells"] >= 1000 and wrong["cells"] >= 1000 and true["skipped"] == wrong["skipped"] == 0
    assert wrong["consistency"] > true["consistency"]


def test_two_rank_orthomosaic_matches_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_mosaic_worker.py), each child under its own time limit and started once."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_mosaic_worker.py")
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
    H, W, Hi, Wi, Cn, views = 7, 9, 5, 6, 3, 2
    site, zone = "z17", 17
    xoff, yoff = O.site_grid(site, H, W)
    dsm = dev(V.relief(H, W, low=K.SITES[site][3] - 20.0))
    img = dev(O.random_image(Cn, Hi, Wi))
    vis = torch.ones(H, W, dtype=torch.uint8, device=DEV)
    count = torch.full((H, W), 0xAB, dtype=torch.uint8, device=DEV)
    best = torch.full((H, W), -9, dtype=torch.int32, device=DEV)
    maps = [torch.full((Cn, H, W), -3.0, device=DEV) for _ in range(3)]
    counts = torch.full((views, 5), -5, dtype=torch.int64, device=DEV)
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
            field, _, index = key.partition("__")
            if field == "rpc":
                index, value = value
                getattr(t[1].rpc, index)[7] = value
            else:
                setattr(t[1], field, value)
        return t

    good = table()
    on_device = lambda t: torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(DEV)
    good_dev = on_device(good)

    def mosaic(t=good, td=p(good_dev), views=views, Cn=Cn, s=p(dsm), H=H, W=W, xoff=xoff, yoff=yoff, res=0.5, row0=0, row1=H, zone=zone, south=0,
               mode=0, cr=None, n=p(count), b=p(best), c=p(counts), q=p(sums)):
        return lib.bn_grid_mosaic(t, td, views, Cn, s, H, W, xoff, yoff, res, row0, row1, zone, south, mode, cr, n, b, p(maps[0]), p(maps[1]),
                                  p(maps[2]), c, q, None)

    flat = table()
    flat[1].rpc.col_scale = 0.0
    for kw in [dict(t=None), dict(td=None), dict(s=None), dict(n=None), dict(c=None), dict(views=0), dict(views=33), dict(views=-1),
               dict(Cn=0), dict(Cn=5), dict(Cn=-1), dict(zone=0), dict(zone=61), dict(zone=-1), dict(south=2), dict(south=-1), dict(H=0), dict(W=0),
               dict(H=-2), dict(H=1 << 15, W=(1 << 15) + 1), dict(row0=-1), dict(row1=H + 1), dict(row0=5, row1=4), dict(res=0.0),
               dict(res=-0.5), dict(res=inf), dict(res=nan), dict(xoff=nan), dict(yoff=inf), dict(mode=2), dict(mode=-1),
               dict(t=table(img=None)), dict(t=table(Hi=0)), dict(t=table(Wi=-3)), dict(t=table(s_row=-1)), dict(t=table(s_col=-1)),
               dict(t=table(s_chan=-1)), dict(t=flat), dict(t=table(rpc=("row_num", nan))), dict(t=table(rpc=("col_den", inf)))]:
        assert mosaic(**kw) == -1, kw
        assert b"grid_mosaic" in lib.bn_last_error()
    assert mosaic(row0=3, row1=3) == 0                                         # accepted, nothing launched
    torch.cuda.synchronize()
    assert (count == 0xAB).all() and (best == -9).all() and all((m == -3.0).all() for m in maps) and (counts == -5).all() and (sums == -5).all()
    counts.zero_()
    sums.zero_()
    assert mosaic() == 0 and mosaic(b=None, q=None) == 0                       # the same arguments, accepted; nullable outputs
    torch.cuda.synchronize()
    assert not (count == 0xAB).any() and not (best == -9).any() and int(counts.sum()) == 2 * views * H * W
    assert all(not (m == -3.0).any() for m in maps)


def test_wrapper_refusals_on_the_device():
    from brdf_nerf_amd import Grid, orthomosaic
    from brdf_nerf_amd import functions as Fn
    rpc = rpc_of(K.make_rpc("z17", 1))
    grid = Grid(0.0, 0.0, 0.5, 5, 4)
    dsm, img = torch.zeros(4, 5, device=DEV), torch.zeros(6 * 7, 3, device=DEV)
    view = (img, 6, 7, rpc)
    for call in (lambda: orthomosaic([view, (img.cpu(), 6, 7, rpc)], dsm, grid, 17), lambda: orthomosaic([view], dsm.cpu(), grid, 17),
                 lambda: orthomosaic([view], dsm, grid, 17, colrow=torch.zeros(1, 4, 5, 2, dtype=torch.float64)),
                 lambda: Fn.grid_mosaic([(img, 6, 7, (21, 3, 1), torch.ones(4, 5, dtype=torch.uint8), 0, rpc)], 3, dsm, 0.0, 0.0, 0.5, 17, 0)):
        with pytest.raises(ValueError, match="device"):
            call()
    with pytest.raises(ValueError, match="no finite cell"):
        orthomosaic([view], torch.full((4, 5), float("nan"), device=DEV), grid, 17)
    with pytest.raises(ValueError, match="strides"):
        Fn.grid_mosaic([(img, 6, 7, (21, 3, 2), None, 0, rpc)], 3, dsm, 0.0, 0.0, 0.5, 17, 0)
    with pytest.raises(ValueError, match="count"):
        Fn.grid_mosaic([(img, 6, 7, (21, 3, 1), None, 0, rpc)], 3, dsm, 0.0, 0.0, 0.5, 17, 0, count=torch.zeros(4, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="rank"):
        Fn.grid_mosaic([(img, 6, 7, (21, 3, 1), None, 0.5, rpc)], 3, dsm, 0.0, 0.0, 0.5, 17, 0)
    with pytest.raises(ValueError, match="channels"):
        Fn.grid_mosaic([(img, 6, 7, (21, 3, 1), None, 0, rpc)], 5, dsm, 0.0, 0.0, 0.5, 17, 0)
