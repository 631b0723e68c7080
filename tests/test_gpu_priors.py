"""GPU tests of the tie-point depth priors (brdf_nerf_amd/camera.py depth_priors / tie_priors / ray_table(priors=),
bn_tie_owner / bn_tie_priors).  Run on the MI355X box with `pytest -m gpu`.

The ownership, the counters, the placement and the arithmetic from the ray onwards are integer rules and float32 / float64
+ - x / sqrt, all correctly rounded on the device: they are held BIT FOR BIT to the numpy statement of tests/priors_cases.py,
which is evaluated on the device's own tie_rays.  tie_rays in turn is bitwise view_rays(rows=, cols=) of the same pixels, and
test_gpu_camera.py holds that chain to its statement.  The goldens (upstream's load_depth_data) are checked through
depth_priors with the bounds test_priors_cpu.py derives."""
import os

import numpy as np
import pytest
import torch

import camera_cases as M
import priors_cases as P
from conftest import ROOT
from test_gpu_parity import DEV
from test_priors_cpu import bits, check_against_golden, golden_inputs

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
HYPER = dict(corrscale=0.9, stdscale=0.8, margin=1e-4, std_span=0.25)        # a std_span other than upstream's 0 shows step 5
SITE = {"z38": ("ecef", False), "z17": ("utm", False), "z21": ("utm", True)}
MAPS = ("valid", "depths", "depth_std", "rays")


def rpc_of(d, downscale=1.0):
    from brdf_nerf_amd.camera import Rpc
    return Rpc.from_dict(d, downscale)


def scene(site, seed, H, W, downscale=1.0):
    """-> a dictionary of the view's arguments: the image's rpc dictionary, its rescaled form, the frame about the centre pixel."""
    cs, south = SITE[site]
    zone = M.SITES[site][2]
    d = M.make_rpc(site, seed)
    lo, hi = M.alt_bounds(site)
    scaled = M.rescaled(d, downscale)
    mid = M.rays(scaled, np.array([W / 2 / downscale]), np.array([H / 2 / downscale]), lo, hi, cs, zone, south, (0.0, 0.0, 0.0), 1.0,
                 precision="exact")["world_near"][0]
    return dict(d=d, scaled=scaled, lo=lo, hi=hi, cs=cs, zone=zone, south=south, center=tuple(np.round(mid, 1).tolist()), rng=300.0,
                H=H, W=W, downscale=downscale)


def tie_data(sc, px, seed):
    """World points and correlations of the tie points (NaN-free for the pixels inside the view)."""
    inside = (px[:, 0] >= 0) & (px[:, 0] < sc["W"]) & (px[:, 1] >= 0) & (px[:, 1] < sc["H"])
    cols, rows = np.where(inside, px[:, 0], 0) / sc["downscale"], np.where(inside, px[:, 1], 0) / sc["downscale"]
    return P.world_points(sc["scaled"], cols, rows, sc["lo"], sc["hi"], sc["cs"], sc["zone"], sc["south"], seed)


def launch(sc, px, pts, cor, cmin, cmax, precision="reference", rpc=None, **kw):
    from brdf_nerf_amd.camera import tie_priors
    rpc = rpc or rpc_of(sc["d"], sc["downscale"])
    return tie_priors(rpc, sc["H"], sc["W"], px, pts, cor, cmin, cmax, sc["lo"], sc["hi"], sc["center"], sc["rng"], cs=sc["cs"],
                      zone=sc["zone"], south=sc["south"], downscale=sc["downscale"], precision=precision, want_rays=True,
                      want_tie_rays=True, device=DEV, **dict(HYPER, **kw))


def check_raw(raw, sc, px, pts, cor, cmin, cmax, precision, what, **kw):
    """Every output of the two launches against the statement on the device's own tie_rays.  -> the statement's result."""
    tie_rays = raw["tie_rays"].cpu().numpy()
    st = P.priors(px, pts, cor, tie_rays, sc["H"], sc["W"], sc["downscale"], sc["center"], sc["rng"], cmin, cmax, precision=precision,
                  **dict(HYPER, **kw))
    assert np.array_equal(raw["owner"].cpu().numpy(), st["owner"]), what
    counts = raw["counts"].tolist()
    assert counts == [st["outside"], st["duplicates"], st["skipped"], st["unsampled"]], (what, counts, st)
    assert raw["shape"] == st["shape"], what
    for k in MAPS:
        assert np.array_equal(bits(raw[k].cpu().numpy().reshape(st[k].shape)), bits(st[k])), (what, k)
    assert np.array_equal(bits(raw["points"].cpu().numpy()), bits(st["points"])), what
    assert np.array_equal(bits(raw["valid_full"].cpu().numpy()), bits(st["valid_full"])), what
    assert st["kept"] + sum(counts) == len(px), what
    return st


@pytest.mark.parametrize("H,W,downscale", [(33, 65, 1.0), (33, 65, 1.5), (33, 65, 2.0), (33, 65, 3.0), (2, 1000, 1.5), (9, 11, 1.0)])
def test_maps_owner_and_counters_bit_equal_to_the_statement(H, W, downscale):
    """T in {1, 63, 64, 65, 257}, both precisions, the three sites: ties in the four corners, outside on every side (negatives
    and the int32 extremes included), up to five on one pixel; tie_rays is view_rays of the same pixels."""
    from brdf_nerf_amd.camera import view_rays
    for k, T in enumerate(P.TIE_T):
        site = sorted(SITE)[k % 3]
        sc = scene(site, 20 + k, H, W, downscale)
        px = P.hard_ties(H, W, T, 300 + T)
        pts, cor = tie_data(sc, px, 40 + k)
        cmin, cmax = (float(cor.min()), float(cor.max())) if T > 1 else (0.0, 1.0)
        for precision in ("reference", "exact"):
            raw = launch(sc, px, pts, cor, cmin, cmax, precision)
            st = check_raw(raw, sc, px, pts, cor, cmin, cmax, precision, (H, W, downscale, T, site, precision))
            own = np.unique(st["owner"][st["owner"] >= 0]).astype(np.int64)
            rays, _ = view_rays(rpc_of(sc["d"], downscale), 0, 0, sc["lo"], sc["hi"], sc["center"], sc["rng"], cs=sc["cs"], zone=sc["zone"],
                                south=sc["south"], rows=px[own, 1] / downscale, cols=px[own, 0] / downscale, precision=precision, device=DEV)
            assert torch.equal(raw["tie_rays"][torch.from_numpy(own).to(DEV)].view(torch.int32), rays.view(torch.int32)), (T, precision)
            if T >= 63:
                assert st["outside"] > 0 and st["duplicates"] > 0 and st["kept"] > 0
            if T >= 63 and downscale > 1:
                assert st["unsampled"] > 0


def test_any_order_of_the_ties_gives_the_same_maps():
    """Sorted, reversed and shuffled: the highest index owns a pixel whatever the order of arrival, so with the repeats of a
    pixel carrying the same point every order gives identical maps and counters; the owner map is the statement's for each."""
    sc = scene("z17", 7, 33, 65, 1.5)
    px = P.hard_ties(33, 65, 257, 9)
    pts, cor = tie_data(sc, px, 3)
    first = {}
    for t, key in enumerate(map(tuple, px)):                   # the repeats of a pixel carry the data of its first tie point
        pts[t], cor[t] = pts[first.setdefault(key, t)], cor[first[key]]
    cmin, cmax = float(cor.min()), float(cor.max())
    srt = np.lexsort((px[:, 0], px[:, 1]))
    results = []
    for order in (srt, srt[::-1].copy(), np.random.default_rng(4).permutation(257)):
        raw = launch(sc, px[order], pts[order], cor[order], cmin, cmax)
        check_raw(raw, sc, px[order], pts[order], cor[order], cmin, cmax, "reference", "order")
        results.append(raw)
    for other in results[1:]:
        for k in MAPS + ("points", "valid_full"):
            assert torch.equal(other[k].view(torch.int32), results[0][k].view(torch.int32)), k
        assert other["counts"].tolist() == results[0]["counts"].tolist()
    assert results[0]["counts"][1] > 0


def test_highest_index_owns_a_pixel_with_five_ties():
    sc = scene("z38", 8, 9, 11)
    px = np.array([[4, 3]] * 5 + [[0, 0]], np.int64)
    pts, cor = tie_data(sc, px, 1)
    pts[:5, 2] += np.arange(5) * 3.0                           # five different points on one pixel
    raw = launch(sc, px, pts, cor, float(cor.min()), float(cor.max()))
    st = check_raw(raw, sc, px, pts, cor, float(cor.min()), float(cor.max()), "reference", "five")
    assert int(raw["owner"][3, 4]) == 4 and raw["counts"].tolist() == [0, 4, 0, 0] and st["kept"] == 2


def test_non_finite_ties_and_a_singular_rpc_are_skipped():
    """A NaN and an inf coordinate, a NaN correlation: counted as skipped, their pixels stay invalid, the others are untouched.
    An image whose Jacobian is singular skips every owner."""
    sc = scene("z21", 9, 33, 65)
    px = P.random_ties(33, 65, 65, 12)
    pts, cor = tie_data(sc, px, 2)
    cmin, cmax = float(cor.min()), float(cor.max())
    clean = launch(sc, px, pts, cor, cmin, cmax)
    pts[3, 0], pts[40, 1], cor[64] = np.nan, np.inf, np.nan
    raw = launch(sc, px, pts, cor, cmin, cmax)
    check_raw(raw, sc, px, pts, cor, cmin, cmax, "reference", "non-finite")
    assert raw["counts"].tolist() == [0, 0, 3, 0]
    valid = raw["valid"].cpu().numpy().reshape(33, 65)
    for t in (3, 40, 64):
        assert valid[px[t, 1], px[t, 0]] == 0 and float(raw["valid_full"][px[t, 1], px[t, 0]]) == 0
    assert valid.sum() == 62 and clean["valid"].sum().item() == 65
    keep = torch.from_numpy(valid.ravel() > 0).to(DEV)
    assert torch.equal(raw["depths"][keep], clean["depths"][keep])
    sing = launch(sc, px, *tie_data(sc, px, 2), cmin, cmax, rpc=rpc_of(M.singular_rpc()))
    assert sing["counts"].tolist() == [0, 0, 65, 0] and not sing["valid"].any() and not sing["valid_full"].any()
    assert torch.isnan(sing["tie_rays"]).all()


@pytest.mark.parametrize("downscale", P.DOWNSCALES)
def test_depth_priors_is_the_statement_with_padding_and_normals(downscale):
    """The public call on 33 x 65: counters, kept + outside + duplicates + skipped + unsampled == T, the padding (float32 of
    the float64 mean; the two float64 sums may differ in order, so the pad may differ in its last float32 bit) and the normals
    (bn_point_normals on the full-resolution grid, bit for bit its statement as in test_gpu_maps.py, then the sampled lines)."""
    from brdf_nerf_amd.camera import depth_priors, tie_priors
    sc = scene("z17", 11, 33, 65, downscale)
    px = P.hard_ties(33, 65, 257, 21)
    pts, cor = tie_data(sc, px, 5)
    kw = dict(cs=sc["cs"], zone=sc["zone"], south=sc["south"], downscale=downscale, device=DEV, **HYPER)
    res = depth_priors(rpc_of(sc["d"], downscale), 33, 65, px, pts, cor, sc["lo"], sc["hi"], sc["center"], sc["rng"], want_rays=True, **kw)
    raw = launch(sc, px, pts, cor, float(cor.min()), float(cor.max()))
    st = check_raw(raw, sc, px, pts, cor, float(cor.min()), float(cor.max()), "reference", downscale)
    for k in ("outside", "duplicates", "skipped", "unsampled", "kept", "shape"):
        assert res[k] == st[k], k
    assert res["kept"] + res["outside"] + res["duplicates"] + res["skipped"] + res["unsampled"] == 257
    assert torch.equal(res["valid_depth"], raw["valid"]) and torch.equal(res["depth_std"], raw["depth_std"])
    assert torch.equal(res["rays"], raw["rays"]) and torch.equal(res["depths"][:, 1], raw["depths"][:, 1])
    want, got = P.padded(st), res["depths"].cpu().numpy()
    keep = st["valid"] > 0
    assert np.array_equal(bits(got[keep]), bits(want[keep]))
    assert (np.abs(got[~keep, 0].astype(np.float64) - want[~keep, 0]) <= np.spacing(want[~keep, 0])).all()
    nrm, vn = P.normals(st, 33, 65, downscale)
    assert np.array_equal(bits(res["valid_normal"].cpu().numpy()), bits(vn))
    gn = res["normals"].cpu().numpy()
    assert np.array_equal(gn[vn == 0], np.tile(np.float32([0, 0, 1]), (int((vn == 0).sum()), 1)))
    assert np.array_equal(bits(gn), bits(nrm))
    lean = depth_priors(rpc_of(sc["d"], downscale), 33, 65, px, pts, cor, sc["lo"], sc["hi"], sc["center"], sc["rng"], want_normals=False,
                        **kw)
    assert "normals" not in lean and "rays" not in lean and torch.equal(lean["depths"], res["depths"])


@pytest.mark.parametrize("name", sorted(P.GOLDENS))
def test_goldens_through_depth_priors(name):
    """Upstream's load_depth_data on the fixture's files, with the bounds of test_priors_cpu.py."""
    from brdf_nerf_amd.camera import depth_priors
    g, v, px, pts3d, correl, (cs, zone, south), hyper = golden_inputs(name)
    res = depth_priors(rpc_of(v["rpc"]), v["H"], v["W"], px, pts3d, correl, v["min_alt"], v["max_alt"], g["center"].tolist(),
                       float(g["range"]), cs=cs, zone=zone, south=south, want_rays=True, device=DEV, **hyper)
    got = {k: res[k].cpu().numpy() for k in ("valid_depth", "depth_std", "depths", "normals", "valid_normal", "rays")}
    diff = bits(got["rays"]) != bits(g["rays"])
    print(f"{name}: {int(diff.sum())} of {diff.size} ray elements differ from the reference (columns {np.flatnonzero(diff.any(0)).tolist()}), "
          f"{int((bits(got['depths'][:, 1]) != bits(g['depths'][:, 1])).sum())} weights")
    assert (res["outside"], res["duplicates"], res["skipped"], res["unsampled"], res["kept"]) == (0, 0, 0, 0, len(px))
    assert not diff.any(), name
    check_against_golden(g, got, len(px), name)


def test_ray_table_with_priors_trains():
    """Two views, the second without priors: the columns are the per-view results, the rays those of the table without priors,
    and one depth-supervised step on 64 rows of it gives a finite loss."""
    from brdf_nerf_amd.camera import depth_priors, ray_table
    from brdf_nerf_amd.trainer import FusedTrainer
    from test_gpu_parity import build_model, make_args, mini
    sc = scene("z17", 12, 12, 10)
    H, W = 12, 10
    view = {"rpc": sc["d"], "H": H, "W": W, "min_alt": sc["lo"], "max_alt": sc["hi"], "sun": M.SUN}
    px = P.random_ties(H, W, 90, 3)
    pts, cor = tie_data(sc, px, 6)
    images = [torch.rand(H * W, 3), torch.rand(H * W, 3)]
    pri = {"pts2d": px, "pts3d": pts, "correl": cor}
    table = ray_table([view, view], images, sc["center"], sc["rng"], zone=17, device=DEV, priors=[pri, None])
    plain = ray_table([view, view], images, sc["center"], sc["rng"], zone=17, device=DEV)
    assert "depths" not in plain.data and torch.equal(table.data["rays"].view(torch.int32), plain.data["rays"].view(torch.int32))
    one = depth_priors(rpc_of(sc["d"]), H, W, px, pts, cor, sc["lo"], sc["hi"], sc["center"], sc["rng"], zone=17, margin=1e-4, device=DEV,
                       want_normals=False)
    n = H * W
    for k in ("depths", "valid_depth", "depth_std"):
        assert table.data[k].shape[0] == 2 * n and torch.equal(table.data[k][:n], one[k]) and not table.data[k][n:].any(), k
    assert one["kept"] == 90 and table.data["valid_depth"].sum().item() == 90
    cfg = mini()
    tr = FusedTrainer(build_model(cfg, 3), make_args(cfg), lr=5e-4, ds_lambda=10.0)
    torch.manual_seed(1)
    b = table.next_batch(64)
    assert b["valid_depth"].sum().item() > 0
    loss, _ = tr.step(b["rays"], b["rgbs"], valid_depth=b["valid_depth"], depths=b["depths"], depth_std=b["depth_std"])
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))


def test_every_refusal_is_a_value_error_on_the_device():
    from brdf_nerf_amd.camera import depth_priors
    sc = scene("z38", 3, 9, 11)
    px = P.random_ties(9, 11, 8, 1)
    pts, cor = tie_data(sc, px, 1)
    nan, inf = float("nan"), float("inf")

    def call(pts2d=px, pts3d=pts, correl=cor, H=9, W=11, lo=sc["lo"], hi=sc["hi"], center=sc["center"], rng=sc["rng"], **kw):
        return depth_priors(rpc_of(sc["d"]), H, W, pts2d, pts3d, correl, lo, hi, center, rng, device=DEV,
                            **dict(dict(cs="ecef"), **kw))

    assert call()["kept"] == 8
    for kw in (dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15), dict(pts2d=np.zeros((0, 2), np.int64), pts3d=np.zeros((0, 3)), correl=np.zeros(0)),
               dict(downscale=nan), dict(downscale=inf), dict(downscale=0.5), dict(rng=0.0), dict(rng=nan), dict(rng=inf),
               dict(correl=np.full(8, 0.5)), dict(correl=np.where(np.arange(8) == 2, nan, cor)), dict(correl=np.where(np.arange(8) == 2, inf, cor)),
               dict(corrscale=nan), dict(stdscale=inf), dict(margin=nan), dict(std_span=inf), dict(cs="wgs"), dict(cs="utm", zone=0),
               dict(cs="utm", zone=61), dict(lo=nan), dict(hi=inf), dict(center=(0.0, nan, 0.0)), dict(precision="fast"),
               dict(pts2d=px.astype(np.float64)), dict(pts3d=pts[:7]), dict(correl=cor[:7])):
        with pytest.raises(ValueError):
            call(**kw)
