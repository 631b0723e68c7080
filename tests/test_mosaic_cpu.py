"""Host tests of the orthomosaic rule (no device): the numpy statement of tests/mosaic_cases.py against the two-pass float64 mean
and std, Welford against the sum-of-squares form on the planted stack, the edge cells, a condition on the end-to-end inputs, the
build, and the wrapper refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import camera_cases as K
import mosaic_cases as M
import orthophoto_cases as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("views", (1, 2, 5, 32))
def test_fuse_against_the_two_pass_mean_and_std(views):
    """Welford's error is of order K 2^-53 of the largest |value|; K 2^-50 leaves a margin of 8 for the per-step roundings.  Held on
    the float64 m and sqrt(M2 / n) before the cast; the float32 outputs are their casts."""
    C, n = 3, 400
    values, states = M.random_stack(views, C, n, seed=1, specials=False)
    got = M.fuse(values, states, list(range(views)))
    used = got["states"] == M.USED
    mean, std = M.two_pass(values, used)
    seen = got["count"] > 0
    assert np.array_equal(got["count"], used.sum(0)) and seen.sum() >= 200 and (got["count"] >= min(views, 2)).any()
    bound = views * 2.0 ** -50 * float(np.abs(values).max())
    dm = np.abs(got["mean64"][:, seen] - mean[:, seen]).max()
    ds = np.abs(got["std64"][:, seen] - std[:, seen]).max()
    print(f"K={views}: Welford within {dm:.3g} (mean) and {ds:.3g} (std) of np.mean / np.std in float64 (bound {bound:.3g})")
    assert dm <= bound and ds <= bound
    assert O.same_f32(got["mean"], got["mean64"].astype(np.float32)) and O.same_f32(got["std"], got["std64"].astype(np.float32))
    assert np.isnan(got["mean"][:, ~seen]).all() and np.isnan(got["std"][:, ~seen]).all() and (got["best"][~seen] == -1).all()


def test_welford_keeps_the_spread_that_sum_of_squares_loses():
    values = M.planted_values()
    got = M.fuse(values, np.full((5, 1), O.KEPT), range(5))
    x = values[:, 0, 0].astype(np.float64)
    two_pass = np.float32(x.std())
    naive = np.float32(M.sum_of_squares_std(values[:, 0, 0]))
    print(f"planted stack: Welford {got['std'][0, 0]:.6g}, two-pass {two_pass:.6g}, sum of squares {naive:.6g}")
    assert got["std"][0, 0] == two_pass
    assert naive != two_pass
    assert got["mean"][0, 0] == np.float32(x.mean()) and got["count"][0] == 5


def test_edge_cells():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    #                    cell 0: unseen   1: one view    2: tie of ranks   3: NaN and inf views   4: all three
    values = np.array([[[nan, 1.5, 2.0, nan, 1.0]], [[7.0, nan, 4.0, inf, 2.0]], [[nan, nan, 9.0, 5.0, 6.0]]], dtype=np.float32)
    states = np.array([[O.NODATA, O.KEPT, O.KEPT, O.KEPT, O.KEPT], [O.OCCLUDED, O.OUTSIDE, O.KEPT, O.KEPT, O.KEPT],
                       [O.OUTSIDE, O.OCCLUDED, O.KEPT, O.KEPT, O.KEPT]], dtype=np.uint8)
    got = M.fuse(values, states, [4, 4, 9])
    assert got["count"].tolist() == [0, 1, 3, 1, 3]
    assert got["best"].tolist() == [-1, 0, 0, 2, 0]                                  # equal ranks go to the lower index
    assert np.isnan(got["best_val"][0, 0]) and np.isnan(got["mean"][0, 0]) and np.isnan(got["std"][0, 0])
    assert got["std"][0, 1] == 0.0 and got["mean"][0, 1] == np.float32(1.5) and got["best_val"][0, 1] == np.float32(1.5)
    assert got["states"][:, 3].tolist() == [M.NONFINITE, M.NONFINITE, M.USED]        # the others still fuse
    assert got["mean"][0, 3] == 5.0 and got["std"][0, 3] == 0.0 and got["best_val"][0, 3] == 5.0
    assert got["mean"][0, 4] == 3.0 and got["std"][0, 4] == np.float32(np.sqrt(14.0 / 3.0))
    assert got["counts"].tolist() == [[1, 0, 0, 3, 1], [0, 1, 1, 2, 1], [0, 1, 1, 3, 0]]
    cells = [2, 4]
    want_q = int(sum(np.rint(np.sqrt(np.float64(M2) / 3.0) * 2.0 ** 20) for M2 in (26.0, 14.0)))
    assert got["sums"] == [len(cells), want_q, 0]
    other = M.fuse(values, states, [9, 4, 1])                                        # a permuted rank moves `best` and nothing else
    assert other["best"].tolist() == [-1, 0, 2, 2, 2] and other["best_val"][0].tolist()[1:] == [1.5, 9.0, 5.0, 6.0]
    for key in ("count", "states", "counts", "sums"):
        assert np.array_equal(other[key], got[key]), key
    assert O.same_f32(other["mean"], got["mean"]) and O.same_f32(other["std"], got["std"])
    huge = M.fuse(np.array([[[3e38]], [[-3e38]]], dtype=np.float32), np.full((2, 1), O.KEPT), [0, 1])
    assert huge["sums"] == [1, 0, 1] and np.isfinite(huge["mean"][0, 0])             # a spread of 2^20 or more is counted, not summed


def test_box_scene_is_seen_by_zero_to_three_views():
    """A condition on the inputs of the GPU end-to-end test, asserted on the statement alone."""
    ds, dsm, xoff, yoff, res, zone = M.box_views()
    planes = [O.linear_image(*O.SCENE_IMAGE, 3) for _ in ds]
    got = M.mosaic(ds, planes, dsm, xoff, yoff, res, zone)
    hist = np.bincount(got["count"].ravel(), minlength=4).tolist()
    print(f"box scene under seeds {M.SCENE_SEEDS}: cells seen by 0 / 1 / 2 / 3 views {hist}; occluded per view "
          f"{got['counts'][:, O.OCCLUDED].tolist()}; rank {got['rank']}; consistency {M.consistency(got['sums'], 3):.6g}")
    assert hist[0] >= 10 and hist[1] >= 100 and hist[2] >= 200 and hist[3] >= 1000
    assert got["counts"][:, M.NONFINITE].sum() == 0 and got["counts"].sum() == 3 * dsm.size
    assert sorted(got["rank"]) == [0, 1, 2]
    assert np.array_equal(got["best"] == -1, got["count"] == 0)


def test_package_surface():
    import brdf_nerf_amd
    from brdf_nerf_amd import _lib
    from brdf_nerf_amd.build import FILE_FLAGS
    assert "orthomosaic" in brdf_nerf_amd.__all__ and callable(brdf_nerf_amd.orthomosaic)
    assert callable(brdf_nerf_amd.functions.grid_mosaic)
    assert "-ffp-contract=off" in FILE_FLAGS["mosaic.hip"]
    csrc = os.path.join(ROOT, "brdf_nerf_amd", "csrc")
    for f in ("mosaic.hip", "gather_rule.h"):
        assert "#pragma clang fp contract(off)" in open(os.path.join(csrc, f)).read()
    for f in ("mosaic.hip", "orthophoto.hip"):
        assert '#include "gather_rule.h"' in open(os.path.join(csrc, f)).read()          # one statement of the taps, shared
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    assert "Orthomosaic of several observed images" in header
    declared = set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", header))
    assert "bn_grid_mosaic" in declared and "bn_grid_mosaic" in _lib.exported_symbols() and len(_lib._SIGS["bn_grid_mosaic"][1]) == 24
    assert re.search(r"#define BN_ABI_VERSION 7\b", header) and _lib.BN_ABI_VERSION == 7
    for name, value in (("BN_MOSAIC_MAX_VIEWS", M.MAX_VIEWS), ("BN_MOSAIC_MAX_CHANNELS", M.MAX_CHANNELS)):
        assert re.search(rf"#define {name} {value}\b", header) and getattr(_lib, name) == value, name
    assert re.search(r"BN_MOSAIC_USED = 3, BN_MOSAIC_NONFINITE = 4", header)
    assert (_lib.BN_MOSAIC_USED, _lib.BN_MOSAIC_NONFINITE) == (M.USED, M.NONFINITE) == (3, 4)
    # the struct as the header implies it: two pointers, two int32, three int64, an int32 padded to 8, 90 doubles
    body = re.search(r"typedef struct \{([^}]*)\} bn_mosaic_view;", header).group(1)
    size, align = {"const float *": 8, "const uint8_t *": 8, "int32_t": 4, "int64_t": 8, "bn_rpc": 720}, 8
    at = 0
    for decl in (d.strip() for d in re.sub(r"/\*.*?\*/", "", body).split(";") if d.strip()):
        kind = next(k for k in size if decl.startswith(k))
        for _ in decl[len(kind):].split(","):
            unit = min(size[kind], align)
            at = (at + unit - 1) // unit * unit + size[kind]
    at = (at + align - 1) // align * align
    assert ctypes.sizeof(_lib.Rpc) == 720 and at == ctypes.sizeof(_lib.MosaicView) == 776
    assert _lib.MosaicView.rpc.offset == 56 and _lib.MosaicView.rank.offset == 48
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "## Orthomosaic of several observed images" in readme


def test_wrapper_refusals_without_a_device():
    from brdf_nerf_amd import Grid, Rpc, orthomosaic
    rpc = Rpc.from_dict(K.make_rpc("z17", 1))
    grid = Grid(0.0, 0.0, 0.5, 5, 4)
    dsm, img = torch.zeros(4, 5), torch.zeros(6 * 7, 3)
    view = (img, 6, 7, rpc)
    with pytest.raises(ValueError, match="0 views"):
        orthomosaic([], dsm, grid, 17)
    with pytest.raises(ValueError, match="33 views"):
        orthomosaic([view] * 33, dsm, grid, 17)
    with pytest.raises(ValueError, match="channels"):
        orthomosaic([view, (torch.zeros(6 * 7, 2), 6, 7, rpc)], dsm, grid, 17)
    with pytest.raises(ValueError, match="channels"):
        orthomosaic([(torch.zeros(6 * 7, 5), 6, 7, rpc)], dsm, grid, 17)
    with pytest.raises(ValueError, match="view 1"):
        orthomosaic([view, (img, 6, 7)], dsm, grid, 17)
    for rank in ([0], [0, 1, 2], [0, 1.5], [0, True], [0, 1 << 31]):
        with pytest.raises(ValueError, match="rank"):
            orthomosaic([view, view], dsm, grid, 17, rank=rank)
    for vd, what in (([[0.0, 0.0, 1.0]], "view_dirs"), ([0.0, 0.0, 1.0], "view_dirs"), ([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]], "upwards"),
                     ([[0.0, 0.0, 1.0], [0.0, float("nan"), 1.0]], "finite"), (torch.ones(2, 3, dtype=torch.int64), "view_dirs")):
        with pytest.raises(ValueError, match=what):
            orthomosaic([view, view], dsm, grid, 17, view_dirs=vd)
    for bad, what in ((img.double(), "float32"), (img[:, :2], "contiguous"), (img.numpy(), "tensor")):
        with pytest.raises(ValueError, match=what):
            orthomosaic([view, (bad, 6, 7, rpc)], dsm, grid, 17)
    with pytest.raises(ValueError, match="pixels"):
        orthomosaic([(img, 6, 8, rpc)], dsm, grid, 17)
    for bad, what in ((dsm.double(), "float32"), (dsm[:, ::2], "contiguous"), (torch.zeros(5, 4), "grid")):
        with pytest.raises(ValueError, match=what):
            orthomosaic([view], bad, grid, 17)
    for kw, what in ((dict(mode="cubic"), "mode"), (dict(layout="chw"), "layout"), (dict(rows=(2, 1)), "rows"), (dict(rows=(0, 5)), "rows"),
                     (dict(eps=-1.0), "eps"), (dict(alt_bounds=(5.0, 5.0)), "alt_bounds"), (dict(zone=61), "zone"),
                     (dict(colrow=torch.zeros(1, 4, 5, 2)), "float64"), (dict(colrow=torch.zeros(2, 4, 5, 2, dtype=torch.float64)), "colrow")):
        kw = dict(dict(zone=17), **kw)
        with pytest.raises(ValueError, match=what):
            orthomosaic([view], dsm, grid, **kw)
    with pytest.raises(ValueError, match="device"):
        orthomosaic([view], dsm, grid, 17)
