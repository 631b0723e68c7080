"""The ray-casting rule's numpy statement on its own cases, the perturbed rules, the package surface and the wrapper refusals: no
GPU, no library.

What each perturbation of the statement breaks (test_perturbations):
  le=np.less   the graze alone among the engineered cases (TOP at 4.5 -> MISS); "below_at_near" (z_in == h at the start) too
  tie='u'      the corner case alone (MISS -> WALL at cell 1)
  top='out'    the block scene's TOP depths (every top is reported where the ray leaves the cell) and two of the closed forms
A running-sum form of lam_u is NOT seen by these cases and no test claims it.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

import cast_cases as K
import visibility_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def block(origin):
    dsm, rays, center, rng, xoff, yoff = K.block_view(origin)
    return dsm, rays, center, rng, xoff, yoff, K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES)


def test_block_scene_counts():
    """The statement's classes on the 48 x 48 view of the block scene: tops, walls and nothing else, the same at a dyadic and at a
    UTM-sized origin."""
    dsm, rays, center, rng, xoff, yoff, (depth, state, cell, nan_cells, counts) = block("dyadic")
    assert counts.tolist() == [K.BLOCK_COUNTS["top"], K.BLOCK_COUNTS["wall"], 0, 0, 0] and counts.sum() == 48 * 48
    heights = dsm.reshape(-1)[cell]
    assert int(((state == K.TOP) & (heights == 30.0)).sum()) == K.BLOCK_COUNTS["roof"]
    assert (heights[state == K.WALL] == 30.0).all()                 # only the building has walls
    assert np.isfinite(depth).all() and (nan_cells == 0).all()
    utm = block("utm")[6]
    assert np.array_equal(utm[1], state) and np.array_equal(utm[2], cell) and np.array_equal(utm[4], counts)
    # the depths are those of the same geometry: equal up to the float32 rounding of the normalised origins
    assert np.abs(utm[0] - depth).max() * rng < 1e-3


def test_top_hits_land_on_the_surface():
    """point_cloud's expression on a TOP depth gives the cell's height within 2^-23 far range metres (one float32 rounding of the
    depth moves the point by at most 2^-24 far range along the ray; doubled)."""
    for origin in K.ORIGINS:
        dsm, rays, center, rng, xoff, yoff, (depth, state, cell, _, _) = block(origin)
        top = state == K.TOP
        r64 = rays.astype(np.float64)
        p = (r64[:, 0:3] + r64[:, 3:6] * depth.astype(np.float64)[:, None]) * rng + np.asarray(center)
        bound = 2.0 ** -23 * float(rays[:, 7].max()) * rng
        err = np.abs(p[top, 2] - dsm.reshape(-1)[cell[top]])
        assert err.max() <= bound, (origin, err.max(), bound)
        # ... and the point lies over the cell that was hit, or within that bound of its edge (the lattice aims every tenth column and
        # row at a cell edge)
        u, v = (p[top, 0] - xoff) / K.RES, (yoff - p[top, 1]) / K.RES
        j, i = np.divmod(cell[top], 64)
        out = np.maximum(np.maximum(i - u, u - (i + 1)), np.maximum(j - v, v - (j + 1)))
        assert out.max() * K.RES <= bound and (out <= 0).sum() > 1500, (origin, out.max() * K.RES)


def test_closed_form_hits():
    dsm, rays, center, rng, xoff, yoff, want = K.closed_form_cases()
    depth, state, cell, nan_cells, counts = K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES)
    assert [(int(s), float(d), int(c)) for s, d, c in zip(state, depth, cell)] == want
    assert counts.tolist() == [2, 1, 0, 0, 0]


def test_graze_and_corner():
    dsm, rays, center, rng, xoff, yoff = K.graze_case()
    depth, state, cell, _, _ = K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES)
    assert (int(state[0]), float(depth[0]), int(cell[0])) == (K.TOP, 4.5, 4)
    dsm, rays, center, rng, xoff, yoff = K.corner_case()
    depth, state, cell, _, _ = K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES)
    assert int(state[0]) == K.MISS and np.isnan(depth[0]) and int(cell[0]) == -1


def test_single_cases():
    dsm, cases, center, rng, xoff, yoff = K.single_cases()
    for name, (r, (want_state, want_depth, want_cell, want_nan)) in cases.items():
        depth, state, cell, nan_cells, counts = K.cast_statement(r, center, rng, dsm, xoff, yoff, K.RES)
        assert int(state[0]) == want_state and int(cell[0]) == want_cell and int(nan_cells[0]) == want_nan, name
        assert (np.isnan(depth[0]) if want_depth is None else float(depth[0]) == want_depth), name
        assert counts.sum() == 1 and counts[want_state] == 1, name
    assert {c[1][0] for c in cases.values()} == {K.TOP, K.MISS, K.NODATA, K.BELOW}
    # +inf always stops a ray, -inf never does; -0.0 is 0
    row = np.array([[-np.inf, np.inf, -0.0]], dtype=np.float32)
    east = K.ray((0.25, 0.25, 5.0), (0.5, 0.0, -0.5), 0.0, 16.0)
    got = K.cast_statement(east, (0.0, 0.0, 0.0), 1.0, row, 0.0, 0.5, K.RES)
    assert (int(got[1][0]), float(got[0][0]), int(got[2][0])) == (K.WALL, 0.5, 1)
    west = K.ray((1.25, 0.25, 0.25), (-0.5, 0.0, -0.5), 0.0, 16.0)
    got = K.cast_statement(west, (0.0, 0.0, 0.0), 1.0, row, 0.0, 0.5, K.RES)
    assert (int(got[1][0]), float(got[0][0]), int(got[2][0])) == (K.TOP, 0.5, 2)        # z == 0.0 == -0.0 at s = 0.5


def all_cases():
    """(name, rays, center, rng, dsm, xoff, yoff) of every case of this file."""
    out = []
    for origin in K.ORIGINS:
        dsm, rays, center, rng, xoff, yoff = block(origin)[:6]
        out.append(("block_" + origin, rays, center, rng, dsm, xoff, yoff))
    for name, case in (("graze", K.graze_case()), ("corner", K.corner_case()), ("closed", K.closed_form_cases()[:6])):
        dsm, rays, center, rng, xoff, yoff = case
        out.append((name, rays, center, rng, dsm, xoff, yoff))
    dsm, cases, center, rng, xoff, yoff = K.single_cases()
    out += [(name, r, center, rng, dsm, xoff, yoff) for name, (r, _) in cases.items()]
    dsm = K.grid_case((33, 65))
    for el in K.ELEVATIONS:
        rays, center, rng = K.scatter_view(257, dsm, *K.ORIGINS["utm"], el, 17.0)
        out.append((f"relief_{el:g}", rays, center, rng, dsm, *K.ORIGINS["utm"]))
    return out


def test_zmax_changes_no_bit():
    """zmax = the maximum of the non-NaN cells against zmax = inf, on every case."""
    for name, rays, center, rng, dsm, xoff, yoff in all_cases():
        plain = K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES)
        early = K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES, zmax=V.grid_zmax(dsm))
        assert same(plain, early), name


def test_nan_cells_are_counted_and_never_hit():
    dsm = K.grid_case((33, 65))
    assert np.isnan(dsm).sum() > 50
    for el in (80.0, 45.0, 12.0):
        rays, center, rng = K.scatter_view(257, dsm, *K.ORIGINS["utm"], el, 17.0)
        depth, state, cell, nan_cells, counts = K.cast_statement(rays, center, rng, dsm, *K.ORIGINS["utm"], K.RES)
        hit = cell >= 0
        assert hit.any() and not np.isnan(dsm.reshape(-1)[cell[hit]]).any()
        assert nan_cells.sum() > 0 and (nan_cells[state == K.NODATA] == 0).all()
        assert ((cell >= 0) == np.isin(state, (K.TOP, K.WALL, K.BELOW))).all() and (np.isnan(depth) == ~hit).all()


def test_perturbations():
    """Each perturbed rule fails exactly the case built for it (the module docstring records the lists)."""
    changed = {}
    for name, rays, center, rng, dsm, xoff, yoff in all_cases():
        want = K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES)
        for key, kw in (("lt", dict(le=np.less)), ("tie_u", dict(tie="u")), ("top_out", dict(top="out"))):
            if not same(K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES, **kw), want):
                changed.setdefault(key, []).append(name)
    assert changed["lt"] == ["graze", "below_at_near"]
    assert changed["tie_u"] == ["corner"]
    assert "block_dyadic" in changed["top_out"] and "block_utm" in changed["top_out"] and "closed" in changed["top_out"]
    dsm, rays, center, rng, xoff, yoff = K.graze_case()
    assert int(K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES, le=np.less)[1][0]) == K.MISS
    dsm, rays, center, rng, xoff, yoff = K.corner_case()
    got = K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES, tie="u")
    assert (int(got[1][0]), int(got[2][0])) == (K.WALL, 1)
    dsm, rays, center, rng, xoff, yoff, want = block("dyadic")
    out = K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES, top="out")
    top = want[1] == K.TOP
    assert np.array_equal(out[1], want[1]) and (out[0][top] != want[0][top]).sum() > 1500      # the classes stay, the depths move
    assert (out[0][top] >= want[0][top]).all()                      # (only a ray aimed at a cell's far edge keeps its depth)


def test_surface_prior_statement():
    dsm, rays, center, rng, xoff, yoff, cast = block("utm")
    holes = dsm.copy()
    holes[30:34, :] = np.nan
    cast = K.cast_statement(rays, center, rng, holes, xoff, yoff, K.RES)
    depths, valid, std = K.surface_prior_statement(cast, weight=0.75, stdscale=2.0, margin=0.5, std_span=3.0)
    keep = np.isin(cast[1], (K.TOP, K.WALL)) & (cast[3] == 0)
    assert 0 < keep.sum() < keep.size and np.array_equal(valid, keep.astype(np.float32))
    assert (depths[keep, 0] == cast[0][keep]).all() and (depths[keep, 1] == 0.75).all() and (std[keep] == 3.0).all()
    assert (depths[~keep, 0] == np.float32(cast[0][keep].astype(np.float64).mean())).all() and (depths[~keep, 1] == 0).all()
    assert (std[~keep] == 0).all()


def test_package_surface():
    import brdf_nerf_amd
    from brdf_nerf_amd import _lib, raycast
    from brdf_nerf_amd.build import FILE_FLAGS
    for name in ("cast_rays", "grid_to_view", "surface_priors"):
        assert name in brdf_nerf_amd.__all__ and callable(getattr(brdf_nerf_amd, name))
    assert callable(brdf_nerf_amd.functions.cast_rays)
    assert "-ffp-contract=off" in FILE_FLAGS["raycast.hip"]
    src = open(os.path.join(ROOT, "brdf_nerf_amd", "csrc", "raycast.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "block_sums::block_count" in src and "atomicAdd" not in src
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    assert "Depth of a surface model along a ray" in header
    declared = set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", header))
    assert "bn_cast_rays" in declared and "bn_cast_rays" in _lib.exported_symbols() and len(_lib._SIGS["bn_cast_rays"][1]) == 18
    codes = (("BN_CAST_TOP", K.TOP), ("BN_CAST_WALL", K.WALL), ("BN_CAST_MISS", K.MISS), ("BN_CAST_NODATA", K.NODATA),
             ("BN_CAST_BELOW", K.BELOW), ("BN_CAST_MAX_SPAN", int(K.MAX_SPAN)))
    for k, (name, value) in enumerate(codes):
        assert getattr(_lib, name) == value and re.search(rf"#define {name} {value}\b", header), name
    assert [c[1] for c in codes[:5]] == [0, 1, 2, 3, 4]
    assert (raycast.TOP, raycast.WALL, raycast.MISS, raycast.NODATA, raycast.BELOW) == (0, 1, 2, 3, 4)


def test_wrapper_refusals_without_a_device():
    from brdf_nerf_amd import Grid, SceneFrame, cast_rays, grid_to_view, score_view, surface_priors
    from brdf_nerf_amd import functions as Fn
    dsm = torch.zeros(4, 5)
    grid = Grid(0.0, 0.0, 0.5, 5, 4)
    utm = SceneFrame((0.0, 0.0, 0.0), 100.0)
    ecef = SceneFrame.ecef((6378137.0, 0.0, 0.0), 100.0)
    rays = torch.zeros(12, 11)
    for fn in (cast_rays, surface_priors):
        with pytest.raises(ValueError, match="ecef"):
            fn(rays, ecef, dsm, grid)
        for bad, what in ((dsm.double(), "float32"), (dsm[:, ::2], "contiguous"), (dsm[0], "2-D"), (torch.zeros(5, 4), "grid"),
                          (dsm, "device")):
            with pytest.raises(ValueError, match=what):
                fn(rays, utm, bad, grid)
        for bad, what in ((rays.double(), "float32"), (rays[:, :7], "rays"), (rays.numpy(), "tensor")):
            with pytest.raises(ValueError, match=what):
                fn(bad, utm, dsm, grid)
    with pytest.raises(ValueError, match="chunk"):
        cast_rays(rays, utm, dsm, grid, chunk=0)
    base = dict(center=(0.0, 0.0, 0.0), rng=1.0, dsm=dsm, xoff=0.0, yoff=0.0, res=0.5)
    nan, inf = float("nan"), float("inf")
    for kw, what in ((dict(res=0.0), "resolution"), (dict(res=inf), "resolution"), (dict(rng=0.0), "range"), (dict(rng=nan), "range"),
                     (dict(center=(0.0, inf, 0.0)), "centre"), (dict(center=(0.0, 0.0)), "centre"), (dict(xoff=nan), "origin"),
                     (dict(yoff=-inf), "origin"), (dict(zmax=nan), "zmax")):
        with pytest.raises(ValueError, match=what):
            Fn.cast_rays(rays, **dict(base, **kw))
    with pytest.raises(ValueError, match="device"):
        Fn.cast_rays(rays, **base)
    # grid_to_view is plain torch: it runs here
    layer = torch.arange(20, dtype=torch.float32).reshape(4, 5)
    cell = torch.tensor([3, -1, 19, 0], dtype=torch.int32)
    out = grid_to_view(layer, cell)
    assert out[[0, 2, 3]].tolist() == [3.0, 19.0, 0.0] and bool(torch.isnan(out[1]))
    assert grid_to_view(layer.long(), cell, fill=-7).tolist() == [3, -7, 19, 0]
    assert grid_to_view(layer > 4, cell, fill=False).tolist() == [False, False, True, False]
    for args, what in (((layer.long(), cell), "fill"), ((layer[0], cell), "raster"), ((layer, cell.float()), "int32"),
                       ((layer, torch.tensor([20])), "outside")):
        with pytest.raises(ValueError, match=what):
            grid_to_view(*args)
    args = (None, None, rays, torch.zeros(12, 3), 3, 4)
    with pytest.raises(ValueError, match="frame"):
        score_view(*args, cast_dsm=dsm)
    with pytest.raises(ValueError, match="grid"):
        score_view(*args, cast_dsm=dsm, frame=utm)
    with pytest.raises(ValueError, match="ecef"):
        score_view(*args, cast_dsm=dsm, frame=ecef, grid=grid)
    with pytest.raises(ValueError, match="cast_dsm"):
        score_view(*args, cast_dsm=torch.zeros(5, 4), frame=utm, grid=grid)
