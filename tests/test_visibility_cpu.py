"""The visibility rule's numpy statement on its own cases, the package surface and the wrapper refusals: no GPU, no library."""
import os
import re

import numpy as np
import pytest
import torch

import visibility_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases():
    """(name, dsm, directions, eps) of every grid the statement is run on here."""
    return [("block", V.block_scene(), np.stack([V.direction(*d) for d in V.BLOCK_DIRS]), 0.0),
            ("relief", V.relief(33, 65, seed=5), V.all_dirs(), 0.0),
            ("relief_eps", V.relief(20, 31, seed=9), V.oblique_dirs(), 0.75),
            ("tie", V.tie_row(), V.TIE_DIR[None], 0.0)]


def test_block_scene_counts():
    """The prototype's counts on the 64 x 64 block scene, direction by direction."""
    dsm = V.block_scene()
    vis, hit, counts = V.grid_statement(dsm, V.RES, [V.direction(*d) for d in V.BLOCK_DIRS])
    assert [int(c) for c in counts[:, 0]] == V.BLOCK_BLOCKED
    assert (counts[0] == [744, 3352, 0]).all() and (counts.sum(-1) == 64 * 64).all()
    # (45, 90): the sun due east at 45 degrees, so the march runs east and the cells WEST of the roof look at the sun through it:
    # the roof's 16 rows times the 24 cells to the western edge
    assert (vis[1][24:40, 0:24] == V.BLOCKED).all() and (vis[1] == V.BLOCKED).sum() == 384
    assert ((hit >= 0) == (vis == V.BLOCKED)).all()
    assert (dsm.reshape(-1)[hit[hit >= 0]] == 30.0).all()          # every blocking cell is a roof cell


def test_flat_grid_and_zenith_are_all_visible():
    flat = np.full((9, 13), 4.0, dtype=np.float32)
    vis, hit, counts = V.grid_statement(flat, V.RES, V.all_dirs())
    assert (vis == V.VISIBLE).all() and (hit == -1).all() and (counts == [0, 9 * 13, 0]).all()
    rough = V.relief(33, 65, seed=2)
    vis, hit, counts = V.grid_statement(rough, V.RES, [V.ZENITH, V.ZENITH * 7.5])
    assert ((vis == V.VISIBLE) == np.isfinite(rough)).all() and ((vis == V.NODATA) == ~np.isfinite(rough)).all() and (hit == -1).all()


@pytest.mark.parametrize("name", [c[0] for c in cases()])
def test_zmax_changes_no_bit(name):
    _, dsm, dirs, eps = next(c for c in cases() if c[0] == name)
    plain = V.grid_statement(dsm, V.RES, dirs, eps)
    early = V.grid_statement(dsm, V.RES, dirs, eps, zmax=V.grid_zmax(dsm))
    for a, b in zip(plain, early):
        assert np.array_equal(a, b)


def test_raising_eps_never_blocks_a_visible_start():
    dsm = V.relief(33, 65, seed=5)
    dirs = V.oblique_dirs()
    before = V.grid_statement(dsm, V.RES, dirs, 0.0)[0]
    assert (before == V.BLOCKED).sum() > 500
    for eps in (0.25, 1.0, 8.0):
        after = V.grid_statement(dsm, V.RES, dirs, eps)[0]
        assert not ((before == V.VISIBLE) & (after == V.BLOCKED)).any() and ((before == V.NODATA) == (after == V.NODATA)).all()
        assert (after == V.BLOCKED).sum() < (before == V.BLOCKED).sum()
        before = after


def test_grid_mode_is_point_mode_on_the_cell_centres():
    """On a dyadic origin and resolution the centres and the quotients are exact: both modes give the same bits."""
    xoff, yoff, res = 1024.0, 2048.0, 0.5
    for dsm in (V.block_scene(), V.relief(33, 65, seed=5)):
        dirs = V.all_dirs()
        g = V.grid_statement(dsm, res, dirs)
        p = V.points_statement(V.cell_centres(dsm, xoff, yoff, res), dsm, xoff, yoff, res, dirs)
        assert np.array_equal(g[0].reshape(len(dirs), -1), p[0]) and np.array_equal(g[1].reshape(len(dirs), -1), p[1])
        assert np.array_equal(g[2], p[2])


def test_both_sides_of_the_tie():
    a = abs(V.TIE_DIR[0])
    assert V.TIE_DIR[0] / a == 1.0 and (V.TIE_DIR[2] / a) * V.RES == 0.5          # su and sz are exact
    for eps in (0.0, 0.25):
        on = V.grid_statement(V.tie_row(eps), V.RES, V.TIE_DIR, eps)
        over = V.grid_statement(V.tie_row(eps, above=True), V.RES, V.TIE_DIR, eps)
        assert on[0][0, 0, 0] == V.VISIBLE and on[1][0, 0, 0] == -1               # h == zt + eps at t = 4: not blocked
        assert over[0][0, 0, 0] == V.BLOCKED and over[1][0, 0, 0] == 4
        assert (on[0][0, 0, 1:4] == V.BLOCKED).all() and (on[0][0, 0, 4:] == V.VISIBLE).all()


def test_points_outside_and_without_data():
    dsm = V.block_scene()
    pts = np.array([[5.0, -5.0, 25.0], [-0.25, -5.0, 11.0], [5.0, 0.25, 11.0], [32.0, -5.0, 11.0], [5.0, -32.0, 11.0],
                    [np.nan, -5.0, 11.0], [5.0, -5.0, np.inf], [0.0, 0.0, 25.0], [5.0, -5.0, 11.0]])
    vis, hit, counts = V.points_statement(pts, dsm, 0.0, 0.0, V.RES, V.direction(30.0, 135.0))
    assert vis[0].tolist() == [1, 2, 2, 2, 2, 2, 2, 1, 0] and hit[0][:8].tolist() == [-1] * 8 and counts[0].tolist() == [1, 2, 6]
    # azimuth 135: |dx| and |dy| differ in the last bit, so from the corner (10, 10) one axis arrives a hair short of cell 24
    assert divmod(int(hit[0][8]), 64) in ((24, 24), (24, 25), (25, 24))


def test_package_surface():
    import brdf_nerf_amd
    from brdf_nerf_amd import _lib
    from brdf_nerf_amd.build import FILE_FLAGS
    for name in ("grid_visibility", "point_visibility", "view_visibility"):
        assert name in brdf_nerf_amd.__all__ and callable(getattr(brdf_nerf_amd, name))
    assert "-ffp-contract=off" in FILE_FLAGS["visibility.hip"]
    src = open(os.path.join(ROOT, "brdf_nerf_amd", "csrc", "visibility.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    assert "Visibility over a surface model" in header
    declared = set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", header))
    for name, nargs in (("bn_grid_visibility", 14), ("bn_points_visibility", 16)):
        assert name in declared and name in _lib.exported_symbols() and len(_lib._SIGS[name][1]) == nargs, name
    assert (_lib.BN_VIS_BLOCKED, _lib.BN_VIS_VISIBLE, _lib.BN_VIS_NODATA) == (V.BLOCKED, V.VISIBLE, V.NODATA) == (0, 1, 2)
    for name, value in (("BN_VIS_BLOCKED", 0), ("BN_VIS_VISIBLE", 1), ("BN_VIS_NODATA", 2), ("BN_VIS_MAX_DIRS", _lib.BN_VIS_MAX_DIRS)):
        assert re.search(rf"#define {name} {value}\b", header), name


def test_wrapper_refusals_without_a_device():
    from brdf_nerf_amd import Grid, SceneFrame, grid_visibility, point_visibility, score_view, view_visibility
    from brdf_nerf_amd import functions as Fn
    dsm = torch.zeros(4, 5)
    up = [0.0, 0.0, 1.0]
    grid = Grid(0.0, 0.0, 0.5, 5, 4)
    for bad, what in ((dsm.double(), "float32"), (dsm[:, ::2], "contiguous"), (dsm[0], "2-D"), (dsm.numpy(), "tensor"), (dsm, "device")):
        with pytest.raises(ValueError, match=what):
            grid_visibility(bad, 0.5, up)
    for dirs, what in (([0.0, 0.0, 0.0], "horizon"), ([0.0, 1.0, -0.5], "horizon"), ([float("nan"), 0.0, 1.0], "finite"),
                       ([[0.0, float("inf"), 1.0]], "finite"), (torch.zeros(2, 4), r"\(K, 3\)"), (torch.zeros(0, 3), r"\(K, 3\)"),
                       (torch.ones(4097, 3), "4096"), (torch.ones(3, dtype=torch.int64), "float")):
        with pytest.raises(ValueError, match=what):
            grid_visibility(dsm, 0.5, dirs)
        with pytest.raises(ValueError, match=what):
            Fn.points_visibility(torch.zeros(3, 3, dtype=torch.float64), dsm, 0.0, 0.0, 0.5, dirs)
    for kw, what in ((dict(resolution=0.0), "resolution"), (dict(resolution=float("inf")), "resolution"), (dict(eps=-1.0), "eps"),
                     (dict(eps=float("nan")), "eps"), (dict(rows=(2, 1)), "rows"), (dict(rows=(0, 5)), "rows"), (dict(dir_tile=0), "dir_tile")):
        with pytest.raises(ValueError, match=what):
            grid_visibility(dsm, **dict(dict(resolution=0.5, dirs=up), **kw))
    with pytest.raises(ValueError, match="zmax"):
        Fn.grid_visibility(dsm, 0.5, up, zmax=float("nan"))
    pts = torch.zeros(3, 3, dtype=torch.float64)
    for bad, what in ((pts.float(), "float64"), (pts[:, :2], r"\(R, 3\)"), (pts.numpy(), "tensor"), (pts, "device")):
        with pytest.raises(ValueError, match=what):
            point_visibility(bad, dsm, grid, up)
    with pytest.raises(ValueError, match="grid"):
        point_visibility(pts, torch.zeros(5, 4), grid, up)
    with pytest.raises(ValueError, match="origin"):
        Fn.points_visibility(pts, dsm, float("nan"), 0.0, 0.5, up)
    rays = torch.zeros(12, 11)
    with pytest.raises(ValueError, match="ecef"):
        view_visibility(rays, torch.zeros(12), SceneFrame.ecef((6378137.0, 0.0, 0.0), 100.0), dsm, grid, up)
    args = (None, None, rays, torch.zeros(12, 3), 3, 4)
    with pytest.raises(ValueError, match="frame"):
        score_view(*args, sun_dir=up)
    with pytest.raises(ValueError, match="ecef"):
        score_view(*args, sun_dir=up, frame=SceneFrame.ecef((6378137.0, 0.0, 0.0), 100.0))
    utm = SceneFrame((0.0, 0.0, 0.0), 100.0)
    with pytest.raises(ValueError, match="shadow_dsm"):
        score_view(*args, sun_dir=up, frame=utm, grid=grid, shadow_dsm=torch.zeros(5, 4))
    with pytest.raises(ValueError, match="horizon"):
        score_view(*args, sun_dir=[0.0, 1.0, 0.0], frame=utm)
    with pytest.raises(ValueError, match="ONE direction"):
        score_view(*args, sun_dir=torch.ones(2, 3), frame=utm)
    with pytest.raises(ValueError, match="eps"):
        score_view(*args, sun_dir=up, frame=utm, shadow_eps=-0.5)
