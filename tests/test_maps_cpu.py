"""CPU tests of the validation maps: the numpy statements of tests/maps_cases.py held to goldens recorded from the reference
(tests/golden/make_maps_goldens.py), the ABI declarations and the refusals of the wrappers.  No GPU, no library call."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import maps_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", M.RAY_GOLDENS)
def test_ray_statement_against_the_reference(name):
    """surf_idx and surf equal the reference's np.argmin + get_surface_feature bit for bit; the counts behind check_vec0 and
    perc_ng_nr are the reference's.  std: within (S + 3) 2^-25 relative of the reference's float32 value - a float32 sum of S
    non-negative three-operation terms in any order is within (S + 3) 2^-24 of the exact one, and the square root halves a relative
    error.  depth_std from the integer sum: within that bound (relative) plus 2^-21 (the half quantum of 2^-20) of the
    reference's mean.  accum: within (S + 2) 2^-24 of sum_s |w X|."""
    g = M.golden(name)
    z, w, depth, X, view, nc = g["z"], g["w"], g["depth"], g["X"], g["view"], int(g["normal_col"])
    R, S, E = X.shape
    got = M.ray_statement(z, w, depth, X, nc, view, accumulate=True)
    assert np.array_equal(got["surf_idx"].astype(np.int64), g["ref_idx"])
    assert np.array_equal(M.bits(got["surf"]), M.bits(g["ref_surf"]))
    c = got["counters"]
    assert c["nr_total"] == R * S and c["std_count"] == R and c["std_skipped"] == 0
    assert 100.0 * c["nr0"] / c["nr_total"] == float(g["ref_vec0"]) and c["nr0"] > 0
    assert float(np.float32(c["bad_nr"] * 100.0 / c["nr_total"])) == float(g["ref_bad"]) and 0 < c["bad_nr"] < c["nr_total"]
    bound = (S + 3) * 2.0 ** -25
    ref_std = g["ref_std"].astype(np.float64)
    rel = np.abs(got["std"].astype(np.float64) - ref_std) / ref_std
    print(f"{name}: std max rel gap {rel.max():.3e} (bound {bound:.3e})")
    assert rel.max() <= bound
    rel_var = np.abs(got["var"].astype(np.float64) - g["ref_var"].astype(np.float64)) / g["ref_var"].astype(np.float64)
    assert rel_var.max() <= 2 * bound
    mean = c["std_sum"] / (c["std_count"] * M.STD_FIX)
    gap = abs(mean - float(g["ref_std_mean"]))
    print(f"{name}: depth_std {mean!r} vs the reference's mean {float(g['ref_std_mean'])!r}: gap {gap:.3e}")
    assert gap <= bound * float(g["ref_std_mean"]) + 2.0 ** -21
    scale = (np.abs(w.astype(np.float64))[:, :, None] * np.abs(X.astype(np.float64))).sum(1)
    err = np.abs(got["accum"].astype(np.float64) - g["ref_accum"].astype(np.float64))
    print(f"{name}: accum max err / sum|wX| {np.max(err / scale):.3e} (bound {(S + 2) * 2.0 ** -24:.3e})")
    assert (err <= (S + 2) * 2.0 ** -24 * scale).all()


@pytest.mark.parametrize("name", M.NORMAL_GOLDENS)
def test_point_normals_statement_against_the_reference(name):
    """round_f32 normals against the reference's float32 result on the float32-rounded points: within 8 x the gap the generator
    measured for this fixture (float32 headroom; the gap itself is not derivable).  valid_normal equals the reference's bit for
    bit.  On the UTM fixture the exact reading differs from the reference's by more than 5 degrees somewhere."""
    g = M.golden(name)
    got = M.point_normals(g["points"], round_f32=True)
    gap = np.abs(got.astype(np.float64) - g["ref_normals"].astype(np.float64)).max()
    print(f"{name}: gap {gap:.3e} (stored {float(g['gap']):.3e})")
    assert gap <= 8 * float(g["gap"]) and float(g["gap"]) < 1e-5
    assert (got[0] == 0).all() and (got[-1] == 0).all() and (got[:, 0] == 0).all() and (got[:, -1] == 0).all()
    assert np.array_equal(M.bits(M.valid_normal(g["valid"])), M.bits(g["ref_valid"]))
    turn = M.angle_deg(M.point_normals(g["points"], round_f32=False), g["ref_normals"])[1:-1, 1:-1].max()
    print(f"{name}: exact vs reference, largest angle {turn:.2f} degrees")
    if name == "maps_normals_utm":
        assert turn > 5.0
        assert abs(g["points"][..., 0].mean() - 3.7e5) < 1e3 and abs(g["points"][..., 1].mean() - 3.3e6) < 1e3


def test_statement_edges():
    """The statement's own edge rules, on the CPU: the first of tied minima, the first NaN, -inf weights skipped, grid points."""
    z, w, depth = M.tie_case()
    idx = M.surf_idx(z, depth)
    S = z.shape[1]
    assert (idx[1::3] == 0).all() and (idx[2::3] == S - 1).all()
    dev = np.abs(z[0::3] - depth[0::3, None])
    assert ((dev == dev.min(1, keepdims=True)).sum(1) == 2).all()                    # an exact tie between two samples in every such ray
    assert (idx[0::3] == np.array([np.flatnonzero(d == d.min())[0] for d in dev])).all()
    z2 = z.copy()
    z2[0, 7] = z2[0, 3] = np.nan
    assert M.surf_idx(z2, depth)[0] == 3
    w2 = w.copy()
    w2[1, 0] = np.nan
    c = M.counters(M.variance(z, w2, depth)[1], S)
    assert c["std_skipped"] == 1 and c["std_count"] == z.shape[0] - 1
    flat = M.point_normals(M.grid_points(np.zeros((5, 6), np.float32), 0.5), round_f32=False)
    assert (flat[1:-1, 1:-1] == np.array([0, 0, -1], np.float32)).all()               # y grows with the row: left-handed, n_z = -1


def test_abi_declares_the_new_symbols():
    from brdf_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(bn_\w+)\s*\(", header, flags=re.M))
    for name in ("bn_ray_maps", "bn_point_normals"):
        assert name in declared and name in _lib._SIGS and name in _lib.exported_symbols(), name
    assert "#define BN_MAPS_MAX_SAMPLES 4096" in header and _lib.BN_MAPS_MAX_SAMPLES == 4096
    assert "#define BN_MAPS_MAX_CHANNELS 64" in header and _lib.BN_MAPS_MAX_CHANNELS == 64
    assert "additive to ABI 7" in header and _lib.BN_ABI_VERSION == 7
    from brdf_nerf_amd.build import FILE_FLAGS
    assert "-ffp-contract=off" in FILE_FLAGS["view_maps.hip"]
    src = open(os.path.join(ROOT, "brdf_nerf_amd", "csrc", "view_maps.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    assert M.COUNTERS == __import__("brdf_nerf_amd").maps.RAY_MAP_COUNTERS


def test_wrappers_refuse_by_name_before_any_device_work():
    """ValueError / NotImplementedError from the Python layer on host tensors, wrong dtypes and sizes: none of these reaches the
    library (the machine this runs on has no device)."""
    from brdf_nerf_amd import depth_normals, point_normals, ray_maps, view_maps, SceneFrame
    z, w, d = torch.rand(4, 8), torch.rand(4, 8), torch.rand(4)
    X = torch.rand(4, 8, 5)
    for kw, what in ((dict(), "device"), (dict(z_vals=z.double()), "float32"), (dict(weights=w[:, :7]), "shape"),
                     (dict(depth=d[:3]), "shape"), (dict(z_vals=torch.rand(4, 16)[:, ::2]), "contiguous"),
                     (dict(X=X.double()), "float32"), (dict(X=torch.rand(4, 8, 65)), "channels"),
                     (dict(X=X, normal_col=3, view=torch.rand(4, 3)), "normal column"), (dict(X=X, normal_col=-1, view=torch.rand(4, 3)),
                                                                                         "normal column"),
                     (dict(X=X, normal_col=0), "view"), (dict(accumulate=True), "accumulate"),
                     (dict(z_vals=torch.rand(2, 4097), weights=torch.rand(2, 4097), depth=torch.rand(2)), "samples"),
                     (dict(z_vals=torch.rand(2, 0), weights=torch.rand(2, 0), depth=torch.rand(2)), "samples")):
        args = dict(z_vals=z, weights=w, depth=d)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            ray_maps(**args)
    pts = torch.rand(5, 6, 3, dtype=torch.float64)
    for bad, kw, what in ((pts, {}, "device"), (pts.float(), {}, "float64"), (pts[..., :2], {}, "image"), (pts, dict(precision="fast"), "precision"),
                          (pts, dict(valid=torch.rand(5, 5)), "shape")):
        with pytest.raises(ValueError, match=what):
            point_normals(bad, **kw)
    with pytest.raises(ValueError, match="view of 5 x 6"):
        depth_normals(torch.rand(29, 8), torch.rand(29), SceneFrame((0, 0, 0), 1.0), 5, 6)
    with pytest.raises(NotImplementedError, match="ecef"):
        SceneFrame((0, 0, 0), 1.0, cs="ecef")
    rays = torch.rand(30, 11)
    plain = SimpleNamespace(sun_v="none")
    args = SimpleNamespace(sun_v="none", visu_scale=1.0)
    with pytest.raises(NotImplementedError, match="gsam_only"):
        view_maps({"coarse": plain}, args, rays, 5, 6, gsam_only=True)
    with pytest.raises(NotImplementedError, match="sun_v analystic"):
        view_maps({"coarse": SimpleNamespace(sun_v="analystic")}, args, rays, 5, 6)
    with pytest.raises(NotImplementedError, match="visu_scale"):
        view_maps({"coarse": plain}, SimpleNamespace(sun_v="none", visu_scale=2.0), rays, 5, 6)
    with pytest.raises(ValueError, match="30 rays for a view of 5 x 7"):
        view_maps({"coarse": plain}, args, rays, 5, 7)
    with pytest.raises(ValueError, match="cross_rows"):
        view_maps({"coarse": plain}, args, rays, 5, 6, cross_rows=5)
    with pytest.raises(ValueError, match="precision"):
        view_maps({"coarse": plain}, args, rays, 5, 6, precision="fast")
