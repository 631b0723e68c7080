"""CPU tests of the tie-point depth priors: the numpy statement (tests/priors_cases.py) against the goldens recorded from the
reference's load_depth_data, the resize rule against its scale_depth, and the host side of brdf_nerf_amd/camera.py.  No GPU.

Bounds (none is taken from the code under test):
  depth    5 x 2^-24 relative to upstream's torch.linalg.norm: three squares, two adds and a root, each rounded once, on both
           sides, in an order upstream does not state.  Measured when the goldens were made: at most 1.6e-7 (z38 ecef; 1.2e-7
           on the two utm fixtures), with 261 to 289 of 1,753 values different from the left-to-right rule.
  pad      (T + 1) 2^-24 relative to upstream's float32 mean of T depths (T roundings of its running sum and the division).
  normals  8 x the gap the generator measured between the statement and upstream's float32 chain (the rule of the maps
           goldens).  The gap itself is 3e-5 to 7e-5 here: where a pixel has four valid neighbours and no point of its own its
           four vectors start at the origin and are about 0.015 rad apart, so a float32 rounding of 2^-24 in a unit vector
           turns their cross product by up to 2^-24 / 0.015 = 4e-6 per rounding; the stored gap must stay below 32 such
           roundings (1.3e-4).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import camera_cases as M
import priors_cases as P
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRIES = ("bn_tie_owner", "bn_tie_priors")
DEPTH_REL = 5 * 2.0 ** -24
GAP_MAX = 32 * 2.0 ** -24 / 0.015


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def golden_inputs(name):
    """-> g (the fixture), view, px, pts3d, correl, (cs, zone, south), hyper."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    v, px, world = P.golden_ties(name)
    assert np.array_equal(px, g["px"].astype(np.int64))
    hyper = {k: float(g[k]) for k in ("corrscale", "stdscale", "margin")}
    return g, v, px, g["pts3d_mm"] / 1000.0, g["correl_u"] / 1e6, world, hyper


def check_against_golden(g, got, T, what):
    """got: {"valid_depth", "depth_std", "rays", "depths" (padded), "normals", "valid_normal"} as numpy arrays."""
    valid = g["valid_depth"] > 0
    assert np.array_equal(bits(got["valid_depth"]), bits(g["valid_depth"])), what
    assert np.array_equal(bits(got["valid_normal"]), bits(g["valid_normal"])), what
    assert np.array_equal(bits(got["depth_std"]), bits(g["depth_std"])), what
    assert np.array_equal(bits(got["depths"][:, 1]), bits(g["depths"][:, 1])), what
    ref = g["depths"][:, 0].astype(np.float64)
    rel = np.abs(got["depths"][:, 0].astype(np.float64) - ref) / ref
    print(f"{what}: depth max rel {rel[valid].max():.3e} (bound {DEPTH_REL:.3e}), pad rel {rel[~valid].max():.3e} "
          f"(bound {(T + 1) * 2.0 ** -24:.3e})")
    assert rel[valid].max() <= DEPTH_REL and rel[~valid].max() <= (T + 1) * 2.0 ** -24, what
    gap = np.abs(got["normals"].astype(np.float64) - g["normals"].astype(np.float64)).max()
    print(f"{what}: normals gap {gap:.3e} (stored {float(g['gap']):.3e})")
    assert gap <= 8 * float(g["gap"]) and float(g["gap"]) < GAP_MAX, what
    return rel[valid].max()


@pytest.mark.parametrize("name", sorted(P.GOLDENS))
def test_statement_against_load_depth_data(name):
    g, v, px, pts3d, correl, (cs, zone, south), hyper = golden_inputs(name)
    H, W = v["H"], v["W"]
    center, rng = g["center"].tolist(), float(g["range"])
    tie_rays = M.rays(v["rpc"], px[:, 0].astype(np.float64), px[:, 1].astype(np.float64), v["min_alt"], v["max_alt"], cs, zone, south,
                      center, rng)["rays"]
    res = P.priors(px, pts3d, correl, tie_rays, H, W, 1.0, center, rng, correl.min(), correl.max(), **hyper)
    assert (res["outside"], res["duplicates"], res["skipped"], res["unsampled"], res["kept"]) == (0, 0, 0, 0, len(px))
    assert np.array_equal(bits(res["rays"]), bits(g["rays"])), name
    nrm, vn = P.normals(res, H, W, 1.0)
    got = {"valid_depth": res["valid"], "depth_std": res["depth_std"], "depths": P.padded(res), "normals": nrm, "valid_normal": vn}
    check_against_golden(g, got, len(px), name)
    assert int(g["valid_normal"].sum()) >= 100 and not g["depth_std"].any()


def test_nearest_lines_equals_scale_depth():
    """Every stored scale_depth of an index image: output pixel (i, j) holds src_rows[i] W + src_cols[j]."""
    from brdf_nerf_amd.camera import nearest_lines
    g = np.load(os.path.join(GOLDEN, "priors_resize.npz"))
    for i, (H, W, down) in enumerate(P.RESIZE_CASES):
        assert g[f"shape{i}"].tolist()[:2] == [H, W] and float(g[f"down{i}"]) == down
        Hout, src_r, _ = nearest_lines(H, down)
        Wout, src_c, _ = nearest_lines(W, down)
        assert [Hout, Wout] == g[f"shape{i}"].tolist()[2:], (H, W, down)
        assert np.array_equal((src_r[:, None] * W + src_c[None, :]).ravel(), g[f"case{i}"].astype(np.int64)), (H, W, down)
        assert (Hout, src_r.tolist()) == P.nearest_src(H, down) and (Wout, src_c.tolist()) == P.nearest_src(W, down)
    # 1000 -> 666 is where a float64 scale samples another line than torch's float32 one
    _, src, _ = nearest_lines(1000, 1.5)
    f64 = np.minimum(np.floor(np.arange(666) * (1000 / 666)).astype(np.int64), 999)
    assert not np.array_equal(src, f64)


def test_nearest_lines_src_and_dst_are_inverse():
    from brdf_nerf_amd.camera import nearest_lines
    for n in list(range(1, 70)) + [255, 256, 257, 511, 512, 513, 1000, 1024, 2047, 2048]:
        for down in (1, 1.5, 2, 2.5, 3, 4, 7):
            if int(n / down) < 1:
                with pytest.raises(ValueError, match="leave none"):
                    nearest_lines(n, down)
                continue
            n_out, src, dst = nearest_lines(n, down)
            assert n_out == int(n / down) == len(src) and len(dst) == n and src.dtype == np.int64 and dst.dtype == np.int32
            assert (np.diff(src) > 0).all() and 0 <= src[0] and src[-1] < n
            assert np.array_equal(dst[src], np.arange(n_out)) and int((dst >= 0).sum()) == n_out
            assert np.array_equal(np.flatnonzero(dst >= 0), src)
            if down == 1:
                assert np.array_equal(src, np.arange(n))


def test_nearest_lines_against_torch_interpolate():
    """The rule on the 5-D shape scale_depth uses, here: a few sizes around the float32 / float64 split."""
    from brdf_nerf_amd.camera import nearest_lines
    for n, down in ((1000, 1.5), (999, 1.5), (2047, 2.5), (513, 7), (69, 4)):
        n_out, src, _ = nearest_lines(n, down)
        ref = torch.nn.functional.interpolate(torch.arange(n, dtype=torch.float32).reshape(1, 1, 1, n, 1), size=(1, n_out, 1))
        assert np.array_equal(ref.reshape(-1).numpy().astype(np.int64), src), (n, down)


def test_entries_are_declared_bound_and_exported():
    import brdf_nerf_amd
    from brdf_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    declared = set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", header))
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _lib._SIGS and hasattr(raw, name), name
    assert _lib.lib().bn_abi_version() == 7
    for name in ("depth_priors", "nearest_lines"):
        assert name in brdf_nerf_amd.__all__ and hasattr(brdf_nerf_amd, name), name


def test_host_layer_refusals():
    """Every refusal of depth_priors / tie_priors / nearest_lines is a ValueError raised before a device is touched."""
    from brdf_nerf_amd.camera import Rpc, depth_priors, nearest_lines, ray_table, tie_priors
    rpc = Rpc.from_dict(M.make_rpc("z38", 3))
    px, pts, cor = np.array([[1, 2], [3, 4]]), np.zeros((2, 3)), np.array([0.25, 0.75])

    def call(pts2d=px, pts3d=pts, correl=cor, H=9, W=11, lo=0.0, hi=10.0, center=(0.0, 0.0, 0.0), rng=1.0, **kw):
        return depth_priors(rpc, H, W, pts2d, pts3d, correl, lo, hi, center, rng, device="cpu", **dict(dict(zone=38), **kw))

    cases = [(dict(pts2d=px.astype(np.float64)), "integer"), (dict(pts2d=np.zeros((2, 3), np.int64)), r"\(T, 2\)"),
             (dict(pts3d=np.zeros((3, 3))), "points"), (dict(correl=np.zeros(3)), "correlations"),
             (dict(correl=np.array([0.5, 0.5])), "not all equal"), (dict(correl=np.array([0.5, np.nan])), "finite"),
             (dict(correl=np.array([0.5, np.inf])), "finite"), (dict(pts2d=np.zeros((0, 2), np.int64), pts3d=np.zeros((0, 3)),
                                                                      correl=np.zeros(0)), "no tie points"),
             (dict(H=0), "pixels"), (dict(W=-1), "pixels"), (dict(H=1 << 16, W=1 << 15), "pixels"), (dict(lo=np.nan), "min_alt"),
             (dict(hi=np.inf), "max_alt"), (dict(rng=0.0), "range"), (dict(rng=np.nan), "range"), (dict(center=(0.0, np.nan, 0.0)), "center"),
             (dict(cs="wgs"), "coordinate system"), (dict(zone=0), "zone"), (dict(zone=61), "zone"), (dict(precision="fast"), "precision"),
             (dict(downscale=0.5), "downscale"), (dict(downscale=np.nan), "downscale"), (dict(downscale=np.inf), "downscale"),
             (dict(downscale=12.0), "leave none"), (dict(corrscale=np.nan), "corrscale"), (dict(stdscale=np.inf), "stdscale"),
             (dict(margin=np.nan), "margin"), (dict(std_span=np.nan), "std_span")]
    for kw, match in cases:
        with pytest.raises(ValueError, match=match):
            call(**kw)
    for cmin, cmax in ((0.5, 0.5), (0.75, 0.25), (np.nan, 1.0), (0.0, np.inf)):
        with pytest.raises(ValueError, match="cmin|cmax"):
            tie_priors(rpc, 9, 11, px, pts, cor, cmin, cmax, 0.0, 10.0, (0.0, 0.0, 0.0), 1.0, zone=38, device="cpu")
    for n, down in ((0, 1.0), ((1 << 24) + 1, 1.0), (5, 0.99), (5, float("nan"))):
        with pytest.raises(ValueError, match="nearest_lines"):
            nearest_lines(n, down)
    view = {"rpc": rpc, "H": 9, "W": 11, "min_alt": 0.0, "max_alt": 10.0, "sun": M.SUN}
    with pytest.raises(ValueError, match="1 views and 2 priors"):
        ray_table([view], [torch.zeros(99, 3)], (0.0, 0.0, 0.0), 1.0, zone=38, device="cpu", priors=[None, None])


def test_library_refuses_bad_arguments_without_a_launch():
    """BN_EINVAL before anything touches a device, with a named message."""
    from brdf_nerf_amd import _lib
    from brdf_nerf_amd.camera import Rpc
    lib = _lib.lib()
    rpc = Rpc.from_dict(M.make_rpc("z38", 3))
    bad = Rpc.from_dict(M.make_rpc("z38", 3))
    bad.struct.col_scale = 0.0
    p = C.c_void_p(4096)                                     # never dereferenced: every call below is refused on the host
    c3, nan_c = (C.c_double * 3)(0.0, 0.0, 0.0), (C.c_double * 3)(0.0, 0.0, float("nan"))
    nan, inf = float("nan"), float("inf")

    def owner(px=p, T=4, H=9, W=11, own=p, counts=p):
        return lib.bn_tie_owner(px, T, H, W, own, counts, None)

    for kw in (dict(px=None), dict(own=None), dict(counts=None), dict(T=-1), dict(T=(1 << 30) + 1), dict(H=0), dict(W=0),
               dict(H=1 << 16, W=(1 << 15) + 1)):
        assert owner(**kw) == -1 and b"tie_owner" in lib.bn_last_error(), kw
    assert owner(T=0) == 0

    def priors(rpc_ref=rpc.ref(), px=p, own=p, pts=p, cor=p, T=4, H=9, W=11, Hout=9, Wout=11, dr=None, dc=None, down=1.0, lo=0.0, hi=10.0,
               cs=_lib.BN_CS_UTM, zone=38, south=0, center=c3, rng=1.0, f32=1, cmin=0.0, cmax=1.0, corrscale=1.0, stdscale=1.0, margin=0.0,
               span=0.0, valid=p, counts=p):
        return lib.bn_tie_priors(rpc_ref, px, own, pts, cor, T, H, W, Hout, Wout, dr, dc, down, lo, hi, cs, zone, south, center, rng, f32,
                                 cmin, cmax, corrscale, stdscale, margin, span, valid, None, None, None, None, None, None, counts, None)

    cases = [dict(rpc_ref=None), dict(px=None), dict(own=None), dict(pts=None), dict(cor=None), dict(center=None), dict(valid=None),
             dict(counts=None), dict(T=-1), dict(T=(1 << 30) + 1), dict(H=0), dict(W=0), dict(Hout=0, dr=p), dict(Wout=0, dc=p),
             dict(H=1 << 16, W=(1 << 15) + 1, Hout=1, Wout=1, dr=p, dc=p), dict(Hout=4), dict(Wout=5), dict(down=nan), dict(down=inf),
             dict(down=0.5), dict(rng=0.0), dict(rng=nan), dict(rng=inf), dict(cmin=nan), dict(cmax=inf), dict(cmin=1.0, cmax=1.0),
             dict(cmin=1.0, cmax=0.5), dict(corrscale=nan), dict(stdscale=inf), dict(margin=nan), dict(span=inf), dict(cs=2), dict(zone=0),
             dict(zone=61), dict(south=2), dict(f32=2), dict(lo=nan), dict(hi=inf), dict(center=nan_c), dict(rpc_ref=bad.ref())]
    for kw in cases:
        assert priors(**kw) == -1 and b"tie_priors" in lib.bn_last_error(), kw
    assert priors(T=0) == 0
