#!/usr/bin/env python
"""Generate the priors goldens (tests/golden/priors_*.npz) by running the REFERENCE's load_depth_data on synthetic tie points.

Run only where the reference tree is present (BRDFNERF_REFERENCE, default /root/reference, read-only):

    python tests/golden/make_priors_goldens.py

The reference is imported as make_camera_goldens.py imports it (the same load_reference() stubs).  Per fixture a temporary
directory receives the view's JSON and its _2DPts.txt, _3DPts.txt (_3DPts_ecef.txt) and _Correl.txt, and upstream's
SatelliteRGBDEPDataset.load_depth_data itself runs on a namespace that carries the dataset's attributes, normalize_rays and
scale_depth.  What does NOT come from upstream, because its packages are not installed: rpcm.RPCModel is the camera
generator's StubCamera (the statement's localisation), `utm` is a stub that returns the fixture's zone, and for cs='utm'
sat_utils.utm_from_latlon is the statement's series.  So the goldens hold load_depth_data's own work - the pairing, the point
normalisation, the norm, the weights, the std, the padding, the normals - not rpcm or pyproj.

Stored per fixture: the six returned tensors at downscale 1, the inputs' hyper-parameters, and the gap between the normals
statement and upstream's normals.  priors_resize.npz: upstream's scale_depth of an index image for priors_cases.RESIZE_CASES.

CONDITIONS ON THE INPUTS (not tolerances on any code):
  * the tie points are sorted row-major and unique, so upstream's k-th-valid-pixel pairing IS the pixel pairing;
  * at least 100 valid normals per fixture;
  * camera_cases.check_rpc on the view;
  * moving every world coordinate that comes out of a transcendental by +-1e-6 m changes fewer than 1 in 10^4 of the
    origin elements of the statement's tie rays (the camera generator's condition, on these pixels).
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import camera_cases as M  # noqa: E402
import priors_cases as P  # noqa: E402
from make_camera_goldens import StubCamera, load_reference  # noqa: E402

HYPER = {"corrscale": 0.9, "stdscale": 1.0, "margin": 1e-4}


def run(ds, sat_utils, name):
    v, px, (cs, zone, south) = P.golden_ties(name)
    cam = np.load(os.path.join(HERE, P.GOLDENS[name][0] + ".npz"))
    center, rng = cam["center"].tolist(), float(cam["range"])
    H, W, d = v["H"], v["W"], v["rpc"]
    order = np.lexsort((px[:, 0], px[:, 1]))
    assert np.array_equal(order, np.arange(len(px))) and len(np.unique(px[:, 1] * W + px[:, 0])) == len(px), "sorted row-major, unique"
    M.check_rpc(d, H, W, v["min_alt"], v["max_alt"], cs, zone, south)
    cols, rows = px[:, 0].astype(np.float64), px[:, 1].astype(np.float64)
    pts3d, correl = P.world_points(d, cols, rows, v["min_alt"], v["max_alt"], cs, zone, south, P.GOLDENS[name][1])
    args = (d, cols, rows, v["min_alt"], v["max_alt"], cs, zone, south, center, rng)
    tie_rays = M.rays(*args)["rays"]
    changed = sum(int((M.rays(*args, world_shift=s)["rays"][:, :3].view(np.int32) != tie_rays[:, :3].view(np.int32)).sum())
                  for s in (1e-6, -1e-6))
    assert changed * 10000 < 2 * tie_rays[:, :3].size, f"{name}: a shift of 1e-6 m changes {changed} origin elements: choose other inputs"

    sat_utils.utm_from_latlon = lambda lats, lons: M.utm(lons, lats, zone, south)
    ds.rpcm.RPCModel = lambda rpc, dict_format="rpcm": StubCamera(rpc)
    sys.modules["utm"] = types.SimpleNamespace(latlon_to_zone_number=lambda lat, lon: zone, latitude_to_zone_letter=lambda lat: "N")
    cls = ds.SatelliteRGBDEPDataset
    me = types.SimpleNamespace(aoi_id="synthetic", args=types.SimpleNamespace(mod_alt_bound=False), cs=cs, img_downscale=1.0,
                               center=torch.tensor(center), range=torch.tensor(rng), **HYPER)
    me.normalize_rays = types.MethodType(cls.normalize_rays, me)
    me.scale_depth = types.MethodType(cls.scale_depth, me)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = tmp + os.sep
        with open(tmp + "view.json", "w") as f:
            json.dump({"img": "view.tif", "height": H, "width": W, "rpc": d, "min_alt": v["min_alt"], "max_alt": v["max_alt"]}, f)
        np.savetxt(tmp + "view_2DPts.txt", px, fmt="%d")
        np.savetxt(tmp + ("view_3DPts_ecef.txt" if cs == "ecef" else "view_3DPts.txt"), pts3d, fmt="%.3f")
        np.savetxt(tmp + "view_Correl.txt", correl, fmt="%.6f")
        out = cls.load_depth_data(me, [tmp + "view.json"], tmp)
        pts3d = np.loadtxt(tmp + ("view_3DPts_ecef.txt" if cs == "ecef" else "view_3DPts.txt")).reshape(-1, 3)
        correl = np.loadtxt(tmp + "view_Correl.txt")
    rays, depths, valid, std, nrm, vnrm = [t.numpy() for t in out]
    assert rays.shape == (H * W, 8) and depths.shape == (H * W, 2) and int(valid.sum()) == len(px)
    assert int(vnrm.sum()) >= 100, f"{name}: {int(vnrm.sum())} valid normals"
    stmt = P.priors(px, pts3d, correl, tie_rays, H, W, 1.0, center, rng, correl.min(), correl.max(), **HYPER)
    n_stmt, v_stmt = P.normals(stmt, H, W, 1.0)
    gap = float(np.abs(n_stmt.astype(np.float64) - nrm.astype(np.float64)).max())
    drel = np.abs(stmt["depths"][:, 0].astype(np.float64) - depths[:, 0])[valid > 0] / depths[valid > 0, 0]
    path = os.path.join(HERE, name + ".npz")
    # the text files hold 3 and 6 decimals: stored as the integers k with k / 1000.0 and k / 1e6 the very doubles upstream parsed
    pts_mm, cor_u = np.rint(pts3d * 1000.0).astype(np.int64), np.rint(correl * 1e6).astype(np.int32)
    assert np.array_equal(pts_mm / 1000.0, pts3d) and np.array_equal(cor_u / 1e6, correl)
    np.savez_compressed(path, px=px.astype(np.int16), pts3d_mm=pts_mm, correl_u=cor_u, center=np.array(center), range=np.float64(rng),
                        rays=rays, depths=depths, valid_depth=valid, depth_std=std, normals=nrm, valid_normal=vnrm, gap=np.float64(gap),
                        **{k: np.float64(x) for k, x in HYPER.items()})
    print(f"{name}: {cs} zone {zone} south {south}: {len(px)} of {H * W} pixels valid, {int(vnrm.sum())} valid normals, depth_std max "
          f"{np.abs(std).max()}, depth vs the left-to-right rule: {int((drel > 0).sum())} differ, max rel {drel.max():.3e}, normals gap "
          f"{gap:.3e}; {os.path.getsize(path)} bytes")


def resize_cases(ds):
    cls = ds.SatelliteRGBDEPDataset
    out = {}
    for i, (H, W, down) in enumerate(P.RESIZE_CASES):
        me = types.SimpleNamespace(img_downscale=down)
        got = cls.scale_depth(me, torch.arange(H * W, dtype=torch.float32), H, W)
        out[f"case{i}"] = np.atleast_1d(got.numpy()).astype(np.int32)
        out[f"shape{i}"] = np.array([H, W, int(H / down), int(W / down)], np.int32)
        out[f"down{i}"] = np.float64(down)
    path = os.path.join(HERE, "priors_resize.npz")
    np.savez_compressed(path, **out)
    print(f"priors_resize: {len(P.RESIZE_CASES)} cases; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    ds_mod, su = load_reference()
    for fixture in P.GOLDENS:
        run(ds_mod, su, fixture)
    resize_cases(ds_mod)
