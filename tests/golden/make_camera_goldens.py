#!/usr/bin/env python
"""Generate the camera goldens (tests/golden/camera_*.npz) by running the REFERENCE's ray assembly on synthetic RPC images.

Run only where the reference tree is present (BRDFNERF_REFERENCE, default /root/reference, read-only):

    python tests/golden/make_camera_goldens.py

datasets/satellite_rgb_dep.py and sat_utils.py are imported with empty stub modules for rasterio, rpcm, torchvision, cv2,
pytorch3d and the dataset package's own siblings, as the other generators stub their I/O imports.  What runs is upstream's
get_rays, normalize_rays, get_sun_dirs, sat_utils.rescale_rpc, rpc_scaling_params and (cs='ecef') latlon_to_ecef_custom, in the
order load_data and init_scaling_params call them.  What does NOT come from upstream, because its packages are not installed:
  * the camera's .localization is the statement's rule 4 (tests/camera_cases.localize) on a stub object that carries the
    dictionary's attributes, so that rescale_rpc scales it;
  * for cs='utm', sat_utils.utm_from_latlon is replaced by the statement's series (camera_cases.utm) in the fixture's zone.
So the goldens hold the ASSEMBLY to upstream - near and far, the difference, the norm, the float32 cast before the
normalisation, the sun columns, the scaling parameters - and for cs='ecef' the geodesy too; RPC localisation and the UTM series
are not checked against rpcm or pyproj.

CONDITIONS ON THE INPUTS (not tolerances on any code):
  * camera_cases.check_rpc on every view: denominators above 0.5, Newton steps 7 and 8 at most 4 x 2^-52, len > 0;
  * moving every world coordinate that comes out of a transcendental by +1e-6 m or by -1e-6 m changes fewer than 1 element in
    10^4 of the statement's precision='reference' rays of the fixture (the device's sin / cos / atanh differ from numpy's by
    far less than that, so its float32 roundings of the world origins are the statement's);
  * the statement itself equals the reference's rays and scene.loc bit for bit.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import camera_cases as M  # noqa: E402

REF = os.environ.get("BRDFNERF_REFERENCE", "/root/reference")


def load_reference():
    def stub(name, **attrs):
        mod = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(mod, k, v)
        sys.modules[name] = mod
        return mod
    tv = stub("torchvision")
    tv.transforms = stub("torchvision.transforms")
    stub("cv2", COLORMAP_RAINBOW=0, COLORMAP_JET=0)
    stub("rasterio")
    stub("rpcm")
    p3 = stub("pytorch3d")
    p3.transforms = stub("pytorch3d.transforms", axis_angle_to_matrix=None)
    sys.path.insert(0, REF)
    import sat_utils
    pkg = stub("datasets")
    pkg.__path__ = [os.path.join(REF, "datasets")]
    stub("datasets.cal_rmse_depth", cal_rmse_depth=None)
    spec = importlib.util.spec_from_file_location("datasets.satellite_rgb_dep", os.path.join(REF, "datasets", "satellite_rgb_dep.py"))
    ds = importlib.util.module_from_spec(spec)
    sys.modules["datasets.satellite_rgb_dep"] = ds
    spec.loader.exec_module(ds)
    return ds, sat_utils


class StubCamera:
    """The attributes of rpcm.RPCModel that upstream touches, with the statement's localisation."""

    def __init__(self, d):
        self.__dict__.update({k: (list(v) if isinstance(v, list) else v) for k, v in d.items()})

    def localization(self, cols, rows, alts):
        lon, lat, bad = M.localize(self.__dict__, cols, rows, alts)
        assert not bad.any()
        return lon, lat


def run(ds, sat_utils, name):
    site, cs, south, downscale = M.GOLDENS[name]
    zone = M.SITES[site][2]
    views = M.golden_views(name)
    sat_utils.utm_from_latlon = lambda lats, lons: M.utm(lons, lats, zone, south)
    raw, stmt_raw = [], []
    for v in views:
        H, W = v["H"], v["W"]
        rpc = sat_utils.rescale_rpc(StubCamera(v["rpc"]), 1.0 / downscale)
        scaled = M.rescaled(v["rpc"], downscale)
        assert all(getattr(rpc, k) == scaled[k] for k in M.KEYS10)
        M.check_rpc(scaled, H, W, v["min_alt"], v["max_alt"], cs, zone, south)
        cols, rows = np.meshgrid(np.arange(W), np.arange(H))
        raw.append(ds.get_rays(cols.flatten(), rows.flatten(), rpc, v["min_alt"], v["max_alt"], cs=cs))
        c, r = M.grid_pixels(H, W)
        stmt_raw.append(M.rays(scaled, c, r, v["min_alt"], v["max_alt"], cs, zone, south, (0.0, 0.0, 0.0), 1.0)["rays"])
        assert np.array_equal(raw[-1].numpy().view(np.int32), stmt_raw[-1].view(np.int32)), f"{name}: un-normalised rays"
    # init_scaling_params (:251-259)
    all_rays = torch.cat(raw, 0)
    all_points = torch.cat([all_rays[:, :3], all_rays[:, :3] + all_rays[:, 7:8] * all_rays[:, 3:6]], 0)
    loc = {}
    for i, ax in enumerate("XYZ"):
        s, o = sat_utils.rpc_scaling_params(all_points[:, i])
        loc[ax + "_scale"], loc[ax + "_offset"] = float(s), float(o)
    assert loc == M.scene_loc(stmt_raw), f"{name}: scene.loc"
    # the dataset's centre and range (:164-165)
    me = types.SimpleNamespace(center=torch.tensor([loc["X_offset"], loc["Y_offset"], loc["Z_offset"]]),
                               range=torch.max(torch.tensor([loc["X_scale"], loc["Y_scale"], loc["Z_scale"]])))
    center, rng = [float(c) for c in me.center], float(me.range)
    out = {"loc": np.array([loc[k] for k in ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")], np.float64),
           "center": np.array(center, np.float64), "range": np.float64(rng)}
    changed = total = 0
    for i, (v, rays) in enumerate(zip(views, raw)):
        rays = ds.SatelliteRGBDEPDataset.normalize_rays(me, rays.clone())
        sun = ds.SatelliteRGBDEPDataset.get_sun_dirs(me, float(v["sun"][0]), float(v["sun"][1]), rays.shape[0])
        ref = torch.hstack([rays, sun]).type(torch.FloatTensor).numpy()
        scaled = M.rescaled(v["rpc"], downscale)
        c, r = M.grid_pixels(v["H"], v["W"])
        args = (scaled, c, r, v["min_alt"], v["max_alt"], cs, zone, south, center, rng, M.sun_direction(*v["sun"]))
        mine = M.rays(*args)["rays"]
        assert np.array_equal(mine.view(np.int32), ref.view(np.int32)), f"{name}: view {i}: the statement is not the reference"
        for shift in (1e-6, -1e-6):
            changed += int((M.rays(*args, world_shift=shift)["rays"][:, :3].view(np.int32) != mine[:, :3].view(np.int32)).sum())
        total += 2 * mine[:, :3].size
        out[f"rays{i}"] = ref
    assert changed * 10000 < total, f"{name}: a shift of 1e-6 m changes {changed} of {total} origin elements: choose other inputs"
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {cs} zone {zone} south {south} downscale {downscale}: center {center} range {rng:.3f}; 1e-6 m changes {changed} of "
          f"{total} origin elements; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    ds_mod, su = load_reference()
    for fixture in M.GOLDENS:
        run(ds_mod, su, fixture)
