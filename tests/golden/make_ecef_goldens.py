#!/usr/bin/env python
"""Generate tests/golden/ecef.npz by running the REFERENCE's ECEF -> geodetic -> UTM path on synthetic inputs.

Run only where the reference tree is present (BRDFNERF_REFERENCE, default /root/reference, read-only):

    python tests/golden/make_ecef_goldens.py

sat_utils.py and datasets/satellite_rgb_dep.py are imported with the stub modules of make_camera_goldens.py.  What runs is
upstream's sat_utils.ecef_to_latlon_custom, latlon_to_ecef_custom and SatelliteRGBDEPDataset.get_latlonalt_from_nerf_prediction
(cs = 'ecef').  What does NOT come from upstream, because pyproj is not installed: sat_utils.utm_from_latlon is replaced by the
statement's series (camera_cases.utm) in the site's zone, as in make_camera_goldens.py - the UTM series is again NOT checked
against pyproj.

Inputs (tests/ecef_cases.py): the three camera sites - zone 38 N, zone 17 at northing 3.35e6, zone 21 S with both `south`
settings - with 257 rays each and depths between min_alt and max_alt, and 64 free points with |lat| up to 80 degrees and altitudes
from -400 to 9000 m, each in the zone of its longitude.

CONDITIONS ON THE INPUTS (not tolerances on any code), asserted here:
  * p = sqrt(x x + y y) > 1 m and every output finite;
  * moving every ECEF coordinate by one float64 ulp, up or down, moves no output of the statement by more than 1e-7 m (degrees
    at 111,320 m per degree): the device's float64 atan2 / sin / cos differ from numpy's by a few ulps at most;
  * every east and north of the site points lies at least 1e-4 m from a multiple of 0.5 m (ecef_cases.make_site_rays redraws a
    depth until it does; every point is kept), so a 0.5 m raster of the device's points has the statement's counts;
  * upstream's e ** 2, a ** 2 and b ** 2 equal the products e e, a a and b b of the rule.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import camera_cases as M  # noqa: E402
import ecef_cases as E  # noqa: E402
from make_camera_goldens import load_reference  # noqa: E402


def metres(lon, lat, alt, east=None, north=None):
    cols = [lon * E.M_PER_DEG, lat * E.M_PER_DEG, alt] + ([] if east is None else [east, north])
    return np.stack(cols, -1)


def check_inputs(xyz, zone, south, what):
    """The conditions on ECEF points: -> the largest movement of an output under one ulp, in metres."""
    xyz = np.asarray(xyz, np.float64)
    assert (np.sqrt(xyz[:, 0] ** 2 + xyz[:, 1] ** 2) > 1.0).all(), what
    zone = np.broadcast_to(np.asarray(zone), xyz.shape[:1])

    def outputs(p):
        lon, lat, alt, bad = E.ecef_geodetic(p[:, 0], p[:, 1], p[:, 2])
        assert not bad.any(), what
        east, north = np.empty_like(lon), np.empty_like(lon)
        for z in np.unique(zone):
            m = zone == z
            east[m], north[m] = M.utm(lon[m], lat[m], int(z), south)
        out = metres(lon, lat, alt, east, north)
        assert np.isfinite(out).all(), what
        return out
    base = outputs(xyz)
    worst = 0.0
    for toward in (np.inf, -np.inf):
        worst = max(worst, float(np.abs(outputs(np.nextafter(xyz, toward)) - base).max()))
    assert worst <= 1e-7, f"{what}: one ulp moves an output by {worst} m: choose other inputs"
    return worst


def main():
    ds, su = load_reference()
    a, e = 6378137.0, 8.1819190842622e-2
    b = np.sqrt(a ** 2 * (1 - e ** 2))
    assert e ** 2 == e * e and a ** 2 == a * a and b ** 2 == b * b
    out = {}
    for name, (site, south) in E.SITES.items():
        zone = M.SITES[site][2]
        su.utm_from_latlon = lambda lats, lons: M.utm(lons, lats, zone, south)
        center, rng = E.make_site_frame(name)
        rays, depth = E.make_site_rays(name)
        me = types.SimpleNamespace(center=torch.tensor(center, dtype=torch.float32), range=torch.tensor(rng, dtype=torch.float32), cs="ecef")
        assert [float(c) for c in me.center] == list(center) and float(me.range) == rng
        east, north, alt = ds.SatelliteRGBDEPDataset.get_latlonalt_from_nerf_prediction(me, torch.from_numpy(rays.copy()),
                                                                                       torch.from_numpy(depth.copy()))
        p = E.D.points(rays, depth, center, rng)
        lat, lon, alt2 = su.ecef_to_latlon_custom(p[:, 0], p[:, 1], p[:, 2])
        assert np.array_equal(alt, alt2)
        lo, hi = M.alt_bounds(site)
        assert (alt > lo).all() and (alt < hi).all(), f"{name}: altitudes [{alt.min()}, {alt.max()}] outside ({lo}, {hi})"
        assert (E.edge_distance(east) >= E.EDGE_MARGIN).all() and (E.edge_distance(north) >= E.EDGE_MARGIN).all()
        worst = check_inputs(p, zone, south, name)
        stmt = E.surface_points(rays, depth, center, rng, "ecef", zone, south)[0]
        gap = float(np.abs(stmt - np.stack([east, north, alt], -1)).max())
        out.update({name + "_rays": rays, name + "_depth": depth, name + "_center": np.array(center, np.float64),
                    name + "_ref": np.stack([lon, lat, alt, east, north], -1)})
        print(f"{name}: zone {zone} south {south}: one ulp moves an output by at most {worst:.2e} m; statement - upstream at most {gap:.2e} m")
    xyz, zone, lla = E.make_free_points()
    x, y, z = su.latlon_to_ecef_custom(lla[:, 1], lla[:, 0], lla[:, 2])
    assert np.array_equal(np.stack([x, y, z], -1), xyz)
    lat, lon, alt = su.ecef_to_latlon_custom(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    worst = check_inputs(xyz, zone, False, "free points")
    east, north = np.empty_like(lon), np.empty_like(lon)
    for i in range(len(lon)):
        east[i], north[i] = (float(v) for v in M.utm(lon[i], lat[i], int(zone[i]), False))
    out.update(free_xyz=xyz, free_zone=zone.astype(np.int32), free_lla=lla, free_ref=np.stack([lon, lat, alt, east, north], -1))
    print(f"free points: one ulp moves an output by at most {worst:.2e} m")
    path = os.path.join(HERE, "ecef.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
