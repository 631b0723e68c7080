"""ECEF scenes: what the world -> (east, north, altitude) conversion costs.  A 512 x 512 synthetic view (262,144 rays), RPV111 +
analytic normals, bf16, rasterised at 0.5 m with the reference's radius 1, once in a UTM frame and once in the ECEF frame of the
same place (range 128 m: the view at its own ground sampling distance).  (a) by device events: bn_surface_points and
bn_dsm_splat_world with cs = ecef, bn_dsm_splat and bn_dsm_splat_world with cs = utm, and the same conversion stated as float64
torch operations on the device; (b) as whole calls by a host clock: dsm_image on the ECEF frame against the UTM frame.  Ends with
bench.py in a child process as the box-speed indicator of the visit.  Writes profiles/ecef_throughput.txt (or the path given as
the first argument).  Nothing here is a gate."""
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import torch  # noqa: E402
import bench  # noqa: E402
from dsm_throughput import LINES, device_ms, say, timed  # noqa: E402
from brdf_nerf_amd import DsmAccumulator, SceneFrame, dsm_image, load_model, point_cloud  # noqa: E402
from brdf_nerf_amd.camera import geo_world  # noqa: E402
from brdf_nerf_amd.dsm import _cloud_grid  # noqa: E402
from brdf_nerf_amd.evaluate import render_image  # noqa: E402


def torch_conversion(rays, depth, frame):
    """The rule of include/brdfnerf_hip.h ("World points of an ECEF scene") up to the geodetic point as float64 torch operations
    on the device, then bn_geo_world for the UTM series: what a caller without world.hip would write."""
    r = rays.double()
    p = (r[:, 0:3] + r[:, 3:6] * depth.double().reshape(-1, 1)) * frame.range
    p = p + torch.tensor(frame.center, dtype=torch.float64, device=p.device)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    a, e = 6378137.0, 8.1819190842622e-2
    asq, esq = a * a, e * e
    b = math.sqrt(asq * (1 - esq))
    ep = math.sqrt((asq - b * b) / (b * b))
    pp = torch.sqrt(x * x + y * y)
    th = torch.atan2(a * z, b * pp)
    s, c = torch.sin(th), torch.cos(th)
    lon = torch.atan2(y, x)
    lat = torch.atan2(z + ((ep * ep) * b) * ((s * s) * s), pp - (esq * a) * ((c * c) * c))
    sl = torch.sin(lat)
    alt = pp / torch.cos(lat) - a / torch.sqrt(1 - esq * (sl * sl))
    lonlat = torch.stack([lon * 180 / math.pi, lat * 180 / math.pi], -1)
    return geo_world(lonlat, alt, cs="utm", zone=frame.zone, south=frame.south)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ecef_throughput.txt")
    dev = torch.device("cuda", 0)
    N, chunk, config, dtype = 512 * 512, 16384, "rpv_nan", "bf16"
    rays = bench.synthetic_batch(N, 3, dev)["rays"]
    args = bench.make_args(4096, 64, 64, dtype, **bench.CONFIG_FLAGS[config][0])
    torch.manual_seed(0)
    models = {"coarse": load_model(args).to(dev)}
    flags = dict(bench.CONFIG_FLAGS[config][1])
    say(f"view 512 x 512 = {N} rays, {config} {dtype}, S = G = 64, chunk {chunk}; 0.5 m cells, radius 1 (disc), range 128 m; device "
        f"{torch.cuda.get_device_name(0)}")
    utm = SceneFrame((368412.25, 3359871.75, 12.5), 128.0)
    site = geo_world(torch.tensor([[-81.7, 30.3]], dtype=torch.float64), 12.5, cs="ecef", device=dev)[0]      # zone 17
    ecef = SceneFrame.ecef(site.float().tolist(), 128.0)
    with torch.no_grad():
        torch.manual_seed(1)
        depth = render_image(models, args, rays, None, keys=("depth",), chunk=chunk, **flags)["depth"]
        say(f"frames: {utm}; {ecef}")
        res = {}
        for what, frame in (("utm", utm), ("ecef", ecef)):
            grid = _cloud_grid(rays, depth, frame, 0.5)
            acc = DsmAccumulator(grid, dev)

            def splat():
                acc.acc.zero_()
                acc.add(rays, depth, frame)
            zero_ms, _ = device_ms(lambda: acc.acc.zero_())
            splat_ms, _ = device_ms(splat)
            deposits = int(acc.acc[..., 1].sum())
            t_g, t_g_med = timed(lambda: dsm_image(models, args, rays, frame, grid=grid, chunk=chunk, **flags), 3)
            t_c, t_c_med = timed(lambda: dsm_image(models, args, rays, frame, chunk=chunk, **flags), 3)
            res[what] = (splat_ms - zero_ms, t_g, t_c)
            entry = "bn_dsm_splat" if what == "utm" else "bn_dsm_splat_world(cs = ecef)"
            say(f"{what}: grid {grid.width} x {grid.height}, {deposits} deposits, skipped {acc.skipped}; {entry} {splat_ms - zero_ms:.3f} ms "
                f"(with the zeroing of acc {splat_ms:.3f}); dsm_image grid given {t_g * 1e3:.1f} ms (median {t_g_med * 1e3:.1f}), grid from the "
                f"cloud {t_c * 1e3:.1f} ms (median {t_c_med * 1e3:.1f})")
        # the fused launch on the UTM frame: what the ECEF launch costs beyond its conversion
        from brdf_nerf_amd import _lib as L
        from brdf_nerf_amd import functions as Fn
        grid = _cloud_grid(rays, depth, utm, 0.5)
        acc = DsmAccumulator(grid, dev)

        def world_utm():
            acc.acc.zero_()
            Fn.dsm_splat_world(rays, depth, utm.center, utm.range, grid.xoff, grid.yoff, grid.resolution, 1, L.BN_DSM_DISC, L.BN_CS_UTM, 17, 0,
                               acc.acc, acc._skipped)
        zero_ms, _ = device_ms(lambda: acc.acc.zero_())
        wu_ms, _ = device_ms(world_utm)
        sp_ms, sp_med = device_ms(lambda: point_cloud(rays, depth, ecef))
        th_ms, th_med = device_ms(lambda: torch_conversion(rays, depth, ecef), 5)
        gap = float((torch_conversion(rays, depth, ecef) - point_cloud(rays, depth, ecef)).abs().max())
        say(f"bn_dsm_splat_world(cs = utm) {wu_ms - zero_ms:.3f} ms; bn_surface_points(cs = ecef) with its output allocation {sp_ms:.3f} ms "
            f"(median {sp_med:.3f}) = {N / sp_ms / 1e6:.2f} G points/s; the conversion as float64 torch operations + bn_geo_world {th_ms:.3f} ms "
            f"(median {th_med:.3f}) -> {th_ms / sp_ms:.1f} x; max |difference| {gap:.2e} m")
        say(f"the ECEF conversion adds {res['ecef'][0] - res['utm'][0]:+.3f} ms to the splat of the view and {(res['ecef'][1] - res['utm'][1]) * 1e3:+.1f} ms "
            f"to dsm_image with the grid given ({(res['ecef'][2] - res['utm'][2]) * 1e3:+.1f} ms with the grid from the cloud, which converts the "
            f"view twice: once for the bounds)")
    del models
    torch.cuda.empty_cache()
    try:
        run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
        line = [json.loads(s) for s in run.stdout.splitlines() if s.startswith("{")][-1]
        say(f"# box-speed indicator: bench.py in the same visit, same box: {line['value'] / 1e3:.1f} k train rays/s, {line['ms_per_step']:.3f} ms "
            f"per step (BASELINE config 2, bf16).")
    except Exception as e:      # the indicator is a note, not a measurement of this file
        say(f"# box-speed indicator: bench.py did not give a result line ({type(e).__name__})")
    with open(out_path, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
