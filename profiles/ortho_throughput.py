"""Orthorectified maps: what the two passes and the resolve cost.  A
512 x 512 synthetic view (262,144 rays), RPV111 + analytic normals, bf16, 0.5 m cells, radius 1 (disc), range 128 m (the view at
its own ground sampling distance), E = 3 and E = 28 random feature channels, mean and top mode (band 0.5 m).

(a) by device events: bn_ortho_top, bn_ortho_splat and bn_ortho_resolve (the recorded
    profiles/ortho_throughput.txt also holds the retired lane-per-ray form of the splat, which this script no longer builds)
    and the same rasterisation as float64 index_put_(accumulate=True) in torch; all rays on a 25 x 27 grid as the contention case;
(b) as whole calls by a host clock: ortho_image against view_maps.
Ends with bench.py in a child process as the box-speed indicator of the visit.  Writes profiles/ortho_throughput.txt (or the path
given as the first argument).  Nothing here is a gate."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import torch  # noqa: E402
import bench  # noqa: E402
from dsm_throughput import LINES, device_ms, say, timed  # noqa: E402
from brdf_nerf_amd import Grid, OrthoAccumulator, SceneFrame, load_model, ortho_image, point_cloud, view_maps  # noqa: E402
from brdf_nerf_amd import functions as Fn  # noqa: E402
from brdf_nerf_amd.dsm import _cloud_grid  # noqa: E402
from brdf_nerf_amd.evaluate import render_image  # noqa: E402


def torch_rasteriser(rays, depth, features, frame, grid, radius=1):
    """Mean mode in torch on the device: float64 sums by index_put_(accumulate=True), one call per footprint cell (disc)."""
    p = point_cloud(rays, depth, frame)
    ok = torch.isfinite(p).all(-1) & (p[:, 2].abs() < 2.0 ** 23)
    p, x = p[ok], features[ok].double()
    i = torch.floor((p[:, 0] - grid.xoff) / grid.resolution).long()
    j = torch.floor((grid.yoff - p[:, 1]) / grid.resolution).long()
    rows = torch.cat([p[:, 2:3], torch.ones_like(p[:, 2:3]), x], 1)
    sums = torch.zeros((grid.height, grid.width, rows.shape[1]), dtype=torch.float64, device=rays.device)
    for k2 in range(-radius, radius + 1):
        for k1 in range(-radius, radius + 1):
            if k1 * k1 + k2 * k2 > radius * radius:
                continue
            row, col = j + k2, i + k1
            m = (row >= 0) & (row < grid.height) & (col >= 0) & (col < grid.width)
            sums.index_put_((row[m], col[m]), rows[m], accumulate=True)
    return (sums[..., 2:] / sums[..., 1:2]).float()


def main():
    try:
        measure()
    finally:
        out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ortho_throughput.txt")
        with open(out_path, "w") as f:
            f.write("\n".join(LINES) + "\n")


def measure():
    dev = torch.device("cuda", 0)
    N, side, chunk, config, dtype = 512 * 512, 512, 16384, "rpv_nan", "bf16"
    rays = bench.synthetic_batch(N, 3, dev)["rays"]
    args = bench.make_args(4096, 64, 64, dtype, **bench.CONFIG_FLAGS[config][0])
    torch.manual_seed(0)
    models = {"coarse": load_model(args).to(dev)}
    flags = dict(bench.CONFIG_FLAGS[config][1])
    say(f"view 512 x 512 = {N} rays, {config} {dtype}, S = G = 64, chunk {chunk}; 0.5 m cells, radius 1 (disc), range 128 m, band 0.5 m; "
        f"device {torch.cuda.get_device_name(0)}")
    frame = SceneFrame((368412.25, 3359871.75, 12.5), 128.0)
    with torch.no_grad():
        torch.manual_seed(1)
        depth = render_image(models, args, rays, None, keys=("depth",), chunk=chunk, **flags)["depth"]
        view = _cloud_grid(rays, depth, frame, 0.5)
        xy = point_cloud(rays, depth, frame)[:, :2]
        (x0, y0), (x1, y1) = xy.min(0).values.tolist(), xy.max(0).values.tolist()
        res = max((x1 - x0) / 24.5, (y1 - y0) / 26.5)
        tight = Grid(x0 - 0.25 * res, y1 + 0.25 * res, res, 25, 27)
        g = torch.Generator(device=dev).manual_seed(2)
        for E in (3, 28):
            feats = torch.rand((N, E), generator=g, device=dev) * 2 - 0.5
            for gname, grid in (("view", view), ("25 x 27", tight)):
                for mode in ("mean", "top"):
                    acc = OrthoAccumulator(grid, dev, E, mode=mode, band=0.5)
                    if mode == "top":
                        acc.add_top(rays, depth, frame)
                    zero_ms = device_ms(lambda: acc.acc.zero_())[0]

                    def splat():
                        acc.acc.zero_()
                        acc.add(rays, depth, frame, feats)
                    fns = {"splat": splat}
                    if mode == "top":
                        # (a max is idempotent: no refill needed; the entry itself, since add_top is refused once add has run)
                        fns["top"] = lambda: Fn.ortho_top(rays, depth, *acc._args(frame), acc.top, acc._top_skipped)
                    fns["resolve"] = acc.result
                    if mode == "mean":
                        fns["torch index_put_ float64"] = lambda: torch_rasteriser(rays, depth, feats, frame, grid)
                    ts = {name: device_ms(fn) for name, fn in fns.items()}
                    acc._counters.zero_()
                    splat()
                    deposits, culled = int(acc.acc[..., 1].sum()), acc.culled
                    line = f"E = {E}, grid {gname} ({grid.width} x {grid.height}), {mode}: {deposits} deposits, {culled} culled, acc zeroing {zero_ms:.3f} ms"
                    for name, (lo, med) in ts.items():
                        lo, med = (lo - zero_ms, med - zero_ms) if name.startswith("splat") else (lo, med)
                        line += f"; {name} {lo:.3f} ms (median {med:.3f})"
                    if mode == "mean" and gname == "view":
                        gap = (torch_rasteriser(rays, depth, feats, frame, grid) - acc.result()[0].permute(1, 2, 0))
                        line += f"; max |torch - maps| {float(gap[torch.isfinite(gap)].abs().max()):.2e}"
                    say(line)
        H = W = side
        vm = view_maps(models, args, rays, H, W, chunk=chunk, **flags)["maps"]
        keys3, keys28, n = ("rgb",), [], 0
        for k, t in vm.items():                                  # the view's float32 maps in their order, up to 28 channels
            d = t.reshape(N, -1).shape[1]
            if t.dtype == torch.float32 and k != "depth" and n + d <= 28:
                keys28.append(k)
                n += d
        del vm
        say(f"(b) the {n} channels: {', '.join(keys28)}")
        t_vm, t_vm_med = timed(lambda: view_maps(models, args, rays, H, W, chunk=chunk, **flags), 3)
        say(f"(b) view_maps: {t_vm * 1e3:.1f} ms (median {t_vm_med * 1e3:.1f})")
        for keys in (keys3, keys28):
            for mode in ("mean", "top"):
                t, t_med = timed(lambda: ortho_image(models, args, rays, H, W, frame, grid=view, keys=keys, mode=mode, chunk=chunk, **flags), 3)
                out = ortho_image(models, args, rays, H, W, frame, grid=view, keys=keys, mode=mode, chunk=chunk, **flags)
                E = sum(d for _, d in out["channels"].values())
                say(f"(b) ortho_image, {E} channels, {mode}: {t * 1e3:.1f} ms (median {t_med * 1e3:.1f}) = view_maps {(t - t_vm) * 1e3:+.1f} ms; "
                    f"culled {out['culled']}, bad features {out['bad_features']}")
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


if __name__ == "__main__":
    main()
