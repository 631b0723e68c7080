"""DSM throughput: a 512 x 512 synthetic view (262,144 rays), RPV111 + analytic normals, bf16, rasterised at 0.5 m with the
reference's radius 1.  (a) render_image alone; (b) dsm_image, with the grid taken from the cloud and with the grid given (each
chunk splatted as it is rendered); (c) the two launches alone (bn_dsm_splat of the whole view, bn_dsm_resolve) by device events;
(d) the same rasterisation stated in torch on the device: float64 index_put_(accumulate=True) per footprint cell.  Two scene
scales: range 128 m - the view at its own ground sampling distance, about one ray per 0.5 m cell, the real workload - and range
6 m, hundreds of rays per cell (contention).  Ends with bench.py in a child process as the box-speed indicator of the visit.
Writes profiles/dsm_throughput.txt (or the path given as the first argument).  Nothing here is a gate."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from brdf_nerf_amd import DsmAccumulator, SceneFrame, dsm_image, load_model, point_cloud  # noqa: E402
from brdf_nerf_amd.dsm import _cloud_grid  # noqa: E402
from brdf_nerf_amd.evaluate import render_image  # noqa: E402

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        ts.append(time.time() - t0)
    return min(ts), sorted(ts)[len(ts) // 2]


def device_ms(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return ts[0], ts[len(ts) // 2]


def torch_statement(rays, depth, frame, grid, radius=1):
    """The rasteriser in torch on the device: float64 sums by index_put_(accumulate=True), one call per footprint cell (disc)."""
    p = point_cloud(rays, depth, frame)
    ok = torch.isfinite(p).all(-1) & (p[:, 2].abs() < 2.0 ** 23)
    p = p[ok]
    i = torch.floor((p[:, 0] - grid.xoff) / grid.resolution).long()
    j = torch.floor((grid.yoff - p[:, 1]) / grid.resolution).long()
    sums = torch.zeros((grid.height, grid.width), dtype=torch.float64, device=rays.device)
    counts = torch.zeros((grid.height, grid.width), dtype=torch.float64, device=rays.device)
    one = torch.ones_like(p[:, 2])
    for k2 in range(-radius, radius + 1):
        for k1 in range(-radius, radius + 1):
            if k1 * k1 + k2 * k2 > radius * radius:
                continue
            row, col = j + k2, i + k1
            m = (row >= 0) & (row < grid.height) & (col >= 0) & (col < grid.width)
            sums.index_put_((row[m], col[m]), p[m, 2], accumulate=True)
            counts.index_put_((row[m], col[m]), one[m], accumulate=True)
    return (sums / counts).float(), counts


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dsm_throughput.txt")
    dev = torch.device("cuda", 0)
    N, chunk, config, dtype = 512 * 512, 16384, "rpv_nan", "bf16"
    rays = bench.synthetic_batch(N, 3, dev)["rays"]
    args = bench.make_args(4096, 64, 64, dtype, **bench.CONFIG_FLAGS[config][0])
    torch.manual_seed(0)
    models = {"coarse": load_model(args).to(dev)}
    flags = dict(bench.CONFIG_FLAGS[config][1])
    say(f"view 512 x 512 = {N} rays, {config} {dtype}, S = G = 64, chunk {chunk}; 0.5 m cells, radius 1 (disc); device {torch.cuda.get_device_name(0)}")
    with torch.no_grad():
        t_img, t_img_med = timed(lambda: render_image(models, args, rays, None, keys=("rgb", "depth"), chunk=chunk, **flags), 3)
        say(f"(a) render_image: {t_img * 1e3:.1f} ms (median {t_img_med * 1e3:.1f}) = {N / t_img / 1e3:.0f} k rays/s")
        torch.manual_seed(1)
        depth = render_image(models, args, rays, None, keys=("depth",), chunk=chunk, **flags)["depth"]
        for rng, what in ((128.0, "own ground sampling distance"), (6.0, "contended")):
            frame = SceneFrame((368412.25, 3359871.75, 12.5), rng)
            grid = _cloud_grid(rays, depth, frame, 0.5)
            t_c, t_c_med = timed(lambda: dsm_image(models, args, rays, frame, chunk=chunk, **flags), 3)
            t_g, t_g_med = timed(lambda: dsm_image(models, args, rays, frame, grid=grid, chunk=chunk, **flags), 3)
            acc = DsmAccumulator(grid, dev)

            def splat():
                acc.acc.zero_()
                acc.add(rays, depth, frame)
            zero_ms, _ = device_ms(lambda: acc.acc.zero_())
            splat_ms, splat_med = device_ms(splat)
            res_ms, res_med = device_ms(acc.result)
            dsm, count = acc.result()
            deposits, cells = int(acc.acc[..., 1].sum()), grid.width * grid.height
            th_ms, th_med = device_ms(lambda: torch_statement(rays, depth, frame, grid), 5)
            t_dsm, t_cnt = torch_statement(rays, depth, frame, grid)
            same = bool((t_cnt.long() == count.long()).all())
            err = float((t_dsm - dsm)[count > 0].abs().max())
            say(f"range {rng:g} m ({what}): grid {grid.width} x {grid.height} = {cells} cells, {deposits} deposits, at most {int(count.max())} per cell, "
                f"{int((count == 0).sum())} cells empty, skipped {acc.skipped}")
            say(f"  (b) dsm_image, grid from the cloud {t_c * 1e3:.1f} ms (median {t_c_med * 1e3:.1f}); grid given {t_g * 1e3:.1f} ms (median "
                f"{t_g_med * 1e3:.1f}) -> {(t_g - t_img) * 1e3:+.1f} ms on render_image")
            say(f"  (c) bn_dsm_splat {splat_ms - zero_ms:.3f} ms (with the zeroing of acc {splat_ms:.3f}, median {splat_med:.3f}; zeroing {zero_ms:.3f}) = "
                f"{deposits / max(splat_ms - zero_ms, 1e-6) / 1e6:.2f} G deposits/s ({2 * deposits} 8-byte atomics); bn_dsm_resolve {res_ms:.3f} ms "
                f"(median {res_med:.3f}) for {cells * 16 / 1e6:.1f} MB read")
            say(f"  (d) torch float64 index_put_ per footprint cell {th_ms:.3f} ms (median {th_med:.3f}) -> {th_ms / (splat_ms + res_ms):.1f} x "
                f"splat + resolve; counts equal {same}, max |dsm difference| {err:.2e} m")
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
