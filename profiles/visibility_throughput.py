"""Sun shadows and view occlusion of a surface model: what the march costs.  Synthetic urban reliefs of 512 x 512 and 2048 x 2048
cells of 0.5 m (a sloping ground with box buildings of 5 to 40 m), K = 1 / 8 / 64 directions spread over the azimuths at
elevations 15 / 30 / 60 degrees.

(a) by device events: bn_grid_visibility (vis and counts, no hit) - and, with a variant library as the second argument, that
    library's entry alternately in the same process (the recorded profiles/visibility_throughput.txt holds the retired
    tile-max-table form this way; the tree no longer builds it) - and the same march as float64 torch ops on the device, for scale;
(b) whole calls by a host clock: grid_visibility, and score_view with and without sun_dir against render_image on a 512 x 512 view;
(c) the block scene as a view: how many pixels view_visibility classifies differently at eps = 0 and eps = resolution.
Ends with bench.py in a child process as the box-speed indicator of the visit.  Writes profiles/visibility_throughput.txt (or the
path given as the first argument).  Nothing here is a gate."""
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from dsm_throughput import LINES, device_ms, say, timed  # noqa: E402
from brdf_nerf_amd import DsmAccumulator, Grid, SceneFrame, fill_holes, grid_visibility, load_model, score_view, view_visibility  # noqa: E402
from brdf_nerf_amd import _lib as L  # noqa: E402
from brdf_nerf_amd import functions as Fn  # noqa: E402
from brdf_nerf_amd.evaluate import render_image  # noqa: E402

RES = 0.5


def urban(side, seed=0):
    """A ground sloping by 6 m over the scene with side^2 / 4096 box buildings of 5 to 40 m and 10 to 40 cells a side."""
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    dsm = (10.0 + 6.0 * (ii + jj) / (2.0 * side)).astype(np.float32)
    for _ in range(side * side // 4096):
        j, i, h, w = (int(v) for v in rng.integers((0, 0, 10, 10), (side, side, 41, 41)))
        dsm[j:j + h, i:i + w] = dsm[j:j + h, i:i + w].max() + np.float32(rng.uniform(5.0, 40.0))
    return dsm


def dirs_of(K, elevation):
    el = math.radians(elevation)
    az = [math.radians(17.0 + 360.0 * k / K) for k in range(K)]
    return torch.tensor([[math.sin(a) * math.cos(el), math.cos(a) * math.cos(el), math.sin(el)] for a in az], dtype=torch.float64)


def torch_march(dsm, res, d, zmax):
    """The rule as float64 torch ops on the device over all cells at once, one direction: -> vis (H, W) uint8."""
    H, W = dsm.shape
    cells = dsm.double()
    jj, ii = torch.meshgrid(torch.arange(H, device=dsm.device), torch.arange(W, device=dsm.device), indexing="ij")
    u0, v0, z0 = (ii + 0.5).double().reshape(-1), (jj + 0.5).double().reshape(-1), cells.reshape(-1)
    a = max(abs(float(d[0])), abs(float(d[1])))
    su, sv, sz = float(d[0]) / a, -(float(d[1]) / a), (float(d[2]) / a) * res
    vis = torch.where(torch.isfinite(z0), 1, 2).to(torch.uint8)
    live = vis == 1
    for t in range(1, max(W, H) + 1):
        ut, vt, zt = u0 + t * su, v0 + t * sv, z0 + t * sz
        live = live & (ut >= 0) & (ut < W) & (vt >= 0) & (vt < H) & ~(zt > zmax)
        if t % 16 == 0 and not bool(live.any()):
            break
        c = (torch.floor(vt).long().clamp(0, H - 1) * W + torch.floor(ut).long().clamp(0, W - 1))
        hit = live & (cells.reshape(-1)[c] > zt)
        vis[hit] = 0
        live = live & ~hit
    return vis.reshape(H, W)


def main():
    try:
        measure()
    finally:
        out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "visibility_throughput.txt")
        with open(out_path, "w") as f:
            f.write("\n".join(LINES) + "\n")


def measure():
    dev = torch.device("cuda", 0)
    here = L.lib()
    variant = L.load(sys.argv[2], baseline=True) if len(sys.argv) > 2 else None
    say(f"urban relief, 0.5 m cells; device {torch.cuda.get_device_name(0)}" +
        (f"; variant library: {os.path.relpath(sys.argv[2], ROOT)}" if variant else ""))
    with torch.no_grad():
        for side in (512, 2048):
            dsm = torch.from_numpy(urban(side)).to(dev)
            zmax = float(dsm.max())
            for K in (1, 8, 64):
                vis = torch.empty((K, side, side), dtype=torch.uint8, device=dev)
                counts = torch.zeros((K, 3), dtype=torch.int64, device=dev)
                for el in (15, 30, 60):
                    d = dirs_of(K, el)
                    call = lambda: Fn.grid_visibility(dsm, RES, d, 0.0, zmax, vis=vis, counts=counts)
                    reps = 20 if side * side * K <= 1 << 24 else 5
                    best = {"kernel": [], "variant": []}
                    for _ in range(2):                               # alternately, in one process
                        best["kernel"].append(device_ms(call, reps))
                        if variant is not None:
                            prev = L.use(variant)
                            best["variant"].append(device_ms(call, reps))
                            L.use(prev)
                    counts.zero_()
                    call()
                    blocked = int(counts[:, 0].sum())
                    line = f"(a) {side} x {side}, K = {K}, elevation {el}: {100.0 * blocked / (K * side * side):.1f} % blocked"
                    for name, ts in best.items():
                        if ts:
                            lo, med = min(t[0] for t in ts), min(t[1] for t in ts)
                            line += f"; {name} {lo:.3f} ms (median {med:.3f}) = {K * side * side / lo / 1e6:.2f} G starts/s"
                    if K == 1 and side == 512:
                        lo, med = device_ms(lambda: torch_march(dsm, RES, d[0], zmax), 3)
                        same = torch.equal(torch_march(dsm, RES, d[0], zmax), vis[0])
                        line += f"; torch float64 ops {lo:.1f} ms (median {med:.1f}), {'the same bytes' if same else 'DIFFERENT bytes'}"
                    say(line)
                t, t_med = timed(lambda: grid_visibility(dsm, RES, dirs_of(K, 30)), 3)
                say(f"(b) grid_visibility, {side} x {side}, K = {K}, elevation 30, whole call (zmax, launch, counts to the host): "
                    f"{t * 1e3:.2f} ms (median {t_med * 1e3:.2f})")
                del vis
        assert L.lib() is here
        eps_counts(dev)
        score_view_cost(dev)
    say("# for context: the README's figure for shadows.sun_visibility (a --sun_v analystic model's learned visibility) is 47.6 ms per sun "
        "and 512 x 512 view.")
    torch.cuda.empty_cache()
    try:
        run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
        line = [json.loads(s) for s in run.stdout.splitlines() if s.startswith("{")][-1]
        say(f"# box-speed indicator: bench.py in the same visit, same box: {line['value'] / 1e3:.1f} k train rays/s, {line['ms_per_step']:.3f} ms "
            f"per step (BASELINE config 2, bf16).")
    except Exception as e:      # the indicator is a note, not a measurement of this file
        say(f"# box-speed indicator: bench.py did not give a result line ({type(e).__name__})")


def eps_counts(dev):
    """(c) The 64 x 64 block scene (ground 10 m, roof 30 m on [24:40, 24:40]) as a view of 128 x 128 pixels: one surface point per
    pixel, seen straight down, as float32 rays with unit depth; the sun at elevation 30, azimuth 135."""
    frame = SceneFrame((368412.25, 3359871.75, 12.5), 128.0)
    grid = Grid(368412.25 - 16.0, 3359871.75 + 16.0, RES, 64, 64)
    truth = torch.full((64, 64), 10.0, device=dev)
    truth[24:40, 24:40] = 30.0
    n = 128
    jj, ii = torch.meshgrid(torch.arange(n, device=dev), torch.arange(n, device=dev), indexing="ij")
    e = grid.xoff + (ii.reshape(-1).double() + 0.5) * (32.0 / n)
    nn = grid.yoff - (jj.reshape(-1).double() + 0.5) * (32.0 / n)
    alt = truth[(jj.reshape(-1) * 64) // n, (ii.reshape(-1) * 64) // n].double()
    p = (torch.stack([e, nn, alt], -1) - torch.tensor(frame.center, dtype=torch.float64, device=dev)) / frame.range
    down = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64, device=dev)
    rays = torch.cat([p - down, down.expand_as(p), torch.zeros((n * n, 2), dtype=torch.float64, device=dev)], 1).float()
    depth = torch.ones(n * n, device=dev)
    own = DsmAccumulator(grid, dev, 1, "disc").add(rays, depth, frame).result()[0]
    own = fill_holes(own)["filled"] if bool(torch.isnan(own).any()) else own
    el, az = math.radians(30.0), math.radians(135.0)
    sun = torch.tensor([math.sin(az) * math.cos(el), math.cos(az) * math.cos(el), math.sin(el)], dtype=torch.float64)
    for name, raster in (("the true block DSM", truth), ("the view's own DSM (radius 1, disc: edge cells hold means)", own)):
        a = view_visibility(rays, depth, frame, raster, grid, sun, eps=0.0)
        b = view_visibility(rays, depth, frame, raster, grid, sun, eps=RES)
        differ = int((a["visible"] != b["visible"]).sum())
        say(f"(c) block scene as a view of {n} x {n} pixels over {name}, sun (30, 135): eps = 0 blocked {int(a['counts'][0, 0])}, "
            f"eps = {RES} blocked {int(b['counts'][0, 0])}, {differ} pixels classified differently")


def score_view_cost(dev):
    N, side, chunk, config, dtype = 512 * 512, 512, 16384, "rpv_nan", "bf16"
    rays = bench.synthetic_batch(N, 3, dev)["rays"]
    args = bench.make_args(4096, 64, 64, dtype, **bench.CONFIG_FLAGS[config][0])
    torch.manual_seed(0)
    models = {"coarse": load_model(args).to(dev)}
    flags = dict(bench.CONFIG_FLAGS[config][1])
    frame = SceneFrame((368412.25, 3359871.75, 12.5), 128.0)
    rgbs = torch.rand((N, 3), device=dev)
    sun = dirs_of(1, 30)[0]
    t_img, t_img_med = timed(lambda: render_image(models, args, rays, None, keys=("rgb", "depth"), chunk=chunk, **flags), 3)
    say(f"(b) 512 x 512 view, {config} {dtype}, chunk {chunk}: render_image {t_img * 1e3:.1f} ms (median {t_img_med * 1e3:.1f})")
    t0, t0_med = timed(lambda: score_view(models, args, rays, rgbs, side, side, frame=frame, chunk=chunk, **flags), 3)
    t1, t1_med = timed(lambda: score_view(models, args, rays, rgbs, side, side, frame=frame, chunk=chunk, sun_dir=sun, **flags), 3)
    res = score_view(models, args, rays, rgbs, side, side, frame=frame, chunk=chunk, sun_dir=sun, **flags)
    say(f"(b) score_view with a frame {t0 * 1e3:.1f} ms (median {t0_med * 1e3:.1f}); with sun_dir {t1 * 1e3:.1f} ms (median {t1_med * 1e3:.1f}) = "
        f"{(t1 - t0) * 1e3:+.1f} ms (fill_holes of the view's DSM, point_cloud, the march, two masked PSNRs); shadow_fraction "
        f"{res['shadow_fraction']:.3f} on a {res['grid'].width} x {res['grid'].height} grid, source {res['shadow_source']}")


if __name__ == "__main__":
    main()
