"""Depth of a surface model along a view's rays: what the walk costs.  A 512 x 512 view of parallel rays over synthetic urban
reliefs of 512 x 512 and 2048 x 2048 cells of 0.5 m (visibility_throughput.urban: a sloping ground with box buildings of 5 to
40 m), the view's pixels aimed at a lattice over the whole raster, at elevations 80 and 45 degrees, azimuth 135.

(a) by device events: bn_cast_rays with nan_cells (every cell of the walk is loaded) and without (cells above zmax are not), depth,
    state and cell written; the classes it counts;
(b) the numpy float64 statement of tests/cast_cases.py on the same rays, by a host clock, and whether the bytes agree;
(c) whole calls by a host clock: cast_rays (zmax, launch, counts to the host) and surface_priors.
Ends with bench.py in a child process as the box-speed indicator of the visit.  Writes profiles/cast_throughput.txt (or the path
given as the first argument).  Nothing here is a gate."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import cast_cases as K  # noqa: E402
from dsm_throughput import LINES, device_ms, say, timed  # noqa: E402
from visibility_throughput import urban  # noqa: E402
from brdf_nerf_amd import Grid, SceneFrame, cast_rays, surface_priors  # noqa: E402
from brdf_nerf_amd import functions as Fn  # noqa: E402

RES, VIEW = 0.5, 512
XOFF, YOFF = 368000.25, 3357000.75


def main():
    try:
        measure()
    finally:
        out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cast_throughput.txt")
        with open(out_path, "w") as f:
            f.write("\n".join(LINES) + "\n")


def measure():
    dev = torch.device("cuda", 0)
    say(f"urban relief, 0.5 m cells, a {VIEW} x {VIEW} view of parallel rays over the whole raster, azimuth 135; device "
        f"{torch.cuda.get_device_name(0)}")
    with torch.no_grad():
        for side in (512, 2048):
            relief = urban(side)
            dsm = torch.from_numpy(relief).to(dev)
            zmax = float(dsm.max())
            center, rng = (XOFF + 0.25 * side, YOFF - 0.25 * side, 20.0), 0.5 * side
            frame, grid = SceneFrame(center, rng), Grid(XOFF, YOFF, RES, side, side)
            step = side * RES / VIEW
            for el in (80.0, 45.0):
                rays_np = K.view(K.lattice(VIEW, XOFF + 0.5 * step, YOFF - 0.5 * step, step), el, 135.0, center, rng, z_ref=10.0,
                                 z_near=zmax + 5.0, z_far=5.0)
                rays = torch.from_numpy(rays_np).to(dev)
                R = rays.shape[0]
                depth = torch.empty((R,), device=dev)
                state = torch.empty((R,), dtype=torch.uint8, device=dev)
                cell = torch.empty((R,), dtype=torch.int32, device=dev)
                nan_cells = torch.empty((R,), dtype=torch.int32, device=dev)
                counts = torch.zeros((5,), dtype=torch.int64, device=dev)
                args = (rays, center, rng, dsm, XOFF, YOFF, RES, zmax)
                full = lambda: Fn.cast_rays(*args, depth=depth, state=state, cell=cell, nan_cells=nan_cells, counts=counts)
                lean = lambda: Fn.cast_rays(*args, depth=depth, state=state, cell=cell, counts=counts, want_nan=False)
                best = {"with nan_cells": [], "without": []}
                for _ in range(2):                                   # alternately, in one process
                    best["with nan_cells"].append(device_ms(full, 20))
                    best["without"].append(device_ms(lean, 20))
                counts.zero_()
                full()
                n = counts.tolist()
                line = f"(a) raster {side} x {side}, elevation {el:g}: top {n[0]}, wall {n[1]}, miss {n[2]}, nodata {n[3]}, below {n[4]}"
                for name, ts in best.items():
                    lo, med = min(t[0] for t in ts), min(t[1] for t in ts)
                    line += f"; kernel {name} {lo:.3f} ms (median {med:.3f}) = {R / lo / 1e3:.1f} M rays/s"
                say(line)
                t0 = time.time()
                want = K.cast_statement(rays_np, center, rng, relief, XOFF, YOFF, RES)
                t_np = time.time() - t0
                same = np.array_equal(depth.cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and \
                    np.array_equal(state.cpu().numpy(), want[1]) and np.array_equal(cell.cpu().numpy(), want[2]) and \
                    np.array_equal(nan_cells.cpu().numpy(), want[3]) and n == want[4].tolist()
                say(f"(b) the numpy statement on the same rays: {t_np:.2f} s on the host, {'the same bytes' if same else 'DIFFERENT bytes'}")
                t, t_med = timed(lambda: cast_rays(rays, frame, dsm, grid), 3)
                say(f"(c) cast_rays, whole call (zmax, launch, counts to the host): {t * 1e3:.2f} ms (median {t_med * 1e3:.2f})")
                t, t_med = timed(lambda: surface_priors(rays, frame, dsm, grid), 3)
                say(f"(c) surface_priors, whole call: {t * 1e3:.2f} ms (median {t_med * 1e3:.2f})")
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
