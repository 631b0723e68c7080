"""The altitude sweep of a DSM under several observed images: what the fused launch costs, and what it saves.  The relief, the images
and the cameras of mosaic_throughput.py - urban reliefs of 512 x 512 and 2048 x 2048 cells of 0.5 m, 2048 x 2048 x 3 images of some
0.5 m per pixel, K = 3 / 20 cameras some 25 degrees off nadir - under Z = 17 / 65 offsets of 0.5 m around the relief, both modes.

(a) by device events: bn_grid_sweep with the K occlusion masks of the base relief (no cost volume);
(b) whole calls by a host clock, alternately in one process: altitude_sweep with view_dirs given, against what the parent commit
    offers for the same answer - Z calls of orthomosaic on dsm + off (each with its own march) plus the torch argmin over the
    stacked sum of the squared std, valid where count >= 2; the share of cells at which the two choose the same level;
(c) with --resources (no GPU needed): VGPRs, scratch, LDS and waves per SIMD of grid_sweep_kernel<C> as the compiler reports them.
Ends with bench.py in a child process as the box-speed indicator of the visit.  Writes profiles/sweep_throughput.txt (or the path
given as the first argument; --resources appends to it).  Nothing here is a gate."""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

VIEWS, LEVELS, STEP = (3, 20), (17, 65), 0.5
FLOPS_PER_PROJECTION = 330               # four 20-term polynomials, uncontracted float64


def resources(out_path):
    from brdf_nerf_amd import build as B
    with tempfile.TemporaryDirectory() as tmp:
        cmd = B.compile_command(os.path.join(B.CSRC, "sweep.hip"), os.path.join(tmp, "sweep.s"), asm=True)
        log = subprocess.run(cmd + ["-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    rows, got = [], None
    for l in log.splitlines():
        m = re.search(r"Function Name: \S*grid_sweep_kernelILi(\d)E", l)
        if m:
            got = {"C": m.group(1)}
            rows.append(got)
        for key, tag in (("VGPRs", " VGPRs:"), ("scratch", "ScratchSize [bytes/lane]:"), ("LDS", "LDS Size [bytes/block]:"),
                         ("waves", "Occupancy [waves/SIMD]:"), ("sgpr_spill", "SGPRs Spill:")):
            if got is not None and tag in l:
                got[key] = l.split(tag)[1].split()[0]
    with open(out_path, "a") as f:
        for got in rows:
            s = f"(c) grid_sweep_kernel<{got['C']}>: {got.get('VGPRs')} VGPRs, {got.get('scratch')} B of scratch per lane, {got.get('LDS')} B of " \
                f"LDS, {got.get('waves')} waves per SIMD, {got.get('sgpr_spill')} SGPRs held in VGPR lanes (gfx950, as the compiler reports them)"
            print(s)
            f.write(s + "\n")


def alternately(first, second, reps):
    """first and second timed in turn by a host clock, reps times after one warm-up each -> (min, median) of each, seconds."""
    import torch
    ts = ([], [])
    for r in range(reps + 1):
        for which, fn in enumerate((first, second)):
            torch.cuda.synchronize()
            t0 = time.time()
            fn()
            torch.cuda.synchronize()
            if r:
                ts[which].append(time.time() - t0)
    return [(min(t), sorted(t)[len(t) // 2]) for t in ts]


def measure():
    import numpy as np
    import torch
    import orthophoto_cases as O
    from dsm_throughput import device_ms, say
    from mosaic_throughput import cameras
    from orthophoto_throughput import IMAGE, RES, ZONE
    from visibility_throughput import urban
    from brdf_nerf_amd import Grid, Rpc, altitude_sweep, camera, orthomosaic
    from brdf_nerf_amd import functions as Fn
    from brdf_nerf_amd.visibility import _zmax
    dev = torch.device("cuda", 0)
    say(f"urban relief, 0.5 m cells, zone {ZONE} north; K images of {IMAGE} x {IMAGE} x 3 float32 each; offsets of {STEP} m around the relief; "
        f"device {torch.cuda.get_device_name(0)}")
    torch.manual_seed(0)
    strides = (IMAGE * 3, 3, 1)
    images = [torch.rand((IMAGE * IMAGE, 3), device=dev) for _ in range(max(VIEWS))]
    with torch.no_grad():
        for side in (512, 2048):
            relief = urban(side)
            xoff, yoff = O.site_grid("z17", side, side, RES)
            grid = Grid(xoff, yoff, RES, side, side)
            dsm = torch.from_numpy(relief).to(dev)
            n = side * side
            lo_alt, hi_alt = float(np.nanmin(relief)), float(np.nanmax(relief))
            for K in VIEWS:
                rpcs = [Rpc.from_dict(d) for d in cameras(K)]
                dirs = torch.stack([torch.as_tensor(camera.view_direction(r, ZONE, False, lo_alt, hi_alt, device=dev)) for r in rpcs])
                views = [(images[k], IMAGE, IMAGE, rpcs[k]) for k in range(K)]
                visible, _, _ = Fn.grid_visibility(dsm, RES, dirs, 0.0, _zmax(dsm))
                table = [(images[k], IMAGE, IMAGE, strides, visible[k], 0, rpcs[k]) for k in range(K)]
                for Z in LEVELS:
                    offsets = (np.arange(Z) - Z // 2) * STEP
                    for mode in ("bilinear", "nearest"):
                        outs = dict(level=torch.empty((side, side), dtype=torch.int32, device=dev), cost_min=torch.empty((side, side), device=dev),
                                    count=torch.empty((side, side), dtype=torch.uint8, device=dev), altitude=torch.empty((side, side), device=dev),
                                    valid=torch.zeros(Z, dtype=torch.int64, device=dev), wins=torch.zeros(Z, dtype=torch.int64, device=dev),
                                    sums=torch.zeros(3, dtype=torch.int64, device=dev))
                        lo, med = device_ms(lambda: Fn.grid_sweep(table, 3, dsm, xoff, yoff, RES, ZONE, 0, offsets, mode=mode, **outs), 5)
                        proj = n * K * Z
                        say(f"(a) {side} x {side}, K = {K}, Z = {Z}, {mode}: bn_grid_sweep {lo:.3f} ms (median {med:.3f}) = {proj / lo / 1e6:.2f} G "
                            f"projections/s, some {proj * FLOPS_PER_PROJECTION / lo / 1e9:.1f} TFLOP/s of float64 in the polynomials alone")
                        got = {}

                        def fused():
                            got["sweep"] = altitude_sweep(views, dsm, grid, ZONE, offsets, view_dirs=dirs, mode=mode)

                        def composed():
                            costs, oks = [], []
                            for off in offsets:
                                m = orthomosaic(views, dsm + float(off), grid, ZONE, view_dirs=dirs, mode=mode)
                                costs.append((m["std"].double() ** 2).sum(0))
                                oks.append(m["count"] >= 2)
                            cost, ok = torch.stack(costs), torch.stack(oks)
                            cost = torch.where(ok, cost, torch.full_like(cost, float("inf")))
                            got["level"] = torch.where(ok.any(0), cost.argmin(0), torch.full_like(cost[0], -1, dtype=torch.int64))
                        (t, t_med), (bt, bt_med) = alternately(fused, composed, 3 if side == 512 else 2)
                        agree = float((got["sweep"]["level"].long() == got["level"]).float().mean())
                        say(f"(b) {side} x {side}, K = {K}, Z = {Z}, {mode}: altitude_sweep, whole call {t * 1e3:.2f} ms (median {t_med * 1e3:.2f}); "
                            f"Z x orthomosaic + torch argmin {bt * 1e3:.2f} ms (median {bt_med * 1e3:.2f}): {bt / t:.1f} times; the same level at "
                            f"{100 * agree:.2f} % of the cells (the composed route marches on dsm + off at every level and squares a float32 std)")
                        del outs, got
                torch.cuda.empty_cache()
    del images
    torch.cuda.empty_cache()
    try:
        run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
        line = [json.loads(s) for s in run.stdout.splitlines() if s.startswith("{")][-1]
        say(f"# box-speed indicator: bench.py in the same visit, same box: {line['value'] / 1e3:.1f} k train rays/s, {line['ms_per_step']:.3f} ms "
            f"per step (BASELINE config 2, bf16).")
    except Exception as e:      # the indicator is a note, not a measurement of this file
        say(f"# box-speed indicator: bench.py did not give a result line ({type(e).__name__})")


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", "sweep_throughput.txt")
    if "--resources" in sys.argv:
        return resources(out_path)
    from dsm_throughput import LINES
    try:
        measure()
    finally:
        with open(out_path, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
