"""Horizon and sky view of a surface model: what the march and the sum cost.  visibility_throughput.py's synthetic urban reliefs of
512 x 512 and 2048 x 2048 cells of 0.5 m, D = 8 / 32 / 64 azimuths from azimuths(D, 17), with and without max_dist = 100 m.

(a) by device events: bn_grid_horizon (slope, no hit) - and, with a variant library as the second argument (the tree built with
    -DBN_HORIZON_NO_ZMAX: the march without its early exit), that library's entry alternately in the same process, with the bytes
    of the two tables compared - and bn_sky_view over the table in tiles of 8 planes;
(b) whole calls by a host clock: sky_view_factor (dir_tile 8) with its peak device memory, and grid_visibility at K = D and
    elevation 30 for scale;
(c) the same march as float64 torch ops on the device at 512 x 512 with one azimuth.
Ends with bench.py in a child process as the box-speed indicator of the visit.  Writes profiles/horizon_throughput.txt (or the path
given as the first argument).  Nothing here is a gate."""
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import torch  # noqa: E402
from dsm_throughput import LINES, device_ms, say, timed  # noqa: E402
from visibility_throughput import RES, dirs_of, urban  # noqa: E402
from brdf_nerf_amd import azimuths, grid_visibility, sky_view_factor  # noqa: E402
from brdf_nerf_amd import _lib as L  # noqa: E402
from brdf_nerf_amd import functions as Fn  # noqa: E402

MAX_DIST = 100.0


def torch_march(dsm, res, az, zmax):
    """The rule as float64 torch ops on the device over all cells at once, one azimuth: -> slope (H, W) float32."""
    H, W = dsm.shape
    cells = dsm.double().reshape(-1)
    jj, ii = torch.meshgrid(torch.arange(H, device=dsm.device), torch.arange(W, device=dsm.device), indexing="ij")
    u0, v0, z0 = (ii + 0.5).double().reshape(-1), (jj + 0.5).double().reshape(-1), cells
    a = max(abs(float(az[0])), abs(float(az[1])))
    su, sv = float(az[0]) / a, -(float(az[1]) / a)
    step = math.sqrt(su * su + sv * sv) * res
    best = torch.zeros_like(z0)
    live = torch.isfinite(z0)
    top = zmax - z0
    for t in range(1, max(W, H) + 1):
        ut, vt, run = u0 + t * su, v0 + t * sv, t * step
        live = live & (ut >= 0) & (ut < W) & (vt >= 0) & (vt < H) & ~(top / run <= best)
        if t % 16 == 0 and not bool(live.any()):
            break
        c = (torch.floor(vt).long().clamp(0, H - 1) * W + torch.floor(ut).long().clamp(0, W - 1))
        s = (cells[c] - z0) / run
        best = torch.where(live & (s > best), s, best)
    return torch.where(torch.isfinite(z0), best, torch.full_like(best, float("nan"))).float().reshape(H, W)


def main():
    try:
        measure()
    finally:
        out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "horizon_throughput.txt")
        with open(out_path, "w") as f:
            f.write("\n".join(LINES) + "\n")


def measure():
    dev = torch.device("cuda", 0)
    here = L.lib()
    variant = L.load(sys.argv[2], baseline=True) if len(sys.argv) > 2 else None
    say(f"urban relief, 0.5 m cells; device {torch.cuda.get_device_name(0)}" +
        (f"; variant library (no zmax exit): {os.path.relpath(sys.argv[2], ROOT)}" if variant else ""))
    with torch.no_grad():
        for side in (512, 2048):
            dsm = torch.from_numpy(urban(side)).to(dev)
            zmax = float(dsm.max())
            for D in (8, 32, 64):
                az = azimuths(D, 17.0)
                slope = torch.empty((D, side, side), dtype=torch.float32, device=dev)
                other = torch.empty_like(slope) if variant is not None else None
                for steps, name in ((None, "whole grid"), (int(MAX_DIST / RES), f"max_dist {MAX_DIST:.0f} m")):
                    call = lambda out=slope: Fn.grid_horizon(dsm, RES, az, steps, zmax, slope=out)
                    reps = 10 if side * side * D <= 1 << 24 else 3
                    best = {"kernel": [], "no zmax exit": []}
                    for _ in range(2):                               # alternately, in one process
                        best["kernel"].append(device_ms(call, reps))
                        if variant is not None:
                            prev = L.use(variant)
                            best["no zmax exit"].append(device_ms(lambda: call(other), reps))
                            L.use(prev)
                    line = f"(a) bn_grid_horizon {side} x {side}, D = {D}, {name}: {100.0 * float((slope > 0).float().mean()):.1f} % of the slopes > 0"
                    for kind, ts in best.items():
                        if ts:
                            lo, med = min(t[0] for t in ts), min(t[1] for t in ts)
                            line += f"; {kind} {lo:.3f} ms (median {med:.3f}) = {D * side * side / lo / 1e6:.2f} G starts/s"
                    if variant is not None:
                        line += ", the same bytes" if torch.equal(slope.view(torch.int32), other.view(torch.int32)) else ", DIFFERENT bytes"
                    if D == 8 and side == 512 and steps is None:
                        lo, med = device_ms(lambda: torch_march(dsm, RES, az[0], zmax), 2)
                        same = torch.equal(torch_march(dsm, RES, az[0], zmax).view(torch.int32), slope[0].view(torch.int32))
                        line += f"; one azimuth as torch float64 ops {lo:.1f} ms (median {med:.1f}), {'the same bytes' if same else 'DIFFERENT bytes'}"
                    say(line)
                acc = torch.zeros((side, side), dtype=torch.float64, device=dev)
                svf = torch.empty((side, side), dtype=torch.float32, device=dev)
                sums = torch.zeros((3,), dtype=torch.int64, device=dev)
                lo, med = device_ms(lambda: Fn.sky_view(slope[:8], acc, D, last=False), 10)
                lo2, med2 = device_ms(lambda: Fn.sky_view(slope[:8], acc, D, svf=svf, sums=sums), 10)
                say(f"(a) bn_sky_view {side} x {side}, a tile of 8 planes: {lo:.3f} ms (median {med:.3f}); the last tile, with svf and sums: "
                    f"{lo2:.3f} ms (median {med2:.3f})")
                del slope, other, acc, svf
                for dist in (None, MAX_DIST):
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    t, t_med = timed(lambda: sky_view_factor(dsm, RES, az=az, max_dist=dist), 2)
                    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                    res = sky_view_factor(dsm, RES, az=az, max_dist=dist)
                    say(f"(b) sky_view_factor {side} x {side}, D = {D}, dir_tile 8, {'whole grid' if dist is None else f'max_dist {dist:.0f} m'}: "
                        f"{t * 1e3:.2f} ms (median {t_med * 1e3:.2f}), peak {peak:.0f} MiB above the DSM; mean svf {res['mean']:.5f}")
                t, t_med = timed(lambda: grid_visibility(dsm, RES, dirs_of(D, 30)), 2)
                say(f"(b) for scale: grid_visibility {side} x {side}, K = {D}, elevation 30, whole call: {t * 1e3:.2f} ms (median {t_med * 1e3:.2f})")
        assert L.lib() is here
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
