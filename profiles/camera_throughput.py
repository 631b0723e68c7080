"""Camera throughput: the rays of a 2048 x 2048 view at the three synthetic sites of tests/camera_cases.py - bn_rpc_rays alone by
device events (one launch, both precisions, UTM and ECEF), view_rays as a whole by a host clock around a synchronise (its
allocation and the read of `skipped` included), and the numpy statement on the host (timed on the view's first 512 rows x 512
columns, 1/16 of the rays, and scaled).  Achieved GB/s counts the 44 bytes per ray written (32 without a sun).  Ends with
bench.py in a child process as the box-speed indicator of the visit.  Writes profiles/camera_throughput.txt (or the path given
as the first argument).  Nothing here is a gate."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import camera_cases as M  # noqa: E402
from dsm_throughput import LINES, device_ms, say, timed  # noqa: E402
from brdf_nerf_amd import camera as Cm  # noqa: E402

H = W = 2048
TILE = 512


def one(site, dev):
    _, _, zone, _ = M.SITES[site]
    lo, hi = M.alt_bounds(site)
    d = M.make_rpc(site, 3)
    rpc = Cm.Rpc.from_dict(d)
    n = H * W
    for cs in ("utm", "ecef"):
        _, center, rng = Cm.scene_bounds([{"rpc": rpc, "H": 64, "W": 64, "min_alt": lo, "max_alt": hi}], cs=cs, zone=zone, device=dev)
        code, z, s = Cm._world_args(cs, zone, False)
        out = torch.empty((n, 11), dtype=torch.float32, device=dev)
        counts = torch.zeros(1, dtype=torch.int64, device=dev)
        sun = Cm.sun_direction(*M.SUN)
        for precision in ("reference", "exact"):
            launch = lambda: Cm.rays_launch(rpc, None, None, W, 0, n, lo, hi, code, z, s, center, rng, sun, Cm._PRECISION[precision], out,
                                            counts=counts)
            k_ms, k_med = device_ms(launch)
            t_all, t_med = timed(lambda: Cm.view_rays(rpc, H, W, lo, hi, center, rng, cs=cs, zone=zone, sun=M.SUN, precision=precision,
                                                      device=dev), 5)
            say(f"({site} {cs} {precision}) {H} x {W}: bn_rpc_rays {k_ms:.3f} ms (median {k_med:.3f}) = {n / k_ms / 1e6:.2f} G rays/s, "
                f"{44 * n / k_ms / 1e6:.1f} GB/s of rays written; view_rays {t_all * 1e3:.3f} ms (median {t_med * 1e3:.3f}); skipped "
                f"{int(counts.item())}")
        if cs == "utm":
            c, r = M.grid_pixels(TILE, TILE)
            t0 = time.time()
            M.rays(d, c, r, lo, hi, cs, zone, False, center, rng, sun)
            t_host = (time.time() - t0) * (n / (TILE * TILE))
            say(f"    numpy statement on the host ({TILE} x {TILE} timed, x {n // (TILE * TILE)}): {t_host:.1f} s for the view = "
                f"{t_host * 1e3 / k_ms:.0f} x the kernel")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "camera_throughput.txt")
    dev = torch.device("cuda", 0)
    say(f"device {torch.cuda.get_device_name(0)}; a lane per ray (near and far in one lane), blocks of 256; rpc_rays_kernel: 101 VGPRs, "
        f"0 bytes of scratch, 4 waves per SIMD (hipcc's kernel-resource-usage remarks)")
    for site in sorted(M.SITES):
        one(site, dev)
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
