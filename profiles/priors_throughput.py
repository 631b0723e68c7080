"""Depth-prior throughput: the tie points of a 2048 x 2048 view (about 4 x 10^5 and 4 x 10^4 of them, distinct pixels in a
shuffled order) - the two launches bn_tie_owner + bn_tie_priors on buffers made once, by device events; the same outputs made
with view_rays(rows=, cols=) and torch index assignments on the device, by device events; and depth_priors as a whole call
(allocation, the amin / amax read, the padding, the normals, the counter read) by a host clock around a synchronise.  Ends with
bench.py in a child process as the box-speed indicator of the visit.  Writes profiles/priors_throughput.txt (or the path given
as the first argument).  Nothing here is a gate."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import camera_cases as M  # noqa: E402
from dsm_throughput import LINES, device_ms, say, timed  # noqa: E402
from brdf_nerf_amd import _lib as L  # noqa: E402
from brdf_nerf_amd import camera as Cm  # noqa: E402

H = W = 2048
HYPER = dict(corrscale=1.0, stdscale=1.0, margin=1e-4, std_span=0.0)


def one(site, cs, T, dev):
    _, _, zone, _ = M.SITES[site]
    lo, hi = M.alt_bounds(site)
    rpc = Cm.Rpc.from_dict(M.make_rpc(site, 3))
    _, center, rng = Cm.scene_bounds([{"rpc": rpc, "H": 64, "W": 64, "min_alt": lo, "max_alt": hi}], cs=cs, zone=zone, device=dev)
    g = torch.Generator(device=dev).manual_seed(T)
    flat = torch.randperm(H * W, device=dev, generator=g)[:T]
    px = torch.stack([flat % W, flat // W], -1).to(torch.int32).contiguous()
    cols, rows = px[:, 0].double(), px[:, 1].double()
    rays, _ = Cm.view_rays(rpc, 0, 0, lo, hi, (0.0, 0.0, 0.0), 1.0, cs=cs, zone=zone, rows=rows, cols=cols, precision="exact", device=dev)
    u = 0.3 + 0.4 * torch.rand(T, device=dev, generator=g, dtype=torch.float64)
    pts = (rays[:, :3].double() + (u * rays[:, 7].double())[:, None] * rays[:, 3:6].double()).contiguous()     # world points on the rays
    cor = (0.3 + 0.7 * torch.rand(T, device=dev, generator=g, dtype=torch.float64)).contiguous()
    cmin, cmax = float(cor.amin()), float(cor.amax())
    code, z, s = Cm._world_args(cs, zone, False)
    f32 = dict(dtype=torch.float32, device=dev)
    owner = torch.full((H, W), -1, dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    valid, depths, std = torch.zeros(H * W, **f32), torch.zeros((H * W, 2), **f32), torch.zeros(H * W, **f32)
    rmap, points, vfull = torch.zeros((H * W, 8), **f32), torch.zeros((H * W, 3), **f32), torch.zeros(H * W, **f32)
    c3 = (C.c_double * 3)(*center)
    p, st = Cm._p, Cm._stream

    def launches():
        L.check(L.lib().bn_tie_owner(p(px), T, H, W, p(owner), p(counts), st()), "bn_tie_owner")
        L.check(L.lib().bn_tie_priors(rpc.ref(), p(px), p(owner), p(pts), p(cor), T, H, W, H, W, None, None, 1.0, lo, hi, code, z, s, c3, rng, 1,
                                      cmin, cmax, 1.0, 1.0, 1e-4, 0.0, p(valid), p(depths), p(std), p(rmap), p(points), p(vfull), None,
                                      p(counts), st()), "bn_tie_priors")

    idx = (px[:, 1].long() * W + px[:, 0].long())
    c32, r32 = torch.tensor(center, **f32), torch.tensor(rng, **f32)

    def in_torch():
        r, _ = Cm.view_rays(rpc, 0, 0, lo, hi, center, rng, cs=cs, zone=zone, rows=rows, cols=cols, device=dev)
        q = (pts.float() - c32) / r32
        depth = torch.linalg.norm(q - r[:, :3], dim=1)
        w = (((cor - cmin) / (cmax - cmin)) * 1.0).float() * (-r[:, 5])
        sd = (1.0 * (1.0 - w) + 1e-4) * 0.0
        valid[idx], vfull[idx], std[idx], rmap[idx], points[idx] = 1.0, 1.0, sd, r[:, :8], q
        depths[idx] = torch.stack([depth, w], -1)

    k_ms, k_med = device_ms(launches)
    t_ms, t_med = device_ms(in_torch)
    whole, whole_med = timed(lambda: Cm.depth_priors(rpc, H, W, px, pts, cor, lo, hi, center, rng, cs=cs, zone=zone, want_rays=True,
                                                     device=dev, **HYPER), 5)
    lean, lean_med = timed(lambda: Cm.depth_priors(rpc, H, W, px, pts, cor, lo, hi, center, rng, cs=cs, zone=zone, want_normals=False,
                                                   device=dev, **HYPER), 5)
    say(f"({site} {cs}) {H} x {W}, {T} tie points: bn_tie_owner + bn_tie_priors {k_ms:.3f} ms (median {k_med:.3f}) = "
        f"{T / k_ms / 1e6:.2f} G ties/s; view_rays + torch index assignments {t_ms:.3f} ms (median {t_med:.3f}) = {t_ms / k_ms:.1f} x; "
        f"depth_priors with rays and normals {whole * 1e3:.3f} ms (median {whole_med * 1e3:.3f}), without {lean * 1e3:.3f} ms "
        f"(median {lean_med * 1e3:.3f}); counters {counts.tolist()[2:]} skipped / unsampled")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "priors_throughput.txt")
    dev = torch.device("cuda", 0)
    say(f"device {torch.cuda.get_device_name(0)}; a lane per tie point, blocks of 256; tie_priors_kernel: 109 VGPRs, 0 bytes of scratch, "
        f"4 waves per SIMD; tie_owner_kernel: 10 VGPRs, 0 bytes of scratch; rpc_rays_kernel unchanged at 101 VGPRs (hipcc's "
        f"kernel-resource-usage remarks)")
    for site, cs in (("z17", "utm"), ("z17", "ecef"), ("z21", "utm")):
        for T in (400000, 40000):
            one(site, cs, T, dev)
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
