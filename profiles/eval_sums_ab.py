"""The launches whose block sums moved into csrc/block_sums.h, working tree against the parent commit's library, alternating in one
process by device events on a 512 x 512 view or grid: the method, the margin and `alternate` are profiles/surface_chain_ab.py's.
The parent's library (python profiles/build_baseline.py HEAD~1 eval_parent, and a copy of it as build/eval_parent2) is loaded
twice; a launch passes when |median(tree) - median(parent)| is within the spread of the two parent loads' per-round medians, or
it is OUTSIDE and the script exits 1.  Writes profiles/eval_sums_ab.txt (or the path given)."""
import os
import sys
from statistics import median

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import torch  # noqa: E402
from dsm_throughput import LINES, say  # noqa: E402
from surface_chain_ab import ROUNDS, REPS, alternate  # noqa: E402
from brdf_nerf_amd import _lib as L  # noqa: E402
from brdf_nerf_amd import functions as Fn  # noqa: E402
from brdf_nerf_amd.metrics import gaussian_window  # noqa: E402


@torch.no_grad()
def measure():
    dev = torch.device("cuda", 0)
    H = W = 512
    tree = L.lib()
    libs = {"tree": tree}
    for name, tag in (("parent", "eval_parent"), ("parent again", "eval_parent2")):
        libs[name] = L.load(os.path.join(ROOT, "brdf_nerf_amd", "build", tag, "libbrdfnerf_hip.so"), baseline=True)
    say(f"view or grid {H} x {W}; {ROUNDS} rounds of {REPS} timings per library and launch; device {torch.cuda.get_device_name(0)}; "
        f"source hashes {', '.join(f'{k} {h.bn_source_hash().decode()}' for k, h in libs.items())}")
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(3, H, W, generator=g).to(dev)
    pred = (gt + 0.1 * torch.randn(3, H, W, generator=g).to(dev)).clamp(0, 1)
    max_val, sums3 = float(gt.max()), torch.zeros(3, dtype=torch.int64, device=dev)
    z1 = (30.0 + 2.0 * torch.randn(H, W, generator=g)).to(dev)
    z2 = (z1 + 0.3 * torch.randn(H, W, generator=g).to(dev)).contiguous()
    n1, n2 = Fn.grid_normals(z1, 0.5), Fn.grid_normals(z2, 0.5)
    mask = (torch.rand(H, W, generator=g) < 0.5).to(torch.uint8).to(dev)
    sums6 = torch.zeros(6, dtype=torch.int64, device=dev)
    u, v = z1.double(), z2.double()
    ncc, skipped = torch.zeros((121, 6), dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    R, S, E = H * W, 128, 16
    zs = torch.sort(torch.rand(R, S, device=dev), dim=1).values
    ws = torch.rand(R, S, device=dev) / S
    depth = (zs * ws).sum(-1).contiguous()
    X, view = torch.randn(R, S, E, device=dev), torch.randn(R, 3, device=dev)
    cnt = torch.zeros(6, dtype=torch.int64, device=dev)
    launches = {f"bn_ssim_map(window {w})": (lambda gw=gaussian_window(w), w=w: Fn.ssim_map(pred, gt, 3, H, W, (H * W, W, 1), None, 1.0, max_val,
                                                                                               w, gw, sums3)) for w in (3, 11)}
    launches.update({
        "bn_normal_angle": lambda: Fn.normal_angle(n1, n2, mask, 0, sums6),
        "bn_ncc_moments(r = 5)": lambda: Fn.ncc_moments(u, v, 20.0, 10, 0, 0, 5, sums=ncc, skipped=skipped),
        "bn_dsm_shift_diff": lambda: Fn.dsm_shift_diff(z1, z2, 1, -2, 0.5, mask, sums6),
        "bn_ray_maps(S = 128, E = 16, accumulate, normal column)": lambda: Fn.ray_maps(zs, ws, depth, X, True, 4, view, cnt)})
    outside = []
    say("launch: median ms of tree / parent / parent again; spread of the parent's per-round medians; |tree - parent|")
    for name, fn in launches.items():
        ts = alternate(libs, fn)
        med = {k: median([t for r in v for t in r]) for k, v in ts.items()}
        rounds = [median(r) for k in ("parent", "parent again") for r in ts[k]]
        spread, gap = max(rounds) - min(rounds), abs(med["tree"] - med["parent"])
        outside += [name] if gap > spread else []
        say(f"{name}: {med['tree']:.4f} / {med['parent']:.4f} / {med['parent again']:.4f} ms; spread {spread:.4f} ms ({min(rounds):.4f} to "
            f"{max(rounds):.4f}); gap {gap:.4f} ms: {'OUTSIDE' if gap > spread else 'within'}")
    L.use(tree)
    say(f"outside their spread: {', '.join(outside) or 'none'}")
    return outside


if __name__ == "__main__":
    try:
        bad = measure()
    finally:
        with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "eval_sums_ab.txt"), "w") as f:
            f.write("\n".join(LINES) + "\n")
    sys.exit(1 if bad else 0)
