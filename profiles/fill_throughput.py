"""Hole-filling throughput: on 512 x 512 and 2048 x 2048 grids with 5 % random holes plus NaN patches of 20 to 60 cells a side
(the pattern a splat leaves: single cells between the rays and whole occluded patches) (a) bn_grid_nearest_col and bn_grid_fill
alone and fill_holes as a whole; (b) the row pass with near_row read through L2 instead of staged into LDS (a variant build,
-DBN_FILL_NO_LDS, taken from brdf_nerf_amd/build/BN_FILL_NO_LDS/ or built there), alternately with the product in one process;
(c) the host paths, both including the copy of the grid to the host: the reference's griddata(method='nearest') and, as the
stronger baseline, scipy.ndimage.distance_transform_edt(return_indices=True); (d) a sparse grid (90 % holes), where the scans
are long.  Kernel times by device events, whole calls by a host clock around a synchronise.  Ends with bench.py in a child
process as the box-speed indicator of the visit.  Writes profiles/fill_throughput.txt (or the path given as the first
argument).  Nothing here is a gate."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dsm_throughput import LINES, device_ms, say, timed  # noqa: E402
from brdf_nerf_amd import _lib as L  # noqa: E402
from brdf_nerf_amd import fill_holes  # noqa: E402
from brdf_nerf_amd import functions as Fn  # noqa: E402
from brdf_nerf_amd.build import HERE as PKG, build  # noqa: E402

VARIANT = os.path.join(PKG, "build", "BN_FILL_NO_LDS", "libbrdfnerf_hip.so")


def grid(H, W, frac, patches, gen):
    jj, ii = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    u = (40.0 + 4.0 * torch.sin(jj / 17.0) * torch.cos(ii / 23.0) + 0.02 * ii + 0.05 * torch.randn(H, W, generator=gen, dtype=torch.float64)).float()
    u[torch.rand(H, W, generator=gen) < frac] = float("nan")
    for _ in range(patches):
        h, w = (int(x) for x in torch.randint(20, 61, (2,), generator=gen))
        r0, c0 = int(torch.randint(0, H - h, (1,), generator=gen)), int(torch.randint(0, W - w, (1,), generator=gen))
        u[r0:r0 + h, c0:c0 + w] = float("nan")
    return u


def host_griddata(u):
    from scipy import interpolate
    a = u.cpu().numpy()
    h, w = a.shape
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))
    m = np.isnan(a)
    out = a.copy()
    out[yy[m], xx[m]] = interpolate.griddata((xx[~m], yy[~m]), a[~m], (xx[m], yy[m]), method="nearest")
    return out


def host_edt(u):
    from scipy import ndimage
    a = u.cpu().numpy()
    idx = ndimage.distance_transform_edt(np.isnan(a), return_distances=False, return_indices=True)
    return a[idx[0], idx[1]]


def one(tag, H, W, frac, patches, gen, dev, variant, host=True):
    u = grid(H, W, frac, patches, gen).to(dev)
    res = fill_holes(u)
    near = Fn.grid_nearest_col(u)
    c_ms, c_med = device_ms(lambda: Fn.grid_nearest_col(u))
    r_ms, r_med = device_ms(lambda: Fn.grid_fill(u, near))
    t_all, t_all_med = timed(lambda: fill_holes(u), 5)
    say(f"({tag}) {H} x {W}, {res['holes']} holes ({100.0 * res['holes'] / (H * W):.1f} %), max distance {res['max_dist']:.2f} cells: "
        f"bn_grid_nearest_col {c_ms:.3f} ms (median {c_med:.3f}), bn_grid_fill {r_ms:.3f} ms (median {r_med:.3f}) = "
        f"{H * W / r_ms / 1e6:.2f} G cells/s; fill_holes {t_all * 1e3:.3f} ms (median {t_all_med * 1e3:.3f}) with its two scalar reads")
    if variant is not None:
        lds, l2 = [], []
        for _ in range(3):                                   # alternately, in one process
            lds.append(device_ms(lambda: Fn.grid_fill(u, near))[1])
            prev = L.use(variant)
            try:
                l2.append(device_ms(lambda: Fn.grid_fill(u, near))[1])
                other = Fn.grid_fill(u, near)[0]
            finally:
                L.use(prev)
        same = torch.equal(other.view(torch.int32), res["filled"].view(torch.int32))
        say(f"    row pass, near_row staged in LDS (kept) {min(lds):.3f} ms; read through L2 {min(l2):.3f} ms (medians of 20, best of 3 "
            f"alternations); same bits: {same}")
    if host:
        t_g, _ = timed(lambda: host_griddata(u), 1)
        t_e, t_e_med = timed(lambda: host_edt(u), 3)
        mine = res["filled"].cpu().numpy()
        g, e = host_griddata(u), host_edt(u)
        say(f"    host, copy included: griddata(method='nearest') {t_g * 1e3:.1f} ms ({t_g / t_all:.0f} x fill_holes), "
            f"distance_transform_edt(return_indices=True) {t_e * 1e3:.1f} ms (median {t_e_med * 1e3:.1f}; {t_e / t_all:.0f} x); cells "
            f"with another value than fill_holes (ties): griddata {int((g != mine).sum())}, edt {int((e != mine).sum())}")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fill_throughput.txt")
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    if not os.path.exists(VARIANT):
        build(defines=["BN_FILL_NO_LDS"])
    variant = L.load(VARIANT, baseline=True)
    say(f"device {torch.cuda.get_device_name(0)}; column pass: a lane per column, blocks of 64; row pass: a block of 256 per row")
    one("a", 512, 512, 0.05, 12, gen, dev, variant)
    one("b", 2048, 2048, 0.05, 150, gen, dev, variant)
    one("c", 64, 64, 0.05, 0, gen, dev, variant, host=False)
    one("d", 512, 512, 0.90, 0, gen, dev, variant, host=False)
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
