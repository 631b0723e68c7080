"""The orthomosaic of several observed images on the grid of a DSM: what the fused launch costs, and what it saves.  The relief and
the camera of orthophoto_throughput.py - urban reliefs of 512 x 512 and 2048 x 2048 cells of 0.5 m, 2048 x 2048 x 3 images of some
0.5 m per pixel - under K = 1 / 4 / 16 / 32 cameras some 25 degrees off nadir, their azimuths spread round the circle.

(a) by device events: bn_grid_mosaic (bilinear, with the K occlusion masks), and the K-launch chain it replaces, bn_grid_pixels +
    bn_image_gather per view;
(b) whole calls by a host clock: orthomosaic with view_dirs given, against K x orthophoto with view_dir given plus a float64 torch
    reduction of the (K, C, H, W) stack (mean, population std, count and the first kept view) - orthophoto's entries are the parent
    commit's; peak device memory of both above the inputs;
(c) with --resources (no GPU needed): VGPRs, scratch, LDS and waves per SIMD of grid_mosaic_kernel<C> as the compiler reports them.
Ends with bench.py in a child process as the box-speed indicator of the visit.  Writes profiles/mosaic_throughput.txt (or the path
given as the first argument; --resources appends to it).  Nothing here is a gate."""
import json
import math
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

VIEWS = (1, 4, 16, 32)


def resources(out_path):
    from brdf_nerf_amd import build as B
    with tempfile.TemporaryDirectory() as tmp:
        cmd = B.compile_command(os.path.join(B.CSRC, "mosaic.hip"), os.path.join(tmp, "mosaic.s"), asm=True)
        log = subprocess.run(cmd + ["-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    rows, got = [], None
    for l in log.splitlines():
        m = re.search(r"Function Name: \S*grid_mosaic_kernelILi(\d)E", l)
        if m:
            got = {"C": m.group(1)}
            rows.append(got)
        for key, tag in (("VGPRs", " VGPRs:"), ("scratch", "ScratchSize [bytes/lane]:"), ("LDS", "LDS Size [bytes/block]:"),
                         ("waves", "Occupancy [waves/SIMD]:"), ("sgpr_spill", "SGPRs Spill:")):
            if got is not None and tag in l:
                got[key] = l.split(tag)[1].split()[0]
    with open(out_path, "a") as f:
        for got in rows:
            s = f"(c) grid_mosaic_kernel<{got['C']}>: {got.get('VGPRs')} VGPRs, {got.get('scratch')} B of scratch per lane, {got.get('LDS')} B of " \
                f"LDS, {got.get('waves')} waves per SIMD, {got.get('sgpr_spill')} SGPRs held in VGPR lanes (gfx950, as the compiler reports them)"
            print(s)
            f.write(s + "\n")


def cameras(K):
    """K cameras of orthophoto_throughput.scene_rpc, the off-nadir altitude term turned round the circle."""
    from orthophoto_throughput import scene_rpc
    ds = []
    for k in range(K):
        d = scene_rpc(seed=k)
        phi = 2.0 * math.pi * k / K + 0.5
        d["col_num"][3], d["row_num"][3] = 0.1 * math.cos(phi), -0.1 * math.sin(phi)
        ds.append(d)
    return ds


def measure():
    import numpy as np
    import torch
    import orthophoto_cases as O
    from dsm_throughput import device_ms, say, timed
    from orthophoto_throughput import IMAGE, RES, ZONE
    from visibility_throughput import urban
    from brdf_nerf_amd import Grid, Rpc, camera, orthomosaic, orthophoto
    from brdf_nerf_amd import functions as Fn
    dev = torch.device("cuda", 0)
    say(f"urban relief, 0.5 m cells, zone {ZONE} north; K images of {IMAGE} x {IMAGE} x 3 float32 each; device {torch.cuda.get_device_name(0)}")
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
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                res = orthomosaic(views, dsm, grid, ZONE, view_dirs=dirs)
                torch.cuda.synchronize()
                peak_fused = torch.cuda.max_memory_allocated() - base
                hist = torch.bincount(res["count"].reshape(-1).long(), minlength=K + 1).tolist()
                say(f"    {side} x {side}, K = {K}: cells seen by 0 .. {K} views {hist if K <= 4 else hist[:3] + ['...'] + hist[-2:]}; consistency "
                    f"{res['consistency']:.4f} over {res['cells']} cells")
                table = [(images[k], IMAGE, IMAGE, strides, res["visible"][k], res["rank"][k], rpcs[k]) for k in range(K)]
                outs = dict(count=res["count"], best=res["best"], best_val=res["best_rgb"], mean=res["mean"], std=res["std"],
                            counts=torch.zeros((K, 5), dtype=torch.int64, device=dev), sums=torch.zeros(3, dtype=torch.int64, device=dev))
                lo, med = device_ms(lambda: Fn.grid_mosaic(table, 3, dsm, xoff, yoff, RES, ZONE, 0, **outs), 10)
                colrow = torch.empty((side, side, 2), dtype=torch.float64, device=dev)
                out = torch.empty((3, side, side), dtype=torch.float32, device=dev)
                state = torch.empty((side, side), dtype=torch.uint8, device=dev)
                c1, c4 = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)

                def chain():
                    for k in range(K):
                        Fn.grid_pixels(rpcs[k], dsm, xoff, yoff, RES, ZONE, 0, colrow=colrow, counts=c1)
                        Fn.image_gather(images[k], IMAGE, IMAGE, 3, strides, colrow, res["visible"][k], out=out, state=state, counts=c4)
                clo, cmed = device_ms(chain, 10)
                say(f"(a) {side} x {side}, K = {K}: bn_grid_mosaic {lo:.3f} ms (median {med:.3f}) = {lo / K:.3f} ms per view, {n * K / lo / 1e6:.2f} G "
                    f"cell-views/s; K x (bn_grid_pixels + bn_image_gather) {clo:.3f} ms (median {cmed:.3f}) = {clo / K:.3f} ms per view")
                t, t_med = timed(lambda: orthomosaic(views, dsm, grid, ZONE, view_dirs=dirs), 5)

                def baseline():
                    singles = [orthophoto(*views[k], dsm, grid, ZONE, view_dir=dirs[k]) for k in range(K)]
                    stack = torch.stack([s["ortho"] for s in singles]).double()                       # (K, C, H, W)
                    used = torch.isfinite(stack).all(1, keepdim=True)
                    cnt = used.sum(0)
                    x = torch.where(used, stack, torch.zeros_like(stack))
                    mean = x.sum(0) / cnt
                    std = torch.sqrt((torch.where(used, (stack - mean) ** 2, torch.zeros_like(stack))).sum(0) / cnt)
                    first = used.squeeze(1).to(torch.uint8).argmax(0)
                    return mean.float(), std.float(), cnt, first
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                bmean, bstd, _, _ = baseline()
                torch.cuda.synchronize()
                peak_base = torch.cuda.max_memory_allocated() - base
                both = torch.isfinite(bmean) & torch.isfinite(res["mean"])
                dmean = float((bmean - res["mean"])[both].abs().max())
                dstd = float((bstd - res["std"])[both].abs().max())
                del bmean, bstd
                bt, bt_med = timed(baseline, 3)
                say(f"(b) {side} x {side}, K = {K}: orthomosaic, whole call {t * 1e3:.2f} ms (median {t_med * 1e3:.2f}), peak {peak_fused / 2 ** 20:.1f} MiB "
                    f"above the inputs; K x orthophoto + float64 torch reduction {bt * 1e3:.2f} ms (median {bt_med * 1e3:.2f}), peak "
                    f"{peak_base / 2 ** 20:.1f} MiB; mean within {dmean:.3g}, std within {dstd:.3g} of it")
                del res, table, outs, colrow, out, state
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
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", "mosaic_throughput.txt")
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
