"""The orthophoto of an observed image on the grid of a DSM: what the chain costs.  Synthetic urban reliefs of 512 x 512 and
2048 x 2048 cells of 0.5 m (visibility_throughput.urban) under a tilted synthetic RPC of some 0.5 m per pixel, against a
2048 x 2048 three-channel image.

(a) by device events: bn_grid_pixels and bn_image_gather (bilinear and nearest, both layouts, with the occlusion mask), and the same
    chain - inverse UTM, polynomials, bilinear taps - as float64 torch ops on the device, for scale and as a cross-check;
(b) whole calls by a host clock: orthophoto with and without occlusion (the march towards the sensor, its direction, the counts
    to the host), grid_pixels, sample_image;
(c) the numpy statement of tests/orthophoto_cases.py on the host, timed on a fraction of the grid;
(d) with --resources (no GPU needed): VGPRs, scratch, LDS and waves per SIMD of the file's kernels as the compiler reports them.
Ends with bench.py in a child process as the box-speed indicator of the visit.  Writes profiles/orthophoto_throughput.txt (or the
path given as the first argument; --resources appends to it).  Nothing here is a gate."""
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
import numpy as np  # noqa: E402

RES, ZONE, SITE = 0.5, 17, (30.3, -81.7, 10.0)          # cell size; the scene: zone 17 north at lat 30.3, lon -81.7, ground at 10 m
IMAGE = 2048


def scene_rpc(seed=0):
    """An image of IMAGE x IMAGE pixels of some 0.5 m around the site: a linear part with an off-nadir altitude term (0.1 of the
    scale per 200 m: some 25 degrees off nadir), every other coefficient drawn at relative size 1e-4."""
    lat, lon, alt = SITE
    rng = np.random.default_rng(seed)
    half = IMAGE / 2.0
    d = {"row_offset": half, "col_offset": half, "lat_offset": lat, "lon_offset": lon, "alt_offset": alt, "row_scale": half,
         "col_scale": half, "lat_scale": half * 0.5 / 110850.0, "lon_scale": half * 0.5 / 96200.0, "alt_scale": 200.0}
    for k in ("row_num", "row_den", "col_num", "col_den"):
        d[k] = rng.uniform(-1e-4, 1e-4, 20)
    d["col_num"][1:4] = (1.0, 0.02, 0.1)
    d["row_num"][1:4] = (0.02, -1.0, -0.06)
    d["col_den"][0] = d["row_den"][0] = 1.0
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def resources(out_path):
    from brdf_nerf_amd import build as B
    with tempfile.TemporaryDirectory() as tmp:
        cmd = B.compile_command(os.path.join(B.CSRC, "orthophoto.hip"), os.path.join(tmp, "orthophoto.s"), asm=True)
        log = subprocess.run(cmd + ["-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    lines, name = [], None
    for l in log.splitlines():
        m = re.search(r"Function Name: \S*?\d\d([a-z_]+_kernel)E", l)
        if m:
            name, got = m.group(1), {}
            lines.append((name, got))
        for key, tag in (("VGPRs", "VGPRs:"), ("scratch", "ScratchSize [bytes/lane]:"), ("LDS", "LDS Size [bytes/block]:"),
                         ("waves", "Occupancy [waves/SIMD]:")):
            if name and " " + tag in l:
                got[key] = l.split(tag)[1].split()[0]
    with open(out_path, "a") as f:
        for name, got in lines:
            s = f"(d) {name}: {got.get('VGPRs')} VGPRs, {got.get('scratch')} B of scratch per lane, {got.get('LDS')} B of LDS, " \
                f"{got.get('waves')} waves per SIMD (gfx950, as the compiler reports them)"
            print(s)
            f.write(s + "\n")


def torch_chain(rpc_d, dsm, xoff, yoff, zone, image):
    """Cell centres -> inverse UTM -> polynomials -> bilinear taps as float64 torch ops on the device (no occlusion, no states beyond
    inside / outside): -> colrow (H, W, 2), ortho (C, H, W)."""
    import torch
    import orthophoto_cases as O
    dev = dsm.device
    H, W = dsm.shape
    e_, e2m, k0A, beta = O.utm_inverse_constants()
    jj, ii = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    xi = (yoff - (jj.double() + 0.5) * RES) / k0A
    eta = (xoff + (ii.double() + 0.5) * RES - 500000.0) / k0A
    xip, etap = xi, eta
    for j in range(1, 7):
        xip = xip - beta[j - 1] * (torch.sin(2.0 * j * xi) * torch.cosh(2.0 * j * eta))
        etap = etap - beta[j - 1] * (torch.cos(2.0 * j * xi) * torch.sinh(2.0 * j * eta))
    sh, cx = torch.sinh(etap), torch.cos(xip)
    lon = (6.0 * zone - 183.0) + torch.atan2(sh, cx) * 180.0 / np.pi
    taup = torch.sin(xip) / torch.sqrt(sh * sh + cx * cx)
    tau = taup
    for _ in range(O.NEWTON_ITERS):
        r = torch.sqrt(1.0 + tau * tau)
        sigma = torch.sinh(e_ * torch.atanh(e_ * tau / r))
        t = tau * torch.sqrt(1.0 + sigma * sigma) - sigma * r
        tau = tau + (taup - t) / torch.sqrt(1.0 + t * t) * (1.0 + e2m * (tau * tau)) / (e2m * r)
    lat = torch.atan(tau) * 180.0 / np.pi
    L = (lon - rpc_d["lon_offset"]) / rpc_d["lon_scale"]
    P = (lat - rpc_d["lat_offset"]) / rpc_d["lat_scale"]
    Hn = (dsm.double() - rpc_d["alt_offset"]) / rpc_d["alt_scale"]
    m4, m5, m6, m7, m8, m9 = L * P, L * Hn, P * Hn, L * L, P * P, Hn * Hn
    m = [torch.ones_like(L), L, P, Hn, m4, m5, m6, m7, m8, m9, (P * L) * Hn, m7 * L, m4 * P, m5 * Hn, m7 * P, m8 * P, m6 * Hn, m7 * Hn,
         m8 * Hn, m9 * Hn]
    poly = lambda c: sum(float(c[k]) * m[k] for k in range(20))
    col = poly(rpc_d["col_num"]) / poly(rpc_d["col_den"]) * rpc_d["col_scale"] + rpc_d["col_offset"]
    row = poly(rpc_d["row_num"]) / poly(rpc_d["row_den"]) * rpc_d["row_scale"] + rpc_d["row_offset"]
    Hi, Wi, C = image.shape
    ok = (col >= 0) & (col <= Wi - 1) & (row >= 0) & (row <= Hi - 1)
    c0 = torch.floor(col).long().clamp(0, Wi - 2)
    r0 = torch.floor(row).long().clamp(0, Hi - 2)
    fx, fy = (col - c0).unsqueeze(-1), (row - r0).unsqueeze(-1)
    img = image.double()
    v = (1 - fy) * ((1 - fx) * img[r0, c0] + fx * img[r0, c0 + 1]) + fy * ((1 - fx) * img[r0 + 1, c0] + fx * img[r0 + 1, c0 + 1])
    v = torch.where(ok.unsqueeze(-1), v, torch.full_like(v, float("nan")))
    return torch.stack([col, row], -1), v.float().permute(2, 0, 1).contiguous()


def measure():
    import torch
    import orthophoto_cases as O
    from dsm_throughput import device_ms, say, timed
    from visibility_throughput import urban
    from brdf_nerf_amd import Grid, Rpc, grid_pixels, orthophoto, sample_image
    from brdf_nerf_amd import functions as Fn
    dev = torch.device("cuda", 0)
    d = scene_rpc()
    rpc = Rpc.from_dict(d)
    say(f"urban relief, 0.5 m cells, zone {ZONE} north; image {IMAGE} x {IMAGE} x 3 float32; device {torch.cuda.get_device_name(0)}")
    torch.manual_seed(0)
    image = torch.rand((IMAGE * IMAGE, 3), device=dev)
    planes = image.reshape(IMAGE, IMAGE, 3).permute(2, 0, 1).contiguous()
    with torch.no_grad():
        for side in (512, 2048):
            relief = urban(side)
            xoff, yoff = O.site_grid("z17", side, side, RES)
            grid = Grid(xoff, yoff, RES, side, side)
            dsm = torch.from_numpy(relief).to(dev)
            n = side * side
            colrow = torch.empty((side, side, 2), dtype=torch.float64, device=dev)
            counts = torch.zeros(1, dtype=torch.int64, device=dev)
            lo, med = device_ms(lambda: Fn.grid_pixels(rpc, dsm, xoff, yoff, RES, ZONE, 0, colrow=colrow, counts=counts), 20)
            say(f"(a) {side} x {side}: bn_grid_pixels {lo:.3f} ms (median {med:.3f}) = {n / lo / 1e6:.2f} G cells/s")
            res = orthophoto(image, IMAGE, IMAGE, rpc, dsm, grid, ZONE)
            vis, c = res["visible"], res["counts"]
            say(f"    states of the {n} cells: {c}; view_dir {[round(v, 3) for v in res['view_dir'].tolist()]}")
            out = torch.empty((3, side, side), dtype=torch.float32, device=dev)
            state = torch.empty((side, side), dtype=torch.uint8, device=dev)
            cnt4 = torch.zeros(4, dtype=torch.int64, device=dev)
            for layout, buf, strides in (("image (H W, 3)", image, (IMAGE * 3, 3, 1)), ("planes (3, H, W)", planes, (IMAGE, 1, IMAGE * IMAGE))):
                for mode in ("bilinear", "nearest"):
                    lo, med = device_ms(lambda: Fn.image_gather(buf, IMAGE, IMAGE, 3, strides, colrow, vis, mode=mode, out=out, state=state,
                                                                counts=cnt4), 20)
                    say(f"(a) {side} x {side}: bn_image_gather {mode}, {layout}, with vis: {lo:.3f} ms (median {med:.3f}) = "
                        f"{n / lo / 1e6:.2f} G cells/s")
            lo, med = device_ms(lambda: torch_chain(d, dsm, xoff, yoff, ZONE, image.reshape(IMAGE, IMAGE, 3)), 3)
            tcr, tv = torch_chain(d, dsm, xoff, yoff, ZONE, image.reshape(IMAGE, IMAGE, 3))
            free = orthophoto(image, IMAGE, IMAGE, rpc, dsm, grid, ZONE, occlusion=False)
            dpx = float((tcr - free["colrow"]).abs().max())
            both = torch.isfinite(tv) & torch.isfinite(free["ortho"])
            dv = float((tv - free["ortho"])[both].abs().max())
            say(f"(a) {side} x {side}: the chain as float64 torch ops on the device {lo:.1f} ms (median {med:.1f}); against the kernels: "
                f"pixels within {dpx:.3g}, values within {dv:.3g} on {int(both.sum())} of {both.numel()} elements")
            for name, fn in (("orthophoto with occlusion", lambda: orthophoto(image, IMAGE, IMAGE, rpc, dsm, grid, ZONE)),
                             ("orthophoto without occlusion", lambda: orthophoto(image, IMAGE, IMAGE, rpc, dsm, grid, ZONE, occlusion=False)),
                             ("orthophoto with occlusion, view_dir given", lambda: orthophoto(image, IMAGE, IMAGE, rpc, dsm, grid, ZONE,
                                                                                              view_dir=res["view_dir"])),
                             ("grid_pixels", lambda: grid_pixels(dsm, grid, rpc, ZONE)),
                             ("sample_image", lambda: sample_image(image, IMAGE, IMAGE, colrow, visible=vis))):
                t, t_med = timed(fn, 5)
                say(f"(b) {side} x {side}: {name}, whole call: {t * 1e3:.2f} ms (median {t_med * 1e3:.2f})")
            rows = max(1, (1 << 16) // side)                      # some 65 k cells of the grid
            host_planes = planes.cpu().numpy()
            t0 = time.time()
            want, _ = O.grid_pixels(d, relief[:rows], xoff, yoff, RES, ZONE)
            O.gather(host_planes, want, None)
            t = time.time() - t0
            dpx = float(np.abs(want - colrow[:rows].cpu().numpy()).max())
            say(f"(c) {side} x {side}: the numpy statement on the host, {rows} rows = {rows * side} cells: {t * 1e3:.1f} ms = "
                f"{t * 1e3 * n / (rows * side):.0f} ms for the grid at that rate; its pixels against the kernel's within {dpx:.3g}")
            del colrow, out, state, res, free, tcr, tv
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
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", "orthophoto_throughput.txt")
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
