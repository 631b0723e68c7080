"""Metric throughput on a 512 x 512 view: (a) bn_ssim_map with windows 3 and 11 (three planes, with the float32 map and without)
against the same computation as torch ops on the device - F.pad(mode='reflect') + F.conv2d in float64; (b) bn_grid_normals +
bn_normal_angle on a 512 x 512 DSM against the four-cross-product normals and the angle in torch float64; (c) score_view (render,
PSNR, two SSIM launches, DSM, altitude and normal-angle MAE) against render_image alone, RPV111 + analytic normals, bf16.  Kernel
times by device events, view times by a host clock around a synchronise.  Ends with bench.py in a child process as the box-speed
indicator of the visit.  Writes profiles/metrics_throughput.txt (or the path given as the first argument).  Nothing here is a gate."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import bench  # noqa: E402
from dsm_throughput import LINES, device_ms, say, timed  # noqa: E402
from brdf_nerf_amd import SceneFrame, dsm_image, load_model, score_view  # noqa: E402
from brdf_nerf_amd import functions as Fn  # noqa: E402
from brdf_nerf_amd.evaluate import render_image  # noqa: E402
from brdf_nerf_amd.metrics import gaussian_window  # noqa: E402


def torch_ssim(x, y, window, max_val):
    """(3, H, W) float32 planes -> SSIM index map in float64 by reflect padding and conv2d."""
    g = torch.tensor(gaussian_window(window), dtype=torch.float64, device=x.device)
    k = torch.outer(g, g).reshape(1, 1, window, window)
    pad = window // 2
    f = lambda t: F.conv2d(F.pad(t.unsqueeze(1), (pad,) * 4, mode="reflect"), k).squeeze(1)
    x, y = x.double(), y.double()
    mx, my, exx, eyy, exy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    C1, C2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2) + 1e-12)


def torch_normals(z, res):
    eps = torch.tensor(2.0 ** -23, dtype=torch.float64, device=z.device)
    unit = lambda v: v / torch.sqrt(torch.maximum((v ** 2).sum(-1, keepdim=True), eps))
    H, W = z.shape
    r, c = torch.meshgrid(torch.arange(H, device=z.device, dtype=torch.float64), torch.arange(W, device=z.device, dtype=torch.float64),
                          indexing="ij")
    P = torch.stack([c * res, r * res, z.double()], -1)
    o = P[1:-1, 1:-1]
    S, N, E, Wv = unit(P[2:, 1:-1] - o), unit(P[:-2, 1:-1] - o), unit(P[1:-1, 2:] - o), unit(P[1:-1, :-2] - o)
    cr = lambda a, b: torch.linalg.cross(a, b)
    n = unit((unit(cr(E, N)) + unit(cr(Wv, S)) + unit(cr(N, Wv)) + unit(cr(S, E))) / 4.0)
    out = torch.zeros((H, W, 3), dtype=torch.float64, device=z.device)
    out[1:-1, 1:-1] = n
    return out.float()


def torch_angle(n1, n2):
    a = torch.acos((n1.double() * n2.double()).sum(-1).clamp(-1, 1)) * 180.0 / torch.pi
    return a, torch.nanmean(a)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "metrics_throughput.txt")
    dev = torch.device("cuda", 0)
    H = W = 512
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(3, H, W, generator=g).to(dev)
    pred = (gt + 0.1 * torch.randn(3, H, W, generator=g).to(dev)).clamp(0, 1)
    say(f"view {H} x {W}, 3 planes; device {torch.cuda.get_device_name(0)}")
    max_val = float(gt.max())
    for window in (3, 11):
        gw = gaussian_window(window)
        sums = torch.zeros(3, dtype=torch.int64, device=dev)
        out = torch.empty(3, H, W, device=dev)
        k_ms, k_med = device_ms(lambda: Fn.ssim_map(pred, gt, 3, H, W, (H * W, W, 1), None, 1.0, max_val, window, gw, sums, out=out))
        n_ms, n_med = device_ms(lambda: Fn.ssim_map(pred, gt, 3, H, W, (H * W, W, 1), None, 1.0, max_val, window, gw, sums))
        t_ms, t_med = device_ms(lambda: torch_ssim(pred, gt, window, max_val).mean(), 10)
        sums.zero_()
        Fn.ssim_map(pred, gt, 3, H, W, (H * W, W, 1), None, 1.0, max_val, window, gw, sums, out=out)
        s = [int(v) for v in sums.cpu()]
        ref = torch_ssim(pred, gt, window, max_val)
        taps = 3 * H * W * window * window
        say(f"(a) bn_ssim_map window {window}: {k_ms:.3f} ms with the map (median {k_med:.3f}), {n_ms:.3f} ms without (median {n_med:.3f}) = "
            f"{taps / n_ms / 1e6:.1f} G taps/s; torch float64 pad + conv2d {t_ms:.3f} ms (median {t_med:.3f}) -> {t_ms / k_ms:.1f} x; "
            f"ssim {s[0] / (s[1] * 2.0 ** 30):.9f} (torch mean {float(ref.mean()):.9f}), max |map difference| {float((ref - out.double()).abs().max()):.2e}, skipped {s[2]}")
    z1 = (30.0 + 2.0 * torch.randn(H, W, generator=g)).to(dev)
    z2 = (z1 + 0.3 * torch.randn(H, W, generator=g).to(dev)).contiguous()
    n_ms, n_med = device_ms(lambda: Fn.grid_normals(z1, 0.5))
    n1, n2 = Fn.grid_normals(z1, 0.5), Fn.grid_normals(z2, 0.5)
    a_ms, a_med = device_ms(lambda: Fn.normal_angle(n1, n2))
    tn_ms, tn_med = device_ms(lambda: torch_normals(z1, 0.5), 10)
    ta_ms, ta_med = device_ms(lambda: torch_angle(n1, n2), 10)
    angle, sums = Fn.normal_angle(n1, n2)
    s = [int(v) for v in sums.cpu()]
    say(f"(b) bn_grid_normals {n_ms:.3f} ms (median {n_med:.3f}), bn_normal_angle {a_ms:.3f} ms (median {a_med:.3f}) on a {H} x {W} DSM; torch "
        f"float64 normals {tn_ms:.3f} ms (median {tn_med:.3f}), angle + nanmean {ta_ms:.3f} ms (median {ta_med:.3f}) -> "
        f"{(2 * tn_ms + ta_ms) / (2 * n_ms + a_ms):.1f} x for two grids and the angle; mae_nr {s[0] / (s[1] * 2.0 ** 20):.6f} deg (torch "
        f"{float(torch_angle(n1, n2)[1]):.6f}), max |normal difference| {float((torch_normals(z1, 0.5) - n1).abs().max()):.2e}")

    N, chunk, config, dtype = H * W, 16384, "rpv_nan", "bf16"
    rays = bench.synthetic_batch(N, 3, dev)["rays"]
    args = bench.make_args(4096, 64, 64, dtype, **bench.CONFIG_FLAGS[config][0])
    torch.manual_seed(0)
    models = {"coarse": load_model(args).to(dev)}
    flags = dict(bench.CONFIG_FLAGS[config][1])
    rgbs = gt.permute(1, 2, 0).reshape(N, 3).contiguous()
    mask = torch.rand(H, W, generator=g).to(dev) < 0.9
    frame = SceneFrame((368412.25, 3359871.75, 12.5), 128.0)
    with torch.no_grad():
        first = dsm_image(models, args, rays, frame, chunk=chunk, **flags)
        grid = first["grid"]
        gt_dsm = torch.nan_to_num(first["dsm"], nan=12.5) + 0.3 * torch.randn(first["dsm"].shape, generator=g).to(dev)
        t_img, t_img_med = timed(lambda: render_image(models, args, rays, rgbs, keys=("rgb", "depth"), chunk=chunk, **flags), 3)
        t_sc, t_sc_med = timed(lambda: score_view(models, args, rays, rgbs, H, W, mask=mask, frame=frame, gt_dsm=gt_dsm, grid=grid,
                                                   chunk=chunk, **flags), 3)
        t_im, t_im_med = timed(lambda: score_view(models, args, rays, rgbs, H, W, mask=mask, chunk=chunk, **flags), 3)
        res = score_view(models, args, rays, rgbs, H, W, mask=mask, frame=frame, gt_dsm=gt_dsm, grid=grid, chunk=chunk, **flags)
    say(f"(c) {config} {dtype}, S = G = 64, chunk {chunk}; DSM grid {grid.width} x {grid.height} at 0.5 m: render_image {t_img * 1e3:.1f} ms (median "
        f"{t_img_med * 1e3:.1f}); score_view, image numbers only {t_im * 1e3:.1f} ms (median {t_im_med * 1e3:.1f}) -> {(t_im - t_img) * 1e3:+.1f} ms; "
        f"with the DSM, mae and mae_nr {t_sc * 1e3:.1f} ms (median {t_sc_med * 1e3:.1f}) -> {(t_sc - t_img) * 1e3:+.1f} ms on render_image")
    say("    " + ", ".join(f"{k} {res[k]:.4f}" for k in ("psnr", "psnr_scl", "ssim", "ssim_scl", "mae", "mae_nr")) + f", ssim_skipped {res['ssim_skipped']}")
    del models
    torch.cuda.empty_cache()
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
