"""Validation-map throughput on a 512 x 512 view (RPV111 + analytic normals, bf16, S = G = 64): (a) render_image alone, view_maps,
and view_maps with a frame (altitude, nr_from_depth), by a host clock around a synchronise, with the peak device memory of each;
(b) bn_ray_maps alone on one chunk's field rows (counts of the normal column only, and with accum over all channels) and
bn_point_normals alone on the view's points, by device events, with the achieved GB/s of the bytes they must read; (c) the same
maps the per-sample way: render_image(keys=...) concatenating the per-sample tensors of the whole view, then torch on the device
- argmin, gather in place of the reference's Python double loop, the float64 variance, the normal counts - with its peak memory.
Ends with bench.py in a child process as the box-speed indicator of the visit.  Writes profiles/maps_throughput.txt (or the path
given as the first argument).  Nothing here is a gate."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import torch  # noqa: E402
import bench  # noqa: E402
from dsm_throughput import LINES, device_ms, say, timed  # noqa: E402
from brdf_nerf_amd import SceneFrame, load_model, point_cloud, view_maps  # noqa: E402
from brdf_nerf_amd import functions as Fn  # noqa: E402
from brdf_nerf_amd.evaluate import render_image  # noqa: E402

PER_SAMPLE = ("rgb", "depth", "z_vals", "weights", "sigmas", "alphas", "transparency", "normal_an", "rays_d")


def torch_maps(models, args, rays, chunk, flags):
    """The maps from the per-sample tensors of the WHOLE view, torch on the device."""
    v = render_image(models, args, rays, None, keys=PER_SAMPLE, chunk=chunk, **flags)
    z, w, depth = v["z_vals"], v["weights"], v["depth"]
    idx = torch.argmin(torch.abs(z - depth.unsqueeze(-1)), dim=1, keepdim=True)
    surf = [t.reshape(z.shape[0], z.shape[1]).gather(1, idx) for t in (v["sigmas"], v["alphas"], v["transparency"], w)]
    std = (((z.double() - depth.double().unsqueeze(-1)) ** 2) * w.double()).sum(-1).sqrt().float()
    n = v["normal_an"].double()
    bad = ((n * v["rays_d"].double()).sum(-1) < 0).sum()
    nr0 = (~(n.pow(2).sum(-1).sqrt() > 0.99999)).sum()
    return idx, surf, std, float(std.mean()), int(bad), int(nr0)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "maps_throughput.txt")
    dev = torch.device("cuda", 0)
    H = W = 512
    N, chunk, config, dtype = H * W, 16384, "rpv_nan", "bf16"
    rays = bench.synthetic_batch(N, 3, dev)["rays"]
    args = bench.make_args(4096, 64, 64, dtype, **bench.CONFIG_FLAGS[config][0])
    torch.manual_seed(0)
    models = {"coarse": load_model(args).to(dev)}
    flags = dict(bench.CONFIG_FLAGS[config][1])
    frame = SceneFrame((368412.25, 3359871.75, 12.5), 128.0)
    say(f"view {H} x {W} = {N} rays, {config} {dtype}, S = G = 64, chunk {chunk}; device {torch.cuda.get_device_name(0)}")
    with torch.no_grad():
        t_img, t_img_med = timed(lambda: render_image(models, args, rays, None, keys=("rgb", "depth"), chunk=chunk, **flags), 3)
        t_map, t_map_med = timed(lambda: view_maps(models, args, rays, H, W, chunk=chunk, **flags), 3)
        t_frm, t_frm_med = timed(lambda: view_maps(models, args, rays, H, W, frame=frame, chunk=chunk, **flags), 3)
        t_tor, t_tor_med = timed(lambda: torch_maps(models, args, rays, chunk, flags), 3)
        _, m_img = peak(lambda: render_image(models, args, rays, None, keys=("rgb", "depth"), chunk=chunk, **flags))
        got, m_map = peak(lambda: view_maps(models, args, rays, H, W, frame=frame, chunk=chunk, **flags))
        _, m_tor = peak(lambda: torch_maps(models, args, rays, chunk, flags))
        say(f"(a) render_image {t_img * 1e3:.1f} ms (median {t_img_med * 1e3:.1f}), peak {m_img:.0f} MiB; view_maps {t_map * 1e3:.1f} ms (median "
            f"{t_map_med * 1e3:.1f}) -> {(t_map - t_img) * 1e3:+.1f} ms; with a frame {t_frm * 1e3:.1f} ms (median {t_frm_med * 1e3:.1f}) -> "
            f"{(t_frm - t_img) * 1e3:+.1f} ms, peak {m_map:.0f} MiB = {m_map - m_img:+.0f} MiB on render_image; {len(got['maps'])} maps; stats " +
            ", ".join(f"{k} {v:.4f}" for k, v in got["stats"].items() if isinstance(v, float)))
        say(f"(c) the per-sample way (render_image(keys=...) of {len(PER_SAMPLE)} keys + torch argmin / gather / float64 variance / counts): "
            f"{t_tor * 1e3:.1f} ms (median {t_tor_med * 1e3:.1f}) -> {(t_tor - t_img) * 1e3:+.1f} ms on render_image, peak {m_tor:.0f} MiB "
            f"= {m_tor - m_img:+.0f} MiB on render_image")
        # (b) the kernels alone, on tensors of one chunk's shapes
        g = torch.Generator().manual_seed(1)
        S, C = 128, 28
        z = torch.sort(torch.rand(chunk, S, generator=g), dim=1).values.to(dev)
        w = torch.rand(chunk, S, generator=g).to(dev) / S
        depth = (z * w).sum(-1).contiguous()
        X = torch.randn(chunk, S, C, generator=g).to(dev)
        view = torch.randn(chunk, 3, generator=g).to(dev)
        cnt = torch.zeros(6, dtype=torch.int64, device=dev)
        for what, fn, nbytes in (
                ("no X", lambda: Fn.ray_maps(z, w, depth, None, False, None, None, cnt), chunk * S * 8),
                ("X of 28 channels, surface row + normal counts (three channels staged)",
                 lambda: Fn.ray_maps(z, w, depth, X, False, 4, view, cnt), chunk * S * (12 + 3 * 4)),
                ("X of 28 channels, accum + surface row + normal counts (all channels staged)",
                 lambda: Fn.ray_maps(z, w, depth, X, True, 4, view, cnt), chunk * S * (12 + C * 4))):
            ms, med = device_ms(fn)
            say(f"(b) bn_ray_maps, {chunk} rays x {S} samples, {what}: {ms:.3f} ms (median {med:.3f}) = {nbytes / ms / 1e6:.0f} GB/s of the "
                f"{nbytes / 2 ** 20:.0f} MiB it must read")
        pts = point_cloud(rays, got["maps"]["depth"], frame).reshape(H, W, 3).contiguous()
        for rf in (True, False):
            ms, med = device_ms(lambda: Fn.point_normals(pts, None, rf))
            say(f"(b) bn_point_normals {H} x {W}, round_f32 = {int(rf)}: {ms:.3f} ms (median {med:.3f}) = {(N * 24 + N * 12) / ms / 1e6:.0f} GB/s of "
                f"the points read once and the normals written")
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
