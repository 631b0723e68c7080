"""Relighting throughput: a 512 x 512 synthetic view (262,144 rays), RPV111 + analytic normals, bf16, under K in {1, 8, 64} sun
directions.  (a) K calls of render_image with the sun written into rays[:, 8:11] - the only way before relight_image, the
baseline; (b) relight_image: one geometry pass + one shading launch per direction tile.  Also the shading launches alone (device
events through bn_prof_enable) and their achieved bytes per second against the bytes they must move: 4 C R read per direction
tile (+ 4 R wsum + 12 R rays_d), 12 R K written.  Output kept in profiles/relight_throughput.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from brdf_nerf_amd import _lib, directions, load_model, relight, relight_image, render_surface  # noqa: E402
from brdf_nerf_amd.evaluate import render_image  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        ts.append(time.time() - t0)
    return min(ts), sorted(ts)[len(ts) // 2]


def main():
    dev = torch.device("cuda", 0)
    N, chunk, config, dtype = 512 * 512, 16384, "rpv_nan", "bf16"
    ks = [int(k) for k in os.environ.get("RELIGHT_KS", "1,8,64").split(",")]
    b = bench.synthetic_batch(N, 3, dev)
    rays = b["rays"]
    args = bench.make_args(4096, 64, 64, dtype, **bench.CONFIG_FLAGS[config][0])
    torch.manual_seed(0)
    models = {"coarse": load_model(args).to(dev)}
    flags = dict(bench.CONFIG_FLAGS[config][1])
    sflags = {k: v for k, v in flags.items() if k in ("apply_brdf", "apply_theta")}
    cosi = flags.get("cos_irra_on", False)
    print(f"view 512 x 512 = {N} rays, {config} {dtype}, S = G = 64, chunk {chunk}; device {torch.cuda.get_device_name(0)}", flush=True)
    with torch.no_grad():
        t_img, t_img_med = timed(lambda: render_image(models, args, rays, None, keys=("rgb", "depth"), chunk=chunk, **flags), 3)
        print(f"one render_image: {t_img * 1e3:.1f} ms (median {t_img_med * 1e3:.1f}) = {N / t_img / 1e3:.0f} k rays/s", flush=True)
        torch.manual_seed(1)
        surf = render_surface(models, args, rays, chunk=chunk, **sflags)
        C = surf.acc.shape[1]
        for K in ks:
            suns = directions(torch.linspace(15, 75, K), torch.linspace(90, 270, K)).to(dev)

            def per_direction():
                r = rays.clone()
                for k in range(K):
                    r[:, 8:11] = suns[k]
                    render_image(models, args, r, None, keys=("rgb", "depth"), chunk=chunk, **flags)
            ta, _ = timed(per_direction, 2 if K <= 8 else 1)          # (timed() runs it once more first, as warm-up)
            out = torch.empty((K, N, 3), device=dev)
            tb, tb_med = timed(lambda: relight_image(models, args, rays, suns, chunk=chunk, cos_irra_on=cosi, out=out, **sflags), 3)
            relight(surf, suns, cos_irra_on=cosi, out=out)
            torch.cuda.synchronize()
            _lib.prof_enable(True)
            for _ in range(5):
                relight(surf, suns, cos_irra_on=cosi, out=out)
            ms, n = _lib.prof_collect()["brdf"]
            _lib.prof_enable(False)
            t_sh = ms / n * 1e-3
            ktile = min(32, max(1, K * ((N + 63) // 64) // 2048))      # the launcher's rule (csrc/relight.hip, bn_ray_shade_dirs)
            tiles = (K + ktile - 1) // ktile
            moved = tiles * (4 * C + 4 + 12) * N + 12 * N * K
            print(f"K = {K}: (a) K calls of render_image {ta * 1e3:.1f} ms; (b) relight_image {tb * 1e3:.1f} ms (median {tb_med * 1e3:.1f}) "
                  f"-> {ta / tb:.1f} x; shading launch alone {t_sh * 1e3:.3f} ms (mean of {n}), {tiles} tile(s) of {ktile}, {moved / 1e6:.1f} MB to move "
                  f"-> {moved / t_sh / 1e9:.0f} GB/s; rgb finite {bool(torch.isfinite(out).all())}", flush=True)


if __name__ == "__main__":
    main()
