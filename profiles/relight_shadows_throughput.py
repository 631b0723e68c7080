"""Relighting with cast shadows, throughput: a 512 x 512 synthetic view (262,144 rays), RPV111 + analytic normals with
--sun_v analystic, gsam_only, bf16, S = G = 64, under K in {1, 8, 64} sun directions.  (a) one render_image(gsam_only=True) -
before relight_image_shadowed the only way was K of them; (b) relight_image_shadowed: one geometry pass + K R G sigma-only points.
Also, on one chunk of 16,384 rays (device events): the bn_sun_ray_table and bn_sun_shade_dirs launches alone, the bytes they must
move (table: 4 (8 + G) K R written, 4 G R read; shading: 8 K R G read, 16 K R written) and their GB/s, and the same two steps done
the way they replace - per direction rendering.sun_far + Fn.stratified_z + torch.cat, and Fn.composite + the torch statement of
shade() (irradiance of the last sample times the BRDF, clamped).  Ends with bench.py's box-speed indicator.  Output kept in
profiles/relight_shadows_throughput.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from brdf_nerf_amd import _lib, directions, functions as Fn, load_model, relight_image_shadowed, render_shadow_surface  # noqa: E402
from brdf_nerf_amd.evaluate import render_image  # noqa: E402
from brdf_nerf_amd.rendering import sun_far  # noqa: E402


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


def device_time(fn, reps=5):
    """Mean device time of fn() between two events (after a warm-up call), s."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def launch_alone(fn, kernel, reps=5):
    """Mean device time of one library kernel class inside fn() (bn_prof_enable), s."""
    fn()
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    for _ in range(reps):
        fn()
    ms, n = _lib.prof_collect()[kernel]
    _lib.prof_enable(False)
    return ms / reps * 1e-3, n // reps


def main():
    dev = torch.device("cuda", 0)
    N, chunk, dtype = 512 * 512, 16384, "bf16"
    ks = [int(k) for k in os.environ.get("RELIGHT_KS", "1,8,64").split(",")]
    rays = bench.synthetic_batch(N, 3, dev)["rays"]
    args = bench.make_args(4096, 64, 64, dtype, sun_v="analystic", **bench.CONFIG_FLAGS["rpv_nan"][0])
    torch.manual_seed(0)
    models = {"coarse": load_model(args).to(dev)}
    model = models["coarse"]
    S, G = args.n_samples, args.guided_samples
    print(f"view 512 x 512 = {N} rays, rpv_nan + --sun_v analystic {dtype}, gsam_only, S = G = {G}, chunk {chunk}; device "
          f"{torch.cuda.get_device_name(0)}", flush=True)
    print(f"field points per extra sun: {S + G} sigma-only + {G} full (render_image) -> {G} sigma-only (relight_image_shadowed)", flush=True)
    with torch.no_grad():
        t_img, t_img_med = timed(lambda: render_image(models, args, rays, None, keys=("rgb", "depth"), chunk=chunk, apply_brdf=True,
                                                      gsam_only=True), 3)
        print(f"one render_image(gsam_only=True): {t_img * 1e3:.1f} ms (median {t_img_med * 1e3:.1f}) = {N / t_img / 1e3:.0f} k rays/s", flush=True)
        torch.manual_seed(1)
        surf = render_shadow_surface(models, args, rays[:chunk])
        R, C = surf.n_rays, surf.spec.out_channels
        desc = surf.desc()
        sigma_spec, named = model.spec(False, False, False, False), model.named()
        for K in ks:
            suns = directions(torch.linspace(15, 75, K), torch.linspace(90, 270, K)).to(dev)
            out = torch.empty((K, N, 3), device=dev)
            tb, tb_med = timed(lambda: relight_image_shadowed(models, args, rays, suns, chunk=chunk, out=out), 3)
            finite = bool(torch.isfinite(out).all())
            del out
            # one chunk: the two launches alone, and the path they replace
            t_tab, _ = launch_alone(lambda: Fn.sun_ray_table(surf.rays, surf.d1, suns, surf.u_sun), "stratified_z")
            table, z_sun = Fn.sun_ray_table(surf.rays, surf.d1, suns, surf.u_sun)
            sigma = Fn.field_sigma(sigma_spec, named, surf.packed, rays=table, z=z_sun)
            t_field = device_time(lambda: Fn.field_sigma(sigma_spec, named, surf.packed, rays=table, z=z_sun))
            rgb, vis = Fn.sun_shade_dirs(desc, sigma, z_sun, surf.rays_d, suns, acc=surf.acc, wsum=surf.wsum, want_vis=True)
            t_sh, _ = launch_alone(lambda: Fn.sun_shade_dirs(desc, sigma, z_sun, surf.rays_d, suns, acc=surf.acc, wsum=surf.wsum, rgb=rgb,
                                                             vis=vis), "brdf")
            _, brdf = Fn.ray_shade_dirs(desc, surf.acc, surf.wsum, surf.rays_d, suns, want_brdf=True)
            sig3, z3 = sigma.view(K, R, G), z_sun.view(K, R, G)

            def old_table():
                for k in range(K):
                    sun_d = suns[k].expand(R, 3)
                    far = sun_far(surf.d1, surf.rays_d, sun_d)
                    Fn.stratified_z(far * 0.01, far, surf.u_sun)
                    torch.cat([surf.rays[:, 0:3] + surf.rays_d * surf.d1.unsqueeze(-1), sun_d], -1).contiguous()

            def old_shade():
                for k in range(K):
                    _, T, _, _ = Fn.composite(z3[k], sig3[k], None, 0.0)
                    (T[:, -1:] * brdf[k]).clamp(0.0, 1.0)
            t_old_tab, t_old_sh = device_time(old_table), device_time(old_shade)
            mv_tab = 4 * (8 + G) * K * R + 4 * G * R
            mv_sh = 8 * K * R * G + 16 * K * R + 4 * (C + 4) * R
            print(f"K = {K}: relight_image_shadowed {tb * 1e3:.1f} ms (median {tb_med * 1e3:.1f}) against K x render_image = "
                  f"{K * t_img * 1e3:.1f} ms (K x the measured single call) -> {K * t_img / tb:.2f} x; rgb finite {finite}", flush=True)
            print(f"    one chunk of {R} rays: bn_sun_ray_table {t_tab * 1e6:.1f} us ({mv_tab / 1e6:.1f} MB -> {mv_tab / t_tab / 1e9:.0f} GB/s) "
                  f"against sun_far + stratified_z + cat per direction {t_old_tab * 1e6:.1f} us; bn_field_sigma on {K * R * G / 1e6:.1f} M "
                  f"points {t_field * 1e3:.3f} ms; bn_sun_shade_dirs {t_sh * 1e6:.1f} us ({mv_sh / 1e6:.1f} MB -> {mv_sh / t_sh / 1e9:.0f} GB/s) "
                  f"against Fn.composite + torch shading per direction {t_old_sh * 1e6:.1f} us", flush=True)
            del table, z_sun, sigma, rgb, vis, brdf, sig3, z3
    cal = bench.box_calibration(dev, when="after everything that is timed")
    print(f"# box-speed indicator (bench.py box_calibration): {cal.get('tflops', float('nan')):.1f} TFLOP/s, {cal.get('kind', cal)}", flush=True)


if __name__ == "__main__":
    main()
