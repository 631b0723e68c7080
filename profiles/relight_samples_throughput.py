"""Per-sample relighting throughput: a 512 x 512 synthetic view (262,144 rays), RPV111 + learned normals with --MultiBRDF 1, bf16,
S = G = 64, under K in {1, 8, 64} sun directions.  (a) one render_image - before relight_image(per_sample=True) the only way was K
of them; (b) relight_image(per_sample=True): one geometry pass, each chunk's rows shaded under all K directions and dropped.  Also
the shading launches alone on the rows of the whole view (device events through bn_prof_enable): their BRDF evaluations per second
(R S K per call) and the bytes per second of what they must move - (4 C S + 4 S + 12) R read per direction tile, 12 R K written -
and, in the same process, the per-ray kernel (bn_ray_shade_dirs, R K evaluations) on the same view's composited sums for
comparison.  Output kept in profiles/relight_samples_throughput.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from brdf_nerf_amd import _lib, directions, load_model, relight, relight_image, render_surface  # noqa: E402
from brdf_nerf_amd.evaluate import render_image  # noqa: E402
from brdf_nerf_amd.relight import Surface  # noqa: E402

SAMPLE_KT = 8           # csrc/relight.hip: directions per tile of the per-sample kernel at most


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


def launches_alone(fn, reps=5):
    """Mean device time of the BRDF launches of one fn() call (after a warm-up call), s."""
    fn()
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    for _ in range(reps):
        fn()
    ms, n = _lib.prof_collect()["brdf"]
    _lib.prof_enable(False)
    return ms / reps * 1e-3, n // reps


def main():
    dev = torch.device("cuda", 0)
    N, chunk, config, dtype = 512 * 512, 16384, "rpv_nlr", "bf16"
    ks = [int(k) for k in os.environ.get("RELIGHT_KS", "1,8,64").split(",")]
    rays = bench.synthetic_batch(N, 3, dev)["rays"]
    args = bench.make_args(4096, 64, 64, dtype, **dict(bench.CONFIG_FLAGS[config][0], MultiBRDF=1))
    torch.manual_seed(0)
    models = {"coarse": load_model(args).to(dev)}
    flags = dict(bench.CONFIG_FLAGS[config][1])
    sflags = {k: v for k, v in flags.items() if k in ("apply_brdf", "apply_theta")}
    cosi = flags.get("cos_irra_on", False)
    print(f"view 512 x 512 = {N} rays, {config} MultiBRDF {dtype}, S = G = 64, chunk {chunk}; device {torch.cuda.get_device_name(0)}", flush=True)
    with torch.no_grad():
        t_img, t_img_med = timed(lambda: render_image(models, args, rays, None, keys=("rgb", "depth"), chunk=chunk, **flags), 3)
        print(f"one render_image: {t_img * 1e3:.1f} ms (median {t_img_med * 1e3:.1f}) = {N / t_img / 1e3:.0f} k rays/s", flush=True)
        torch.manual_seed(1)
        surf = render_surface(models, args, rays, chunk=chunk, per_sample=True, **sflags)
        S, C = surf.rows.shape[1], surf.rows.shape[2]
        held = (surf.rows.numel() + surf.weights.numel()) * 4
        print(f"per-sample surface: rows {tuple(surf.rows.shape)} + weights = {held / 1e9:.2f} GB (held only for the launch timings below)", flush=True)
        per_ray = Surface(surf.acc, surf.wsum, surf.depth, surf.rays_d, surf.model, surf.args, surf.spec, surf.apply_brdf, surf.apply_theta)
        for K in ks:
            suns = directions(torch.linspace(15, 75, K), torch.linspace(90, 270, K)).to(dev)
            out = torch.empty((K, N, 3), device=dev)
            tb, tb_med = timed(lambda: relight_image(models, args, rays, suns, chunk=chunk, cos_irra_on=cosi, out=out, per_sample=True,
                                                     **sflags), 3)
            finite = bool(torch.isfinite(out).all())
            t_sh, n_sh = launches_alone(lambda: relight(surf, suns, cos_irra_on=cosi, out=out))
            ktile = min(SAMPLE_KT, max(1, K * ((N + 63) // 64) // 2048))      # the launcher's rule (bn_sample_shade_dirs)
            tiles = (K + ktile - 1) // ktile
            moved = tiles * (4 * C * S + 4 * S + 12) * N + 12 * N * K
            evals = N * S * K
            t_ray, _ = launches_alone(lambda: relight(per_ray, suns, cos_irra_on=cosi, out=out))
            print(f"K = {K}: relight_image(per_sample) {tb * 1e3:.1f} ms (median {tb_med * 1e3:.1f}) against K x render_image = "
                  f"{K * t_img * 1e3:.1f} ms (K x the measured single call) -> {K * t_img / tb:.1f} x; per-sample shading alone "
                  f"{t_sh * 1e3:.3f} ms ({n_sh} launch, mean of 5; {tiles} tile(s) of {ktile}): {evals / 1e6:.1f} M evaluations -> "
                  f"{evals / t_sh / 1e9:.1f} G evaluations/s, {moved / 1e6:.0f} MB to move -> {moved / t_sh / 1e9:.0f} GB/s; per-ray kernel "
                  f"on the same view {t_ray * 1e3:.3f} ms: {N * K / 1e6:.1f} M evaluations -> {N * K / t_ray / 1e9:.1f} G evaluations/s; "
                  f"rgb finite {finite}", flush=True)


if __name__ == "__main__":
    main()
