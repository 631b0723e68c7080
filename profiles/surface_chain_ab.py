"""The surface-model launches of the working tree against the parent commit's, alternating in one process, on the 512 x 512 view
of dsm_throughput.py / ecef_throughput.py / ortho_throughput.py (range 128 m, 0.5 m cells, radius 1, disc), by device events.
The parent's library (python profiles/build_baseline.py HEAD~1 surface_parent, and a copy of it as build/surface_parent2) is
loaded TWICE: the same code against itself is the noise floor.  A library's figure is the median of all its timings; a launch's
spread is the range of the per-round medians of the two parent loads together, i.e. how far the median of a few timings of
IDENTICAL code moves within this run.  The change is meant to move none of these numbers, so the spread is the only margin:
|median(tree) - median(parent)| <= spread, or the launch is OUTSIDE and the script exits 1.  Accumulators are not zeroed between
launches (the timing does not depend on the values).  Writes profiles/surface_chain_ab.txt (or the path given)."""
import os
import sys
from statistics import median

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import torch  # noqa: E402
import bench  # noqa: E402
from dsm_throughput import LINES, say  # noqa: E402
from brdf_nerf_amd import DsmAccumulator, OrthoAccumulator, SceneFrame, load_model  # noqa: E402
from brdf_nerf_amd import _lib as L  # noqa: E402
from brdf_nerf_amd import functions as Fn  # noqa: E402
from brdf_nerf_amd.camera import geo_world  # noqa: E402
from brdf_nerf_amd.dsm import _cloud_grid  # noqa: E402
from brdf_nerf_amd.evaluate import render_image  # noqa: E402

ROUNDS, REPS = 12, 10


def alternate(libs, fn):
    """-> {library name: ROUNDS lists of REPS ms}, the libraries taking turns within a round; round 0 is the warm-up."""
    ts = {k: [] for k in libs}
    for rnd in range(ROUNDS + 1):
        for name, handle in libs.items():
            L.use(handle)
            fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
            for a, b in ev:
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            ts[name] += [[a.elapsed_time(b) for a, b in ev]] if rnd else []
    return ts


@torch.no_grad()
def measure():
    dev = torch.device("cuda", 0)
    N, config = 512 * 512, "rpv_nan"
    rays = bench.synthetic_batch(N, 3, dev)["rays"]
    args = bench.make_args(4096, 64, 64, "bf16", **bench.CONFIG_FLAGS[config][0])
    torch.manual_seed(0)
    models = {"coarse": load_model(args).to(dev)}
    tree = L.lib()
    libs = {"tree": tree}
    for name, tag in (("parent", "surface_parent"), ("parent again", "surface_parent2")):
        libs[name] = L.load(os.path.join(ROOT, "brdf_nerf_amd", "build", tag, "libbrdfnerf_hip.so"), baseline=True)
    say(f"view 512 x 512 = {N} rays, {config} bf16; 0.5 m cells, radius 1 (disc), range 128 m; {ROUNDS} rounds of {REPS} timings per library "
        f"and launch; device {torch.cuda.get_device_name(0)}; source hashes {', '.join(f'{k} {h.bn_source_hash().decode()}' for k, h in libs.items())}")
    utm = SceneFrame((368412.25, 3359871.75, 12.5), 128.0)
    site = geo_world(torch.tensor([[-81.7, 30.3]], dtype=torch.float64), 12.5, cs="ecef", device=dev)[0]      # zone 17
    ecef = SceneFrame.ecef(site.float().tolist(), 128.0)
    torch.manual_seed(1)
    depth = render_image(models, args, rays, None, keys=("depth",), chunk=16384, **dict(bench.CONFIG_FLAGS[config][1]))["depth"]
    acc = {f: DsmAccumulator(_cloud_grid(rays, depth, f, 0.5), dev) for f in (utm, ecef)}

    def world(f, g):
        return lambda: Fn.dsm_splat_world(rays, depth, f.center, f.range, g.xoff, g.yoff, g.resolution, 1, L.BN_DSM_DISC, *f.world_args(),
                                          acc[f].acc, acc[f]._skipped)
    top = OrthoAccumulator(acc[utm].grid, dev, 0, mode="top")
    launches = {"bn_dsm_splat": lambda: acc[utm].add(rays, depth, utm), "bn_dsm_splat_world(cs = utm)": world(utm, acc[utm].grid),
                "bn_dsm_splat_world(cs = ecef)": world(ecef, acc[ecef].grid), "bn_dsm_resolve": acc[utm].result,
                "bn_ortho_top": lambda: Fn.ortho_top(rays, depth, *top._args(utm), top.top, top._top_skipped)}
    g = torch.Generator(device=dev).manual_seed(2)
    for E in (3, 28):
        feats = torch.rand((N, E), generator=g, device=dev) * 2 - 0.5
        o = OrthoAccumulator(acc[utm].grid, dev, E, mode="mean")
        launches[f"bn_ortho_splat(E = {E})"] = lambda o=o, feats=feats: o.add(rays, depth, utm, feats)
        launches[f"bn_ortho_resolve(E = {E})"] = o.result
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
        with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "surface_chain_ab.txt"), "w") as f:
            f.write("\n".join(LINES) + "\n")
    sys.exit(1 if bad else 0)
