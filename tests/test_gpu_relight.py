"""GPU tests of relighting (brdf_nerf_amd/relight.py, bn_ray_shade_dirs): K sun directions and BRDF lobes from ONE geometry pass.
Run on the MI355X box with `pytest -m gpu`.  Cases, directions and the oracle statement: tests/relight_cases.py."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import assert_close
import relight_cases as RC
from test_gpu_parity import DEV, _free_port, make_args

pytestmark = pytest.mark.gpu
R_TEST = 300            # not a multiple of the kernel's 64-ray block


def build(name, dtype="fp32", level=False, **cfg_kw):
    """Model and rays of a case, built as tests/test_gpu_parity.py builds its own (make_args, make_params, synthetic_table).
    level=True: the learned-normal head gets the bias of level ground (relight_cases.level_normals)."""
    from brdf_nerf_amd import load_model
    from brdf_nerf_amd.raytable import synthetic_table
    cfg = RC.config(name, **cfg_kw)
    args = make_args(cfg, dtype)
    model = load_model(args)
    sd = {k: torch.from_numpy(v) for k, v in cfg.make_params(RC.MODEL_SEED).items()}
    model.load_state_dict(RC.level_normals(sd) if level else sd)
    rays = synthetic_table(R_TEST, device=DEV, seed=RC.RAYS_SEED).data["rays"].clone()
    return cfg, args, {"coarse": model.to(DEV)}, rays


def flags(name):
    fl = RC.CASES[name][1]
    return dict(apply_brdf=fl.get("apply_brdf", False), apply_theta=fl.get("apply_theta", False)), fl.get("cos_irra_on", False)


@pytest.mark.parametrize("name,dtype", [(n, "fp32") for n in RC.CASES] + [("rpv111", "bf16")])
def test_relight_image_matches_render_rays_per_direction(name, dtype):
    """Against the product path: for each of the K suns, reseed, write the sun into rays[:, 8:11] and call render_rays; reseed and
    call relight_image once with all K.  rgb[k] matches rgb_coarse of call k to assert_close's defaults (the project's bound for
    end-to-end rgb in fp32 mode); depth is the same computation on the same draws: equal bit for bit."""
    from brdf_nerf_amd import relight_image, render_rays
    cfg, args, models, rays = build(name, dtype)
    fl, cosi = flags(name)
    suns = RC.sun_directions().to(DEV)
    assert suns.shape[0] >= 5
    torch.manual_seed(17)
    got = relight_image(models, args, rays, suns, cos_irra_on=cosi, **fl)
    assert tuple(got["rgb"].shape) == (suns.shape[0], R_TEST, 3)
    for k in range(suns.shape[0]):
        r = rays.clone()
        r[:, 8:11] = suns[k]
        torch.manual_seed(17)
        with torch.no_grad():
            want, _ = render_rays(models, args, r, None, mode="test", cos_irra_on=cosi, **fl)
        err = float((got["rgb"][k] - want["rgb_coarse"]).abs().max())
        print(f"{name} {dtype} sun {k}: max |rgb - rgb_coarse| = {err:.3e}")
        assert_close(got["rgb"][k], want["rgb_coarse"], msg=f"{name} rgb[{k}]")
        assert torch.equal(got["depth"], want["depth_coarse"]), f"{name} depth, sun {k}"


@pytest.mark.parametrize("name", list(RC.CASES))
def test_kernel_matches_oracle_brdf_in_sun_and_lobe_mode(name):
    """Against oracle/brdf.py, independent of the product's shading code: from the surface's acc / wsum (copied to the CPU,
    float64) the expected BRDF and rgb of every (ray, direction), compared with both outputs of the kernel at the tolerance of
    the per-point parity test of the same BRDF kind (test_gpu_parity.py test_brdf_*_golden).  Every entry is compared; the
    oracle's values are asserted finite."""
    from brdf_nerf_amd import relight, render_surface
    cfg, args, models, rays = build(name, level=True)
    fl, cosi = flags(name)
    rtol, atol = RC.ORACLE_TOL[RC.CASES[name][2]]
    torch.manual_seed(3)
    surf = render_surface(models, args, rays, **fl)
    lobe = RC.lobe_directions()
    lobe_sun = torch.tensor([RC.unit(*RC.LOBE_SUN)], dtype=torch.float32)
    for mode, sun, view in (("sun", RC.sun_directions(), None), ("lobe", lobe_sun.expand(lobe.shape[0], 3), lobe)):
        rgb, brdf = relight(surf, sun, cos_irra_on=cosi, view_dirs=view, want_brdf=True, **{"apply_brdf": fl["apply_brdf"]})
        want_rgb, want_brdf = RC.oracle_shade(cfg, surf.acc, surf.wsum, surf.rays_d, sun, view, fl["apply_brdf"], fl["apply_theta"], cosi)
        assert bool(torch.isfinite(want_rgb).all()) and bool(torch.isfinite(want_brdf).all()), f"{name} {mode}: oracle not finite"
        e = (brdf.cpu().double() - want_brdf).abs()
        print(f"{name} {mode}: brdf max abs err {float(e.max()):.3e}, max err/tol {float((e / (atol + rtol * want_brdf.abs())).max()):.3f}")
        assert_close(brdf, want_brdf, rtol, atol, f"{name} {mode} brdf")
        assert_close(rgb, want_rgb, rtol, atol, f"{name} {mode} rgb")


def test_field_is_evaluated_once():
    """relight_image with K = 8 calls the model's evaluate exactly as often as ONE render_image of the same rays and chunk."""
    from brdf_nerf_amd import relight_image
    from brdf_nerf_amd.evaluate import render_image
    cfg, args, models, rays = build("rpv111")
    fl, cosi = flags("rpv111")
    model = models["coarse"]
    calls = []
    orig = model.evaluate
    model.evaluate = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    render_image(models, args, rays, chunk=100, cos_irra_on=cosi, **fl)
    n_image = len(calls)
    del calls[:]
    suns = torch.cat([RC.sun_directions(), RC.sun_directions()[:2]]).to(DEV)
    assert suns.shape[0] == 8
    relight_image(models, args, rays, suns, chunk=100, cos_irra_on=cosi, **fl)
    assert n_image == 6 and len(calls) == n_image, (n_image, len(calls))      # 3 chunks x (pass 1 + guided samples)


def _synthetic_surface(name, R, seed):
    """A Surface with made-up composited sums (level ground with tilted normals, parameters inside their heads' ranges): the
    tiling tests need many rays, not a render."""
    from brdf_nerf_amd.relight import Surface
    cfg, args, models, _ = build(name)
    fl, _ = flags(name)
    model = models["coarse"]
    spec = model.spec(fl["apply_brdf"], fl["apply_theta"], model.normal in ("analystic_learned", "learned"),
                      model.normal in ("analystic_learned", "analystic"))
    g = torch.Generator().manual_seed(seed)
    acc = 0.1 + 0.8 * torch.rand(R, spec.out_channels, generator=g)
    ch = RC.channels(cfg, fl["apply_brdf"], fl["apply_theta"])
    n = torch.cat([0.3 * torch.randn(R, 2, generator=g), torch.ones(R, 1)], -1)
    acc[:, ch["normal"]:ch["normal"] + 3] = n
    d = torch.cat([0.2 * torch.randn(R, 2, generator=g), -torch.ones(R, 1)], -1)
    d = d / d.norm(dim=-1, keepdim=True)
    wsum = 0.9 + 0.1 * torch.rand(R, generator=g)
    return Surface(acc.to(DEV), wsum.to(DEV), torch.rand(R, generator=g).to(DEV), d.to(DEV).contiguous(), model, args, spec,
                   fl["apply_brdf"], fl["apply_theta"])


@pytest.mark.parametrize("name", ["rpv111", "hapke_bct"])
def test_tiling_is_invisible(name):
    """Every (direction, ray) is computed on its own: K = 1, K = one kernel tile (32 directions) + 1 with R not a multiple of the
    64-ray block, `out=` on the device and on the host, and relight over direction tiles all give bitwise the rows of one call;
    brdf_lobe on picked rows equals relight in lobe mode on those rows."""
    from brdf_nerf_amd import brdf_lobe, directions, relight
    R, K = 130001, 33                                   # 2032 ray blocks x 33 directions: the kernel takes tiles of 32
    surf = _synthetic_surface(name, R, 5)
    suns = directions(torch.linspace(25, 80, K), torch.linspace(0, 330, K)).to(DEV)
    assert suns.shape == (K, 3)
    whole, whole_b = relight(surf, suns, cos_irra_on=True, want_brdf=True)
    bits = lambda t: t.contiguous().view(torch.int32)               # bitwise, NaN payloads included
    equal = lambda a, b: a.shape == b.shape and torch.equal(bits(a), bits(b))
    for k in (0, 16, 32):                                # K = 1: one direction per launch
        one, one_b = relight(surf, suns[k:k + 1], cos_irra_on=True, want_brdf=True)
        assert equal(one[0], whole[k]) and equal(one_b[0], whole_b[k]), k
    assert equal(relight(surf, suns, cos_irra_on=True, dir_tile=7), whole)
    out = torch.full((K, R, 3), -1.0, device=DEV)
    assert relight(surf, suns, cos_irra_on=True, out=out) is out and equal(out, whole)
    host = torch.full((K, R, 3), -1.0)
    assert relight(surf, suns, cos_irra_on=True, out=host, dir_tile=5) is host and equal(host, whole.cpu())
    small = surf.select(slice(0, 70))                    # few rays: one direction per tile in the kernel
    assert equal(relight(small, suns, cos_irra_on=True), whole[:, :70])
    rows = torch.tensor([3, 64, 65, 129999, 130000])
    views, sun = RC.lobe_directions().to(DEV), torch.tensor(RC.unit(*RC.LOBE_SUN))
    lobe_b, lobe_rgb = brdf_lobe(surf, rows, views, sun, cos_irra_on=True)
    assert tuple(lobe_b.shape) == (5, views.shape[0], 3)
    ref_rgb, ref_b = relight(surf, sun, cos_irra_on=True, view_dirs=views, want_brdf=True)
    assert equal(lobe_b, ref_b[:, rows.to(DEV)].permute(1, 0, 2)) and equal(lobe_rgb, ref_rgb[:, rows.to(DEV)].permute(1, 0, 2))
    paired_b, _ = brdf_lobe(surf, rows, views, sun.expand(views.shape[0], 3))
    assert equal(paired_b, lobe_b)


def test_two_rank_relight_matches_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_relight_worker.py), each child under its own time limit and started
    once: the gathered surface and the relit image equal the single-rank result bitwise."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_relight_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=_free_port(), WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, worker], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=300)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append("TIMEOUT\n" + p.communicate()[0])
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert all("RESULT" in o and "ok" in o for o in outs), "\n".join(outs)
