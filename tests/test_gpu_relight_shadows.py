"""GPU tests of relighting with cast shadows (brdf_nerf_amd/shadows.py, bn_sun_ray_table / bn_sun_shade_dirs): a --sun_v analystic
view under K sun directions from ONE geometry pass.  Run on the MI355X box with `pytest -m gpu`.  Cases and the float64
statement: tests/relight_shadow_cases.py (checked on the CPU by tests/test_relight_shadows_cpu.py)."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from conftest import assert_close
import relight_cases as RC
import relight_shadow_cases as HC
from test_gpu_parity import DEV, _free_port, make_args

pytestmark = pytest.mark.gpu
R_TEST, CHUNK = 300, 100        # three chunks; R no multiple of the kernel's 64-ray block

bits = lambda t: t.contiguous().view(torch.int32)               # bitwise, NaN payloads included
equal = lambda a, b: a.shape == b.shape and torch.equal(bits(a), bits(b))


def build(name, dtype="fp32", level=False, R=R_TEST, **cfg_kw):
    """Model and rays of a case, built as tests/test_gpu_relight.py builds its own."""
    from brdf_nerf_amd import load_model
    from brdf_nerf_amd.raytable import synthetic_table
    cfg = HC.config(name, **cfg_kw)
    args = make_args(cfg, dtype)
    assert args.sun_v == "analystic"
    model = load_model(args)
    sd = {k: torch.from_numpy(v) for k, v in cfg.make_params(RC.MODEL_SEED).items()}
    model.load_state_dict(RC.level_normals(sd) if level else sd)
    rays = synthetic_table(R, device=DEV, seed=RC.RAYS_SEED).data["rays"].clone()
    return cfg, args, {"coarse": model.to(DEV)}, rays


def render_per_sun(models, args, rays, sun, seed, chunk, cosi):
    """render_rays(gsam_only=True) with `sun` written into the rays, over the chunks of one render_image call, after the seed."""
    from brdf_nerf_amd import render_rays
    r = rays.clone()
    r[:, 8:11] = sun
    torch.manual_seed(seed)
    keys = ("rgb_coarse", "depth_coarse", "sun_coarse")
    parts = {k: [] for k in keys}
    with torch.no_grad():
        for i in range(0, r.shape[0], chunk):
            want, _ = render_rays(models, args, r[i:i + chunk], None, mode="test", apply_brdf=True, cos_irra_on=cosi, gsam_only=True)
            for k in keys:
                parts[k].append(want[k])
    return tuple(torch.cat(parts[k]) for k in keys)


@pytest.mark.parametrize("name,dtype", [(n, "fp32") for n in HC.CASES] + [("rpv111", "bf16")])
def test_matches_render_rays_per_direction(name, dtype):
    """Against the product path: per sun reseed, write it into rays[:, 8:11] and call render_rays(gsam_only=True); reseed and call
    relight_image_shadowed once.  rgb[k] and visibility[k] (against sun_coarse[:, -1, 0]) match to assert_close's defaults - the
    compositing kernel multiplies in wave-scan order, this one serially: not bitwise; depth is the same computation on the same
    draws: equal bit for bit.  Once in one call and once over three chunks (against render_image(gsam_only=True, chunk=100), whose
    row-0 quirk is per chunk).  rpv111_cos: the cosine branch drops the visibility upstream, so the sun pass only runs because the
    map is asked for (want_visibility=True); without that it is None."""
    from brdf_nerf_amd import relight_image_shadowed
    from brdf_nerf_amd.evaluate import render_image
    cfg, args, models, rays = build(name, dtype)
    cosi = HC.cos_on(name)
    suns = RC.sun_directions().to(DEV)
    K = suns.shape[0]
    for chunk in (R_TEST, CHUNK):
        torch.manual_seed(17)
        got = relight_image_shadowed(models, args, rays, suns, chunk=chunk, cos_irra_on=cosi, want_visibility=True)
        assert tuple(got["rgb"].shape) == (K, R_TEST, 3) and tuple(got["visibility"].shape) == (K, R_TEST)
        for k in range(K):
            want_rgb, want_depth, want_sun = render_per_sun(models, args, rays, suns[k], 17, chunk, cosi)
            err = float((got["rgb"][k] - want_rgb).abs().max())
            verr = float((got["visibility"][k] - want_sun[:, -1, 0]).abs().max())
            print(f"{name} {dtype} chunk {chunk} sun {k}: max |rgb - rgb_coarse| = {err:.3e}, max |vis - sun_coarse| = {verr:.3e}, "
                  f"visibility in [{float(want_sun[:, -1, 0].min()):.3f}, {float(want_sun[:, -1, 0].max()):.3f}]")
            assert_close(got["rgb"][k], want_rgb, msg=f"{name} rgb[{k}]")
            assert torch.equal(got["depth"], want_depth), f"{name} depth, sun {k}"
            assert_close(got["visibility"][k], want_sun[:, -1, 0], msg=f"{name} visibility[{k}]")
    # the chunked view once more against evaluate.render_image itself
    r = rays.clone()
    r[:, 8:11] = suns[2]
    torch.manual_seed(17)
    img = render_image(models, args, r, chunk=CHUNK, apply_brdf=True, cos_irra_on=cosi, gsam_only=True)
    assert_close(got["rgb"][2], img["rgb"], msg=f"{name} render_image rgb")
    assert torch.equal(got["depth"], img["depth"])
    if cosi:
        torch.manual_seed(17)
        plain = relight_image_shadowed(models, args, rays, suns, chunk=CHUNK, cos_irra_on=True)
        assert plain["visibility"] is None and equal(plain["rgb"], got["rgb"])


def _torch_table(rays, d1, sun_k, u):
    """The sun pass's rays and depths for ONE direction as rendering._sample_passes forms them."""
    from brdf_nerf_amd import functions as Fn
    from brdf_nerf_amd.rendering import sun_far
    R = rays.shape[0]
    rays_d, sun_d = rays[:, 3:6], sun_k.expand(R, 3)
    far = sun_far(d1, rays_d, sun_d)
    near = far * 0.01
    z = Fn.stratified_z(near, far, u)
    sun_rays = torch.cat([rays[:, 0:3] + rays_d * d1.unsqueeze(-1), sun_d], -1).contiguous()
    return torch.cat([sun_rays, near, far], -1), z


@pytest.mark.parametrize("R", [300, 1])
def test_ray_table_is_bitwise_the_torch_statement(R):
    """bn_sun_ray_table for 33 directions - the six suns, (1, 0, 0) (the |sun_z| <= 1e-5 branch), one below the horizon
    (sun_z < 0), padded with turned copies - against rendering.sun_far + Fn.stratified_z + the torch.cat of _sample_passes per
    direction: table and z_sun torch.equal."""
    from brdf_nerf_amd import directions, functions as Fn
    from brdf_nerf_amd.raytable import synthetic_table
    G = 16
    rays = synthetic_table(300, device=DEV, seed=RC.RAYS_SEED).data["rays"][:R].contiguous()
    g = torch.Generator().manual_seed(8)
    d1 = (0.5 + torch.rand(R, generator=g)).to(DEV)
    u = torch.rand(R, G, generator=g).to(DEV)
    suns = torch.cat([RC.sun_directions(), torch.tensor([[1.0, 0.0, 0.0], RC.unit(-30, 75)]),
                      directions(torch.linspace(20, 85, 25), torch.linspace(0, 340, 25))]).to(DEV)
    K = suns.shape[0]
    assert K == 33 and float(suns[7, 2]) < 0
    table, z_sun = Fn.sun_ray_table(rays, d1, suns, u)
    assert tuple(table.shape) == (K * R, 8) and tuple(z_sun.shape) == (K * R, G)
    for k in range(K):
        want_t, want_z = _torch_table(rays, d1, suns[k], u)
        assert equal(table[k * R:(k + 1) * R], want_t), k
        assert equal(z_sun[k * R:(k + 1) * R], want_z), k
    assert equal(table[6 * R:7 * R, 7], d1)                      # ratio 1 where the sun lies in the horizon


def _sun_pass_inputs(surf, suns):
    """sigma_sun, z_sun (K, R, G) of a one-chunk surface, as relight_shadowed forms them."""
    from brdf_nerf_amd import functions as Fn
    K, (R, G) = suns.shape[0], surf.u_sun.shape
    table, z_sun = Fn.sun_ray_table(surf.rays, surf.d1, suns, surf.u_sun)
    sigma = Fn.field_sigma(surf.model.spec(False, False, False, False), surf.model.named(), surf.packed, rays=table, z=z_sun)
    return sigma.view(K, R, G), z_sun.view(K, R, G)


@pytest.mark.parametrize("name,noise_std", [(n, 0.0) for n in HC.CASES if not HC.cos_on(n)] + [("rpv111", 0.5), ("lambert", 0.5)])
def test_shade_kernel_matches_float64_oracle(name, noise_std):
    """Against the float64 statement, independent of the product's shading code: levelled normals; the kernel's own sigma_sun,
    z_sun and acc / rows copied to the CPU; rgb and vis over every entry at ORACLE_TOL of the kind; the oracle's values finite.
    noise_std = 0.5: with the pass's noise array."""
    from brdf_nerf_amd import functions as Fn, render_shadow_surface
    cfg, args, models, rays = build(name, level=True, noise_std=noise_std)
    rtol, atol = HC.tolerance(name)
    suns = RC.sun_directions().to(DEV)
    torch.manual_seed(3)
    surf = render_shadow_surface(models, args, rays)
    assert surf.per_sample == HC.per_sample(name) and (surf.noise_sun is not None) == (noise_std != 0)
    sigma, z_sun = _sun_pass_inputs(surf, suns)
    src = dict(X=surf.rows, w=surf.weights) if surf.per_sample else dict(acc=surf.acc, wsum=surf.wsum)
    rgb, vis = Fn.sun_shade_dirs(surf.desc(), sigma, z_sun, surf.rays_d, suns, noise=surf.noise_sun, noise_std=noise_std, want_vis=True, **src)
    osrc = dict(rows=surf.rows, weights=surf.weights) if surf.per_sample else dict(acc=surf.acc, wsum=surf.wsum)
    want_rgb, want_vis = HC.oracle_sun_shade(cfg, sigma, z_sun, suns, surf.rays_d, noise=surf.noise_sun, noise_std=noise_std, **osrc)
    assert bool(torch.isfinite(want_rgb).all()) and bool(torch.isfinite(want_vis).all()), f"{name}: oracle not finite"
    for what, got, want in (("rgb", rgb, want_rgb), ("vis", vis, want_vis)):
        e = (got.cpu().double() - want).abs()
        print(f"{name} noise {noise_std} {what}: max abs err {float(e.max()):.3e}, max err/tol {float((e / (atol + rtol * want.abs())).max()):.3f}, "
              f"values in [{float(want.min()):.3f}, {float(want.max()):.3f}]")
    assert_close(rgb, want_rgb, rtol, atol, f"{name} rgb")
    assert_close(vis, want_vis, rtol, atol, f"{name} vis")


def _synthetic_inputs(name, R, G, K, seed):
    """Made-up inputs of bn_sun_shade_dirs, the way test_gpu_relight._synthetic_surface makes up sums: level ground with tilted
    normals, parameters inside their heads' ranges; random densities >= 0 (half of them zero) and sorted depths."""
    cfg, args, models, _ = build(name)
    model = models["coarse"]
    spec = model.spec(True, False, model.normal in ("analystic_learned", "learned"), model.normal in ("analystic_learned", "analystic"))
    from brdf_nerf_amd.rendering import shade_desc
    desc = shade_desc(model, args, spec, True, False)
    Cc = spec.out_channels
    ch = RC.channels(cfg, True, False)
    g = torch.Generator().manual_seed(seed)
    per_sample = HC.per_sample(name)
    shape = (R, G, Cc) if per_sample else (R, Cc)
    x = 0.1 + 0.8 * torch.rand(*shape, generator=g)
    if "normal" in ch:
        n = torch.cat([0.3 * torch.randn(*shape[:-1], 2, generator=g), torch.ones(*shape[:-1], 1)], -1)
        x[..., ch["normal"]:ch["normal"] + 3] = n / n.norm(dim=-1, keepdim=True) if per_sample else n
    d = torch.cat([0.2 * torch.randn(R, 2, generator=g), -torch.ones(R, 1)], -1)
    d = (d / d.norm(dim=-1, keepdim=True)).to(DEV).contiguous()
    if per_sample:
        w = torch.softmax(2.0 * torch.randn(R, G, generator=g), -1)
        src = dict(X=x.to(DEV), w=w.to(DEV))
    else:
        src = dict(acc=x.to(DEV), wsum=(0.9 + 0.1 * torch.rand(R, generator=g)).to(DEV))
    s = torch.rand(K, R, G, generator=g)
    sigma = torch.where(s < 0.5, torch.zeros(()), 8.0 * (s - 0.5)).to(DEV)
    z = torch.sort(0.01 + torch.rand(K, R, G, generator=g), -1)[0].to(DEV).contiguous()
    return desc, sigma, z, d, src


@pytest.mark.parametrize("name", ["rpv111", "lambert", "rpv111_multi"])
@pytest.mark.parametrize("G", [3, 16, 64])
def test_tiling_is_invisible(name, G):
    """Every (direction, ray) is computed on its own: K = 1, a split of the 33 directions, a ray subset, `out=` as a [:, i:j]
    slice of a larger buffer and `out=` on the host all give bitwise the rows of ONE K = 33 call - R = 300 is no multiple of the
    64-ray block, G = 3 is the smallest, 16 one piece of the LDS staging, 64 several."""
    from brdf_nerf_amd import directions, functions as Fn
    R, K = 300, 33
    desc, sigma, z, d, src = _synthetic_inputs(name, R, G, K, 5)
    suns = directions(torch.linspace(25, 80, K), torch.linspace(0, 330, K)).to(DEV)
    whole, whole_v = Fn.sun_shade_dirs(desc, sigma, z, d, suns, want_vis=True, **src)
    assert float(whole_v.max()) > float(whole_v.min()) >= 0.0 and float(whole.max()) > 0.0
    again, again_v = Fn.sun_shade_dirs(desc, sigma, z, d, suns, want_vis=True, **src)
    assert equal(again, whole) and equal(again_v, whole_v)
    for k in (0, 16, 32):
        one, one_v = Fn.sun_shade_dirs(desc, sigma[k:k + 1].contiguous(), z[k:k + 1].contiguous(), d, suns[k:k + 1], want_vis=True, **src)
        assert equal(one[0], whole[k]) and equal(one_v[0], whole_v[k]), k
    for tile in (2, 7):
        for k0 in range(0, K, tile):
            t, tv = Fn.sun_shade_dirs(desc, sigma[k0:k0 + tile].contiguous(), z[k0:k0 + tile].contiguous(), d, suns[k0:k0 + tile], want_vis=True, **src)
            assert equal(t, whole[k0:k0 + tile]) and equal(tv, whole_v[k0:k0 + tile]), (tile, k0)
    i, j = 37, 170                                            # a ray subset that starts inside a block
    sub_src = {k: v[i:j].contiguous() for k, v in src.items()}
    sub, sub_v = Fn.sun_shade_dirs(desc, sigma[:, i:j].contiguous(), z[:, i:j].contiguous(), d[i:j], suns, want_vis=True, **sub_src)
    assert equal(sub, whole[:, i:j]) and equal(sub_v, whole_v[:, i:j])
    big, big_v = torch.full((K, 2 * R, 3), -1.0, device=DEV), torch.full((K, 2 * R), -1.0, device=DEV)
    Fn.sun_shade_dirs(desc, sigma[:, i:j].contiguous(), z[:, i:j].contiguous(), d[i:j], suns, rgb=big[:, 100 + i:100 + j], vis=big_v[:, 100 + i:100 + j],
                      **sub_src)
    assert equal(big[:, 100 + i:100 + j], whole[:, i:j]) and equal(big_v[:, 100 + i:100 + j], whole_v[:, i:j])
    assert bool((big[:, :100 + i] == -1).all()) and bool((big[:, 100 + j:] == -1).all()) and bool((big_v[:, 100 + j:] == -1).all())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_direction_tiles_are_invisible_end_to_end(dtype):
    """relight_shadowed with dir_tile=1 (one field pass per direction) equals dir_tile=None (one over all) bitwise - the field's
    sigma-only pass is batch invariant (P1 of tests/test_gpu_half_invariants.py) - and so do dir_tile=4, `out=` on the host and
    sun_visibility."""
    from brdf_nerf_amd import relight_shadowed, render_shadow_surface, sun_visibility
    cfg, args, models, rays = build("rpv111", dtype)
    suns = RC.sun_directions().to(DEV)
    torch.manual_seed(5)
    surf = render_shadow_surface(models, args, rays, chunk=CHUNK)
    assert surf.bounds == [(0, 100), (100, 200), (200, 300)]
    whole, whole_v = relight_shadowed(surf, suns, want_visibility=True)
    for tile in (1, 4):
        rgb, vis = relight_shadowed(surf, suns, dir_tile=tile, want_visibility=True)
        assert equal(rgb, whole) and equal(vis, whole_v), tile
    host = torch.full((suns.shape[0], R_TEST, 3), -1.0)
    assert relight_shadowed(surf, suns, out=host, dir_tile=5) is host and equal(host, whole.cpu())
    assert equal(sun_visibility(surf, suns, dir_tile=1), whole_v)


@pytest.mark.parametrize("name", ["rpv111", "rpv111_cos"])
def test_field_points_are_counted(name, monkeypatch):
    """K = 8, chunk = 100: relight_image_shadowed evaluates exactly R S + K R G sigma-only points and R G full points - one
    geometry pass plus the sun points; with the cosine branch (rpv111_cos) no sun point at all."""
    from brdf_nerf_amd import functions as Fn, relight_image_shadowed
    cfg, args, models, rays = build(name)
    model = models["coarse"]
    S, G, K = cfg.n_samples, cfg.guided_samples, 8
    count = {"sigma": 0, "full": 0}
    sigma0, eval0 = Fn.field_sigma, model.evaluate

    def sigma(spec, named, packed, xyz=None, rays=None, z=None, out=None):
        count["sigma"] += xyz.shape[0] if xyz is not None else z.numel()
        return sigma0(spec, named, packed, xyz=xyz, rays=rays, z=z, out=out)

    def evaluate(spec, packed, xyz=None, rays=None, z=None, **kw):
        count["full"] += xyz.shape[0] if xyz is not None else z.numel()
        return eval0(spec, packed, xyz=xyz, rays=rays, z=z, **kw)
    monkeypatch.setattr(Fn, "field_sigma", sigma)
    model.evaluate = evaluate
    suns = torch.cat([RC.sun_directions(), RC.sun_directions()[:2]]).to(DEV)
    assert suns.shape[0] == K
    relight_image_shadowed(models, args, rays, suns, chunk=CHUNK, cos_irra_on=HC.cos_on(name))
    want_sigma = R_TEST * S + (0 if HC.cos_on(name) else K * R_TEST * G)
    assert count == {"sigma": want_sigma, "full": R_TEST * G}, (count, want_sigma, R_TEST * G)


def test_abi_rejects_bad_arguments():
    """bn_sun_shade_dirs through ctypes: non-zero with bn_last_error set for a NULL input, a descriptor with irr set, cos_irradiance
    with a normal channel, both and neither of acc / X, per-ray mode with kind LAMBERT, G < 3 and G > BN_MAX_G - argument checks,
    nothing is launched; the same calls with good arguments return 0."""
    from brdf_nerf_amd import _lib as L
    R, G, K, Cc = 2, 4, 1, 13
    f = lambda *shape: torch.full(shape, 0.5, device=DEV)
    sg, z, acc, ws, X, w, rd, sun, rgb, irr = f(K, R, G), f(K, R, G), f(R, Cc), f(R), f(R, G, Cc), f(R, G), f(R, 3), f(K, 3), f(K, R, 3), f(R)
    z[:] = torch.linspace(0.1, 0.4, G, device=DEV)
    acc[:, 4:7] = X[..., 4:7] = torch.tensor([0.0, 0.0, 1.0], device=DEV)
    rd[:] = torch.tensor([0.0, 0.0, -1.0], device=DEV)
    sun[:] = torch.tensor(RC.unit(50, 190), device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def desc(kind=L.BN_SHADE_RPV, irr_t=None, cos=0):
        d = L.ShadeDesc()
        d.kind, d.C, d.ch_normal, d.ch_p0, d.ch_p1, d.ch_p2 = kind, Cc, 4, 7, 10, -1
        d.rhoc_is_albedo = d.shell = d.usealldepth = 0
        d.cos_irradiance = cos
        d.hpk_scl, d.f0, d.rgb_padding, d.lambda_rgb, d.lambda_ds, d.lambda_hs = 4.0, 0.04, 0.001, 1.0, 0.0, 0.0
        if irr_t is not None:
            d.irr, d.irr_stride = irr_t.data_ptr(), 1
        return d

    def call(d, sigma=sg, a=acc, x=None, g=G):
        return L.lib().bn_sun_shade_dirs(C.byref(d), p(sigma), p(z), None, 0.0, p(a), p(ws), p(x), p(w), p(rd), 3, p(sun), R, g, K, p(rgb),
                                         3 * R, None, 0, None)

    def refused(status, word):
        msg = L.lib().bn_last_error().decode()
        assert status != 0 and "sun_shade_dirs" in msg and word in msg, (status, msg, word)
    assert call(desc()) == 0 and call(desc(), a=None, x=X) == 0 and call(desc(kind=L.BN_SHADE_LAMBERT), a=None, x=X) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rgb).all())
    refused(call(desc(), sigma=None), "null")
    refused(call(desc(irr_t=irr)), "irradiance")
    refused(call(desc(cos=1)), "cos_irradiance")
    refused(call(desc(), x=X), "both")
    refused(call(desc(), a=None), "neither")
    refused(call(desc(kind=L.BN_SHADE_LAMBERT)), "Lambertian")
    refused(call(desc(), g=2), "G=2")
    refused(call(desc(), g=L.BN_MAX_G + 1), f"G={L.BN_MAX_G + 1}")


def test_two_ranks_reproduce_their_shards():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_relight_shadows_worker.py), each child under its own time limit and
    started once: the gathered rgb / depth / visibility equal bitwise what single-process calls on rays[lo:hi] give after the
    same per-rank seed."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_relight_shadows_worker.py")
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
