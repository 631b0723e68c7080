"""Shared by tests/test_gpu_relight_shadows.py, tests/test_relight_shadows_cpu.py and tests/dist_relight_shadows_worker.py: the
--sun_v analystic model flags the shadowed-relighting tests cover (all rendered with apply_brdf=True, gsam_only=True, the only
form in which the reference runs that model), and the float64 statement of what bn_sun_shade_dirs computes,

    alpha_s = 1 - exp(-delta_s relu(sigma_s + noise_s noise_std)),  delta_{G-1} = 1e10,  T_s = prod_{j<s} (1 - alpha_j + 1e-10)
    per ray     rgb = clamp01(T_{G-1} BRDF(sun, view, composited sums))
    per sample  rgb = clamp01(sum_s w_s (c_s (1 + 2 pad) - pad) T_s),   c_s = albedo_s (Lambertian) | BRDF(row_s, sun, view)

built from oracle/brdf.py, oracle/render.py's composite and relight_cases.oracle_shade / channels.  Directions, seeds and
tolerances come from tests/relight_cases.py.

The inputs were fixed on the CPU before any GPU run: test_relight_shadows_cpu.py renders every case with the oracle, checks this
statement against the oracle's own rgb_coarse / sun_coarse, and asserts that its float32 evaluation stays within half of
ORACLE_TOL of its float64 evaluation for every (ray, direction).  The learned-normal heads are levelled
(relight_cases.level_normals) wherever the oracle is compared, for the reason given there.
"""
import torch

import relight_cases as RC
from oracle import brdf as OB
from oracle import render as ORD
from oracle.config import FieldConfig

_RPV = dict(funcM=1, funcF=1, funcH=1)
# name -> (FieldConfig flags, render flags, BRDF kind for the tolerance); sun_v="analystic" and apply_brdf=True everywhere
CASES = {
    "lambert": (dict(), dict(), "lambert"),
    "rpv111": (dict(normal="analystic", **_RPV), dict(), "rpv"),
    "hapke_bc": (dict(b=1, c=1, normal="learned"), dict(), "hapke"),
    "microfacet": (dict(roughness=True, normal="learned"), dict(), "microfacet"),
    "rpv111_multi": (dict(normal="learned", MultiBRDF=True, **_RPV), dict(), "rpv"),
    "rpv111_cos": (dict(normal="analystic", **_RPV), dict(cos_irra_on=True), "rpv"),       # the visibility is dropped
}


def config(name, **kw):
    base = dict(feat=64, n_samples=16, guided_samples=16, sun_v="analystic")
    base.update(CASES[name][0])
    base.update(kw)
    return FieldConfig(**base)


def cos_on(name):
    return bool(CASES[name][1].get("cos_irra_on", False))


def per_sample(name):
    """Shaded sample by sample: a Lambertian kind (no BRDF heads) or one BRDF per sample."""
    cfg = config(name)
    return bool(cfg.MultiBRDF) or not (cfg.roughness or cfg.RPV or cfg.b == 1 or cfg.shell_hapke > 0)


def tolerance(name):
    return RC.ORACLE_TOL[CASES[name][2]]


def transmittance(sigma_sun, z_sun, noise=None, noise_std=0.0, dtype=torch.float64):
    """T (K, R, G) of the sun pass from its densities and depths (K, R, G): oracle/render.py composite (cal_weight,
    models/spsbrdfnerf.py:50-69) per direction; noise (R, G) is shared by the directions."""
    sig, z = sigma_sun.to(dtype).cpu(), z_sun.to(dtype).cpu()
    K, R, G = sig.shape
    nz = None if noise is None else noise.to(dtype).cpu().unsqueeze(0).expand(K, R, G).reshape(K * R, G)
    _, T, _, _ = ORD.composite(z.reshape(K * R, G), sig.reshape(K * R, G), nz, noise_std)
    return T.reshape(K, R, G)


def sample_brdf(cfg, rows, rays_d, sun_k, dtype=torch.float64):
    """c_s (R, G, 3) of one direction: the row's albedo, or its BRDF (oracle/render.py:216-276, MultiBRDF)."""
    rows, rays_d = rows.to(dtype).cpu(), rays_d.to(dtype).cpu()
    R, G, C = rows.shape
    ch = RC.channels(cfg, True, False)
    assert ch["C"] == C, (ch, rows.shape)
    flat = rows.reshape(R * G, C)
    albedo = flat[:, :3]
    if not cfg.MultiBRDF:
        return albedo.reshape(R, G, 3)
    col = lambda name, n: flat[:, ch[name]:ch[name] + n] if name in ch else None
    l, v, normal = sun_k.to(dtype).cpu().expand(R * G, 3), (-rays_d).repeat_interleave(G, 0), col("normal", 3)
    if cfg.roughness:
        brdf = OB.microfacet(l, v, normal, albedo, col("roughness_from_xyz", 1), cfg.fresnel_f0)[1]
    elif cfg.RPV:
        rh = albedo if cfg.funcH == 2 else col("rhoc_from_xyz", 3)
        brdf = OB.rpv(l, v, normal, albedo, col("k_from_xyz", 3), col("theta_rpv_from_xyz", 3), rh)[0]
    else:
        brdf = OB.hapke(l, v, normal, albedo, col("b_from_xyz", 3), col("c_from_xyz", 3), None, cfg.hpk_scl, cfg.shell_hapke)[0]
    return brdf.reshape(R, G, 3)


def oracle_sun_shade(cfg, sigma_sun, z_sun, sun, rays_d, acc=None, wsum=None, rows=None, weights=None, noise=None, noise_std=0.0,
                     dtype=torch.float64):
    """rgb (K, R, 3) and vis (K, R) = T_{G-1} of the shadowed shading, from the sun pass's densities and depths (K, R, G) and
    either the composited sums (one BRDF per ray) or the rows (R, G, C) and weights (R, G)."""
    T = transmittance(sigma_sun, z_sun, noise, noise_std, dtype)
    vis = T[..., -1]
    sun = sun.to(dtype).cpu()
    if rows is None:
        _, brdf = RC.oracle_shade(cfg, acc, wsum, rays_d, sun, None, True, False, False, dtype)
        return (vis.unsqueeze(-1) * brdf).clamp(0.0, 1.0), vis
    pad, wx = cfg.rgb_padding, weights.to(dtype).cpu().unsqueeze(-1)
    rgb = []
    for k in range(sun.shape[0]):
        c = sample_brdf(cfg, rows, rays_d, sun[k], dtype)
        rgb.append((wx * (c * (1 + 2 * pad) - pad) * T[k].unsqueeze(-1)).sum(-2).clamp(0.0, 1.0))
    return torch.stack(rgb), vis


def oracle_rows(cfg, res):
    """The field-output rows (R, G, C) of an oracle render_rays result, put back together from its per-sample entries, and their
    weights (relight_sample_cases.oracle_rows, for models with or without a normal field)."""
    w = res["weights_coarse"].detach()
    ch = RC.channels(cfg, True, False)
    rows = torch.zeros(w.shape[0], w.shape[1], ch["C"], dtype=w.dtype)
    names = {"k_from_xyz": "rpv_k", "theta_rpv_from_xyz": "rpv_theta", "rhoc_from_xyz": "rpv_rhoc", "b_from_xyz": "hpk_b",
             "c_from_xyz": "hpk_c", "roughness_from_xyz": "roughness"}
    parts = [(0, "albedo"), (3, "sigmas")] + [(ch[n], key) for n, key in names.items() if n in ch]
    if "normal" in ch:
        parts.append((ch["normal"], "normal_lr" if cfg.normal in ("learned", "analystic_learned") else "normal_an"))
    for c0, key in parts:
        t = res[key + "_coarse"].detach().reshape(w.shape[0], w.shape[1], -1)
        rows[:, :, c0:c0 + t.shape[-1]] = t
    return rows, w


def oracle_render(name, rays, suns, seed, levelled=True, dtype=torch.float64):
    """The CPU oracle's own render_rays(gsam_only=True, apply_brdf=True) of `rays` with each sun written into rays[:, 8:11], after
    the same seed, and from it what the statement reads: per direction the sun pass's densities and depths, rebuilt with the
    oracle's own pieces from the pass-1 depth and the pass's logged uniforms (rendering.py:244-259).
    -> dict sigma_sun, z_sun (K, R, G), rows (R, G, C), weights (R, G), acc (R, C), wsum (R,), rays_d, rgb (K, R, 3), vis (K, R)."""
    from oracle.field import field_forward
    cfg = config(name)
    state = cfg.make_params(RC.MODEL_SEED)
    state = {k: torch.from_numpy(v) for k, v in state.items()}
    p = {k: v.to(dtype) for k, v in (RC.level_normals(state) if levelled else state).items()}
    G = cfg.guided_samples
    out = dict(sigma_sun=[], z_sun=[], rgb=[], vis=[])
    for k in range(suns.shape[0]):
        r = rays.to(dtype).clone()
        r[:, 8:11] = suns[k].to(dtype)
        rnd = ORD.Randoms(generator=torch.Generator().manual_seed(seed))
        res, _ = ORD.render_rays(p, cfg, r, rnd, mode="test", apply_brdf=True, cos_irra_on=cos_on(name), gsam_only=True)
        o, d, sun_d, d1 = r[:, 0:3], r[:, 3:6], r[:, 8:11], res["_pass1"]["depth"]
        far = d1.clone().unsqueeze(-1)
        if abs(float(sun_d[0, 2])) > 0.00001:
            far = torch.abs(d[0, 2] / sun_d[0, 2]) * far
        z_sun = ORD.get_z_vals(G, far * 0.01, far, rnd.log[2].to(dtype))
        xyz = (o + d * d1.unsqueeze(-1)).unsqueeze(1) + sun_d.unsqueeze(1) * z_sun.unsqueeze(2)
        with torch.no_grad():
            sig = field_forward(p, cfg, xyz.reshape(-1, 3), sigma_only=True, apply_brdf=False, apply_theta=False, nr_an_on=False,
                                nr_lr_on=False).view(-1, G)
        out["sigma_sun"].append(sig)
        out["z_sun"].append(z_sun)
        out["rgb"].append(res["rgb_coarse"].detach())
        out["vis"].append(res["sun_coarse"][:, -1, 0].detach())
        if k == 0:                          # the geometry does not depend on the sun
            rows, w = oracle_rows(cfg, res)
            out.update(rows=rows, weights=w, acc=(w.unsqueeze(-1) * rows).sum(1), wsum=w.sum(-1), rays_d=r[:, 3:6])
    return {k: (torch.stack(v) if isinstance(v, list) else v) for k, v in out.items()}
