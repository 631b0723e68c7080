"""Shared by tests/test_gpu_relight_samples.py, tests/test_relight_samples_cpu.py and tests/dist_relight_samples_worker.py:
the --MultiBRDF 1 model flags the per-sample relighting tests cover, their fixed inputs, and the per-sample shading

    rgb[c] = clamp01( sum_s w_s (brdf_c(row_s, sun, view) (1 + 2 pad) - pad) irr )

stated with oracle/brdf.py alone (float64).  Directions, channel layout and tolerances come from tests/relight_cases.py.

The synthetic rows and the direction lists were fixed on the CPU before any GPU run: test_relight_samples_cpu.py asserts that the
oracle is finite on them at every entry and that its float32 evaluation agrees with its float64 one within half the tolerance of
the GPU comparison.
"""
import math

import torch

import relight_cases as RC
from oracle import brdf as OB
from oracle.config import FieldConfig

# name -> (FieldConfig flags, render flags, BRDF kind for the tolerance); every model has one BRDF per sample
CASES = {
    "rpv111_nlr": (dict(funcM=1, funcF=1, funcH=1, normal="learned"), dict(apply_brdf=True, cos_irra_on=True), "rpv"),
    "rpv_m1f1h2": (dict(funcM=1, funcF=1, funcH=2, normal="learned"), dict(apply_brdf=True), "rpv"),        # rhoc is the albedo
    "hapke_bct": (dict(b=1, c=1, theta=1, normal="learned"), dict(apply_brdf=True, apply_theta=True, cos_irra_on=True), "hapke"),
    "microfacet": (dict(roughness=True, normal="learned"), dict(apply_brdf=True), "microfacet"),
}
N_SUN = 70              # more than one 64-wide anything, and no multiple of the kernel's direction tile


def config(name, **kw):
    base = dict(feat=64, n_samples=16, guided_samples=16, MultiBRDF=True)
    base.update(CASES[name][0])
    base.update(kw)
    return FieldConfig(**base)


def flags(name):
    fl = CASES[name][1]
    return dict(apply_brdf=fl.get("apply_brdf", False), apply_theta=fl.get("apply_theta", False), cos_irra_on=fl.get("cos_irra_on", False))


def sun_directions_many():
    """N_SUN suns: the six of relight_cases.sun_directions(), repeated with small fixed rotations (group g = i // 6 is turned by
    g degrees in azimuth and raised by 0.4 g degrees: elevations stay within 25 - 84.4 degrees, azimuths within 12 degrees of
    the six; see synthetic_rows for why they stay in six narrow bands)."""
    base = [(25, 10), (35, 100), (50, 190), (62, 250), (71, 320), (80, 45)]
    d = [RC.unit(base[i % 6][0] + 0.4 * (i // 6), base[i % 6][1] + 1.0 * (i // 6)) for i in range(N_SUN)]
    return torch.tensor(d, dtype=torch.float32)


def lobe_pairs():
    """(sun, view) of lobe mode: the 32 view directions of relight_cases.lobe_directions() around its one fixed sun."""
    view = RC.lobe_directions()
    return torch.tensor([RC.unit(*RC.LOBE_SUN)], dtype=torch.float32).expand(view.shape[0], 3).contiguous(), view


def oracle_sample_shade(cfg, rows, weights, rays_d, sun, view=None, flags=None, dtype=torch.float64):
    """rgb, brdf (K, R, 3) of the per-sample shading (oracle/render.py:216-276, MultiBRDF, no sun pass) from the depth-sorted
    field-output rows (R, S, C) and their weights (R, S), with oracle/brdf.py alone.  view (K, 3): replaces -rays_d.  brdf is
    sum_s w_s brdf_s, before padding, irradiance and clamp.  flags: apply_brdf / apply_theta / cos_irra_on."""
    fl = dict(apply_brdf=False, apply_theta=False, cos_irra_on=False)
    fl.update(flags or {})
    ab, at = fl["apply_brdf"], fl["apply_theta"]
    rows, weights, rays_d, sun = rows.to(dtype).cpu(), weights.to(dtype).cpu(), rays_d.to(dtype).cpu(), sun.to(dtype).cpu()
    ch = RC.channels(cfg, ab, at)
    R, S, C = rows.shape
    assert ch["C"] == C and "normal" in ch, (ch, rows.shape)
    pad = cfg.rgb_padding
    flat = rows.reshape(R * S, C)
    col = lambda name, n: flat[:, ch[name]:ch[name] + n] if name in ch else None
    normal, albedo = col("normal", 3), flat[:, :3]
    wx = weights.unsqueeze(-1)
    rep = lambda t: t.repeat_interleave(S, 0)
    rgbs, brdfs = [], []
    for k in range(sun.shape[0]):
        l = sun[k].expand(R * S, 3)
        v = rep(-rays_d) if view is None else view[k].to(dtype).cpu().expand(R * S, 3)
        if cfg.roughness and ab:
            brdf = OB.microfacet(l, v, normal, albedo, col("roughness_from_xyz", 1), cfg.fresnel_f0)[1]
        elif cfg.RPV and ab:
            rh = albedo if cfg.funcH == 2 else col("rhoc_from_xyz", 3)
            brdf = OB.rpv(l, v, normal, albedo, col("k_from_xyz", 3), col("theta_rpv_from_xyz", 3), rh)[0]
        elif (ab and cfg.b == 1) or cfg.shell_hapke > 0:
            th = col("theta_from_xyz", 1)
            brdf = OB.hapke(l, v, normal, albedo, col("b_from_xyz", 3) if ab else None, col("c_from_xyz", 3) if ab else None,
                            None if th is None else th.reshape(-1), cfg.hpk_scl, cfg.shell_hapke)[0]
        else:
            raise ValueError("a model without a BRDF is shaded per ray (relight_cases.oracle_shade)")
        brdf = brdf.reshape(R, S, 3)
        irr = sun[k, 2].abs() if fl["cos_irra_on"] else 1.0
        rgbs.append((wx * (brdf * (1 + 2 * pad) - pad) * irr).sum(-2).clamp(0.0, 1.0))
        brdfs.append((wx * brdf).sum(-2))
    return torch.stack(rgbs), torch.stack(brdfs)


def oracle_rows(cfg, res, apply_brdf, apply_theta):
    """The field-output rows (R, S + G, C) of an oracle render_rays result, put back together from its per-sample entries."""
    w = res["weights_coarse"].detach()
    ch = RC.channels(cfg, apply_brdf, apply_theta)
    rows = torch.zeros(w.shape[0], w.shape[1], ch["C"], dtype=w.dtype)
    put = lambda c0, t: rows.__setitem__((slice(None), slice(None), slice(c0, c0 + t.shape[-1])), t.detach().reshape(w.shape[0], w.shape[1], -1))
    put(0, res["albedo_coarse"])
    put(3, res["sigmas_coarse"])
    put(ch["normal"], res["normal_lr_coarse"] if cfg.normal in ("learned", "analystic_learned") else res["normal_an_coarse"])
    names = {"k_from_xyz": "rpv_k", "theta_rpv_from_xyz": "rpv_theta", "rhoc_from_xyz": "rpv_rhoc", "b_from_xyz": "hpk_b",
             "c_from_xyz": "hpk_c", "theta_from_xyz": "hpk_theta", "roughness_from_xyz": "roughness"}
    for name, key in names.items():
        if name in ch:
            put(ch[name], res[key + "_coarse"])
    return rows, w


def synthetic_rows(name, R, S, seed):
    """Made-up rows of a case, the way test_gpu_relight._synthetic_surface makes up sums: level ground with tilted up-facing unit
    normals, albedo and parameters inside their heads' ranges.  The weights are a random softmax-like profile per ray, scaled to a
    sum of 0.9 - 1, with a quarter of the samples set to exactly zero.
    Three choices keep oracle/brdf.py itself well conditioned in float32 on EVERY (ray, sample, direction) - found on the CPU
    (test_relight_samples_cpu.py), where the first attempt (normals tilted by 0.3 randn, nadir rays, roughness from 0.1) missed:
    - Hapke's shadowing term jumps between 0 and inf where the relative azimuth of view and sun about the normal rounds to pi
      (relight_cases.lobe_directions).  A near-nadir view under a tilted normal has an arbitrary azimuth, and over R S K
      evaluations some land there.  So the rays look 25 - 35 degrees off nadir from azimuth 325 - 335 degrees, at least 34 degrees
      from the anti-solar azimuth of every sun of sun_directions_many(), and the normals tilt by at most 0.05 per component
      (4 degrees), which turns those azimuths by less than that margin (a sun 6 degrees off the zenith by up to 55 of its 94).
    - cos(incidence) stays off its 1e-5 clamp (relight_cases.level_normals): the same small tilt.
    - The microfacet distribution's denominator (n.h)^2 (a^4 - 1) + 1 cancels to ~a^4 at the specular peak, a = roughness: from
      roughness 0.4 up float32 keeps 4 digits there, at 0.1 it cannot.
    -> rows (R, S, C), weights (R, S), rays_d (R, 3), float32 on the CPU."""
    cfg = config(name)
    fl = flags(name)
    ch = RC.channels(cfg, fl["apply_brdf"], fl["apply_theta"])
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, generator=g)
    rows = u(0.1, 0.9, R, S, ch["C"])
    if "roughness_from_xyz" in ch:
        rows[..., ch["roughness_from_xyz"]] = u(0.4, 0.9, R, S)
    n = torch.cat([u(-0.05, 0.05, R, S, 2), torch.ones(R, S, 1)], -1)
    rows[..., ch["normal"]:ch["normal"] + 3] = n / n.norm(dim=-1, keepdim=True)
    w = torch.softmax(2.0 * torch.randn(R, S, generator=g), -1) * u(0.9, 1.0, R, 1)
    w = torch.where(torch.rand(R, S, generator=g) < 0.25, torch.zeros(()), w)
    assert bool((w == 0).any()) and float(w.sum(-1).max()) <= 1.0
    el, az = torch.deg2rad(u(55.0, 65.0, R)), torch.deg2rad(u(325.0, 335.0, R))       # where the camera is, seen from the ground
    view = torch.stack([torch.sin(az) * torch.cos(el), torch.cos(az) * torch.cos(el), torch.sin(el)], -1)
    return rows.contiguous(), w.contiguous(), (-view).contiguous()


def tolerance(name):
    """(rtol, atol) of the case's BRDF kind: relight_cases.ORACLE_TOL, the per-point parity tolerances.  The sum over a ray's
    samples has non-negative weights with sum_s w_s <= 1, so a bound that holds per term holds for the sum."""
    return RC.ORACLE_TOL[CASES[name][2]]


assert math.isclose(float(sun_directions_many()[0].norm()), 1.0, abs_tol=1e-6)
