"""Shared by tests/test_gpu_relight.py, tests/test_relight_cpu.py and tests/dist_relight_worker.py: the model flags the relighting
tests cover, their directions, and the ray-level shading stated with oracle/brdf.py alone (float64) from composited sums.

The directions were fixed on the CPU before any GPU run: for the models and rays of the tests, oracle/brdf.py evaluated in
float64 is finite for every (ray, direction) (test_relight_cpu.py asserts it for the oracle's own surface of each case).
"""
import math

import torch

from oracle import brdf as OB
from oracle.config import FieldConfig

# name -> (FieldConfig flags, render flags, BRDF kind for the tolerance)
CASES = {
    "lambert": (dict(), dict(), "lambert"),
    "lambert_normals_cos": (dict(normal="learned"), dict(cos_irra_on=True), "lambert"),
    "rpv111": (dict(funcM=1, funcF=1, funcH=1, normal="analystic"), dict(apply_brdf=True, cos_irra_on=True), "rpv"),
    "hapke_bc": (dict(b=1, c=1, normal="learned"), dict(apply_brdf=True), "hapke"),
    "hapke_bct": (dict(b=1, c=1, theta=1, normal="learned"), dict(apply_brdf=True, apply_theta=True, cos_irra_on=True), "hapke"),
    "hapke_shell3": (dict(shell_hapke=3, normal="learned"), dict(), "hapke"),
    "microfacet": (dict(roughness=True, normal="learned"), dict(apply_brdf=True), "microfacet"),
}
# (rtol, atol) of the per-point BRDF parity tests of the same kind (tests/test_gpu_parity.py test_brdf_*_golden);
# Lambertian: conftest.assert_close's defaults
ORACLE_TOL = {"lambert": (1e-4, 1e-6), "rpv": (1e-4, 1e-6), "hapke": (2e-4, 2e-6), "microfacet": (1e-4, 1e-6)}
MODEL_SEED = 11
RAYS_SEED = 4


def config(name, **kw):
    base = dict(feat=64, n_samples=16, guided_samples=16)
    base.update(CASES[name][0])
    base.update(kw)
    return FieldConfig(**base)


def unit(el_deg, az_deg):
    """The reference's angle convention, written out here on its own (eval.py:300-314): (sin az cos el, cos az cos el, sin el)."""
    el, az = math.radians(el_deg), math.radians(az_deg)
    return [math.sin(az) * math.cos(el), math.cos(az) * math.cos(el), math.sin(el)]


def sun_directions():
    """Six suns, elevation 25-80 degrees, spread in azimuth."""
    return torch.tensor([unit(25, 10), unit(35, 100), unit(50, 190), unit(62, 250), unit(71, 320), unit(80, 45)], dtype=torch.float32)


LOBE_SUN = (50.0, 190.0)


def lobe_directions():
    """View grid of a lobe around the fixed sun LOBE_SUN: elevation 25-70 degrees x 8 azimuths at +-30, 75, 120, 150 degrees from
    the sun's.  The principal plane (relative azimuth 0 / 180) and the zenith are left out on purpose: Hapke's shadowing term
    exp(-2 tan((phi + 1e-5) / 2)) (oracle/brdf.py _f) jumps between 0 and inf at phi = pi, where float64 and float32 land on
    different sides - the formula, not an implementation, is singular there (seen on the CPU: the oracle in float32 against itself
    in float64 differs by the whole value)."""
    d = [unit(el, LOBE_SUN[1] + s * a) for el in (25, 40, 55, 70) for a in (30, 75, 120, 150) for s in (1, -1)]
    return torch.tensor(d, dtype=torch.float32)


def level_normals(state):
    """Give the learned-normal head of a state dict (make_params) the bias of level ground: composited normals point up, as they
    do in a trained model of a near-nadir scene.  A freshly initialised head points anywhere, away from the sun included, where
    cos(incidence) sits on its 1e-5 clamp and cos(acos(1e-5)) cannot be held to 1e-4 in float32 by any implementation (the
    oracle in float32 misses itself in float64 by 15 x the tolerance there; tests/test_relight_cpu.py shows both this and the
    principal-plane jump on the CPU).  rpv111 is left as it is: its normals are analytic (no head to level) and RPV has no
    1 / cos(incidence) term - it holds the tolerance in float32 with back-facing normals.  (The head's sign: normal = -output.)"""
    if "grad_from_xyz.bias" in state:
        b = state["grad_from_xyz.bias"]
        b[2] = b[2] - 6.0
    return state


def l2_normalize64(x):
    eps = float(torch.finfo(torch.float32).eps)
    return x / torch.sqrt(torch.clamp_min((x * x).sum(-1, keepdim=True), eps))


def channels(cfg, apply_brdf, apply_theta):
    """Channel layout of a field output row as the oracle's inference() walks it (oracle/render.py:159-178)."""
    idx, ch = 4 + (1 if cfg.beta else 0), {}
    if cfg.normal in ("analystic", "analystic_learned"):
        ch["normal"] = idx
        idx += 3
    if cfg.normal in ("learned", "analystic_learned"):
        ch["normal"] = idx                              # learned wins when both are present
        idx += 3
    for name in cfg.brdf_head_names(apply_brdf, apply_theta):
        ch[name] = idx
        idx += 1 if name in ("roughness_from_xyz", "theta_from_xyz") else 3
    ch["C"] = idx
    return ch


def oracle_shade(cfg, acc, wsum, rays_d, sun, view=None, apply_brdf=False, apply_theta=False, cos_irra_on=False, dtype=torch.float64):
    """rgb, brdf (K, R, 3) of the ray-level shading (oracle/render.py:194-279, MultiBRDF == 0, no sun pass) from the composited
    sums, with oracle/brdf.py.  view (K, 3): replaces -rays_d."""
    acc, wsum, rays_d, sun = acc.to(dtype).cpu(), wsum.to(dtype).cpu().reshape(-1, 1), rays_d.to(dtype).cpu(), sun.to(dtype).cpu()
    ch = channels(cfg, apply_brdf, apply_theta)
    assert ch["C"] == acc.shape[1], (ch, acc.shape)
    R, pad = acc.shape[0], cfg.rgb_padding
    albedo_s = acc[:, :3] * (1 + 2 * pad) - pad * wsum
    normal_s = l2_normalize64(acc[:, ch["normal"]:ch["normal"] + 3]) if "normal" in ch else None
    col = lambda name, n: acc[:, ch[name]:ch[name] + n] if name in ch else None
    rgbs, brdfs = [], []
    for k in range(sun.shape[0]):
        l = sun[k].expand(R, 3)
        v = -rays_d if view is None else view[k].to(dtype).cpu().expand(R, 3)
        if cfg.roughness and apply_brdf:
            brdf = OB.microfacet(l, v, normal_s, albedo_s, col("roughness_from_xyz", 1), cfg.fresnel_f0)[1]
        elif cfg.RPV and apply_brdf:
            rh = albedo_s if cfg.funcH == 2 else col("rhoc_from_xyz", 3)
            brdf = OB.rpv(l, v, normal_s, albedo_s, col("k_from_xyz", 3), col("theta_rpv_from_xyz", 3), rh)[0]
        elif (apply_brdf and cfg.b == 1) or cfg.shell_hapke > 0:
            th = col("theta_from_xyz", 1)
            brdf = OB.hapke(l, v, normal_s, albedo_s, col("b_from_xyz", 3) if apply_brdf else None,
                            col("c_from_xyz", 3) if apply_brdf else None, None if th is None else th.reshape(-1), cfg.hpk_scl,
                            cfg.shell_hapke)[0]
        else:
            brdf = albedo_s
        irr = sun[k, 2].abs() if (cos_irra_on and normal_s is not None) else 1.0
        rgbs.append((irr * brdf).clamp(0.0, 1.0))
        brdfs.append(brdf)
    return torch.stack(rgbs), torch.stack(brdfs)


def oracle_surface(cfg, rays, seed, apply_brdf=False, apply_theta=False, dtype=torch.float64):
    """acc, wsum, rays_d of the CPU oracle's own render of `rays` (oracle/render.py, parameters make_params(MODEL_SEED)): what the
    directions are checked against on a machine without a GPU."""
    from oracle import render as ORD
    p = {k: torch.from_numpy(v).to(dtype) for k, v in cfg.make_params(MODEL_SEED).items()}
    g = torch.Generator().manual_seed(seed)
    res, _ = ORD.render_rays(p, cfg, rays.to(dtype), ORD.Randoms(generator=g), mode="test", apply_brdf=apply_brdf, apply_theta=apply_theta)
    w = res["weights_coarse"].detach()
    ch = channels(cfg, apply_brdf, apply_theta)
    acc = torch.zeros(rays.shape[0], ch["C"], dtype=dtype)
    ws = lambda t: (w.unsqueeze(-1) * t.detach().reshape(w.shape[0], w.shape[1], -1)).sum(-2)
    acc[:, :3] = ws(res["albedo_coarse"])
    if "normal" in ch:
        key = "normal_lr_coarse" if cfg.normal in ("learned", "analystic_learned") else "normal_an_coarse"
        acc[:, ch["normal"]:ch["normal"] + 3] = ws(res[key])
    names = {"k_from_xyz": "rpv_k", "theta_rpv_from_xyz": "rpv_theta", "rhoc_from_xyz": "rpv_rhoc", "b_from_xyz": "hpk_b",
             "c_from_xyz": "hpk_c", "theta_from_xyz": "hpk_theta", "roughness_from_xyz": "roughness"}
    for name, key in names.items():
        if name in ch:
            t = ws(res[key + "_coarse"])
            acc[:, ch[name]:ch[name] + t.shape[1]] = t
    return acc, w.sum(-1), rays[:, 3:6].to(dtype)

