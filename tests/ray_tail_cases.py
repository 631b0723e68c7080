"""Shared by tests/test_ray_tail_cpu.py and tests/test_gpu_ray_tail_f64.py: the fixed inputs of the ray tail (csrc/ray_tail.hip:
ray_shade_loss_kernel<KIND> behind bn_ray_shade_loss, and lambert_loss_kernel of csrc/render_kernels.hip behind bn_lambert_loss)
and its reference, ray_tail_ref: a plain torch statement of rendering.shade_ray + losses, the BRDF taken from oracle/brdf.py
through brdf_cases._call, evaluated in float64 on the float32 inputs cast exactly, gradients by autograd.  The same statement in
float32 fixes the tolerances (TOL).

Two kinds of table:
  well-posed  CASES: R rows per case, drawn from a seed as brdf_cases._draw draws them and kept only where, in float64, the BRDF's
              margin predicate (brdf_cases.margins) holds for (l, v, normal_s, albedo_s, params) and every irr * brdf_c (from 0
              and from 1), | |depth - td| - ts | and | ts - sqrt(var) | are at least M = 0.02 from their switch: float32 and
              float64 take the same arms.  The composited normal is n * s, s in [0.05, 1]: the normaliser does real work
  on-branch   ON_BRANCH: dyadic rows that sit EXACTLY on a switch (the two clamps of rgb, the three-way depth gate, the
              normaliser's clamp), exact in both precisions; branch_trace names the intermediates that prove the arm

How errors are scaled (compare), for the CPU measurement and the GPU comparison alike:
  per-ray values (rgb [R][3], ray_loss [R])    |err| / (|ref| + s), s = the quantity's largest magnitude in that ray
  batch values (loss, loss_acc per slot)       |err| / (2 |ref|): every entry relative to itself
  gradient entries (d_<group> [R][w], d_wsum, d_depth)
                                               |err| / (|ref| + B), B = the largest magnitude in that ray's block of the group
A zero error counts as 0 whatever the scale; a non-zero error on a zero scale is infinite.  The channels of d_acc that the kind
does not read (unread_channels) must be exactly 0.

Two constants reach the kernel as float32 and the reference as the double they were rounded from: hpk_scl = 1.3 (3.7e-8 of the
value) and f0 = 0.04 (2.2e-8 of the glossy term): both far below every tolerance here.
"""
import math
from types import SimpleNamespace

import torch

import brdf_cases as K
from brdf_nerf_amd import _lib as L, losses
from brdf_nerf_amd.rendering import FP32_EPS, identity_desc, l2_normalize, shade_desc

M = K.M
SENTINEL_ROWS = 64
LAM_RGB, LAM_DS, LAM_HS, PAD = 0.7, 10.0, 0.3, 0.01
KIND_NAME = {L.BN_SHADE_LAMBERT: "lambert", L.BN_SHADE_RPV: "rpv", L.BN_SHADE_HAPKE: "hapke", L.BN_SHADE_MICROFACET: "microfacet"}
KINDS = tuple(KIND_NAME.values())

# Tolerances of the GPU comparison, per (kind, quantity).  Each is 4 x the largest float32-ray_tail_ref-against-float64-ray_tail_ref
# error over the well-posed cases of the kind (CASES, and LL_CASES under "lambert"; the measurement, its case and row stand beside
# it), rounded up to one significant digit; test_ray_tail_cpu.py asserts that the float32 reference stays within HALF of each.  The
# other half is for what the kernel does differently: forward-mode order, the device's transcendentals, atomic order in loss_acc.
TOL_TABLE = {   # (kind, quantity): (TOL, measured float32-against-float64 error, its case, its row)
    ("lambert", "d_albedo"):     (3e-06, 6.398e-07, "lambert_loss S65_C4_R65_on", 60),
    ("lambert", "d_depth"):      (2e-05, 3.263e-06, "lambert_ncos_sunnone_R64", 20),
    ("lambert", "d_wsum"):       (4e-05, 8.179e-06, "lambert_loss S130_C3_R65_off", 44),
    ("lambert", "loss"):         (2e-07, 3.771e-08, "lambert_ncos_sunnone_R64", 0),
    ("lambert", "loss_acc"):     (5e-07, 1.102e-07, "lambert_ncos_sunnone_R64", 46),
    ("lambert", "ray_loss"):     (5e-07, 1.102e-07, "lambert_ncos_sunnone_R64", 46),
    ("lambert", "rgb"):          (3e-07, 6.321e-08, "lambert_irr_R130", 26),
    ("rpv", "d_albedo"):         (2e-04, 4.635e-05, "rpv_t_bothnormals_model_R65", 54),
    ("rpv", "d_depth"):          (2e-06, 4.277e-07, "rpv_ktr_far_R65", 44),
    ("rpv", "d_k"):              (2e-04, 4.509e-05, "rpv_ktr_model_R130", 64),
    ("rpv", "d_normal"):         (3e-04, 5.926e-05, "rpv_ktr_model_R130", 19),
    ("rpv", "d_rhoc"):           (3e-05, 5.552e-06, "rpv_ktr_sunnone_R63", 2),
    ("rpv", "d_theta"):          (2e-04, 4.642e-05, "rpv_t_bothnormals_model_R65", 54),
    ("rpv", "d_wsum"):           (2e-03, 4.413e-04, "rpv_ktr_model_R130", 57),
    ("rpv", "loss"):             (3e-07, 5.093e-08, "rpv_k_beta_unread_R65", 0),
    ("rpv", "loss_acc"):         (3e-07, 7.009e-08, "rpv_none_far_R64", 0),
    ("rpv", "ray_loss"):         (2e-06, 3.079e-07, "rpv_ktr_sunnone_R63", 58),
    ("rpv", "rgb"):              (1e-06, 2.254e-07, "rpv_ktr_far_R65", 58),
    ("hapke", "d_albedo"):       (3e-05, 6.904e-06, "hapke_bct_model_R130", 83),
    ("hapke", "d_b"):            (5e-05, 1.225e-05, "hapke_bct_model_R130", 83),
    ("hapke", "d_c"):            (4e-05, 9.756e-06, "hapke_bct_model_R130", 83),
    ("hapke", "d_depth"):        (1e-05, 2.410e-06, "hapke_bct_model_R130", 38),
    ("hapke", "d_normal"):       (9e-05, 2.211e-05, "hapke_bct_model_R130", 83),
    ("hapke", "d_theta"):        (2e-04, 3.379e-05, "hapke_bct_model_R130", 83),
    ("hapke", "d_wsum"):         (5e-04, 1.157e-04, "hapke_bct_model_R130", 53),
    ("hapke", "loss"):           (4e-07, 7.737e-08, "hapke_bc_far_R64", 0),
    ("hapke", "loss_acc"):       (4e-07, 7.960e-08, "hapke_b_beta_model_R65", 7),
    ("hapke", "ray_loss"):       (1e-06, 2.272e-07, "hapke_bc_far_R64", 47),
    ("hapke", "rgb"):            (5e-06, 1.132e-06, "hapke_bct_model_R130", 83),
    ("microfacet", "d_albedo"):  (2e-06, 4.332e-07, "microfacet_model_R130", 81),
    ("microfacet", "d_depth"):   (9e-06, 2.230e-06, "microfacet_model_R130", 40),
    ("microfacet", "d_normal"):  (5e-04, 1.018e-04, "microfacet_model_R130", 94),
    ("microfacet", "d_rough"):   (5e-04, 1.016e-04, "microfacet_model_R130", 94),
    ("microfacet", "d_wsum"):    (5e-04, 1.014e-04, "microfacet_model_R130", 94),
    ("microfacet", "loss"):      (2e-07, 2.511e-08, "microfacet_model_R130", 0),
    ("microfacet", "loss_acc"):  (3e-07, 7.024e-08, "microfacet_model_R130", 33),
    ("microfacet", "ray_loss"):  (5e-07, 1.091e-07, "microfacet_far_R65", 12),
    ("microfacet", "rgb"):       (4e-07, 7.994e-08, "microfacet_far_R65", 61),
}
TOL = {k: v[0] for k, v in TOL_TABLE.items()}
# Gradient entries left out of the comparison on the well-posed tables: none (so the cap of 1 % of a case's gradient entries, and
# never a whole ray, holds trivially: EXCLUDED is the list the tests read, and it is empty).
EXCLUDED_SHARE = 0.0
EXCLUDED = {}                  # case -> [(ray, group, column, reason)]
EXCLUDED_CAP = 0.01
# On-branch (table, row, quantity) triples where the float32 reference ITSELF misses TOL / 2 against the float64 reference, each
# with the measurement and the derived bound it is held to instead; test_ray_tail_cpu.py pins the list both ways.
#   ob_rpv / n_zero / d_rhoc   a zero composited normal gives normal_s = 0 and ci = cv = 1e-5, the clamped arm of brdf_cases' rows
#                               sun_back and view_back: d_rhoc reads 1 / tan(acos(1e-5)) through G, which float32 returns with up to
#                               1.2e-2 of itself (brdf_cases.ACOS_TOL, derived there and reused as it is)
ILL = {  # (table, row, quantity): (measured float32 reference vs float64 reference, what it is, bound)
    ("ob_rpv", "n_zero", "d_rhoc"): (1.51e-03, "G of ci = cv = 1e-5", K.on_branch_bound("rpv", "sun_back", "d_rhoc")),
}
# On-branch entries where reverse-mode autograd of the float64 statement is itself not finite, and what must hold there instead.
# A zero composited normal under the microfacet BRDF is brdf_cases' row n_0: d = nan_to_num(0 / (0 * inf)) is replaced by 0 and is
# the normal's and the roughness' only path to the value, so both gradients are exactly 0 (brdf_cases.REPLACED_ZERO); autograd
# multiplies the zero it sends into the replaced graph by an infinite local derivative.  Everywhere else a non-finite reference
# entry must be non-finite on the device too.
REPLACED_ZERO = {("ob_microfacet", "n_zero"): ("normal", "rough")}


# ------------------------------------------------------------------------------------------------ descriptors
_INT = ("kind", "C", "ch_normal", "ch_p0", "ch_p1", "ch_p2", "rhoc_is_albedo", "shell", "cos_irradiance", "usealldepth")
_FLT = ("hpk_scl", "f0", "rgb_padding", "lambda_rgb", "lambda_ds", "lambda_hs")


def hand_desc(kind, C, ch_normal=-1, p=(-1, -1, -1), rhoc_is_albedo=0, shell=0, cos=0, usealldepth=0, hpk_scl=4.0, pad=PAD,
              lam=(LAM_RGB, LAM_DS, LAM_HS)):
    """An L.ShadeDesc filled by hand: layouts that no model produces."""
    d = L.ShadeDesc()
    d.kind, d.C, d.ch_normal = {v: k for k, v in KIND_NAME.items()}[kind], C, ch_normal
    d.ch_p0, d.ch_p1, d.ch_p2 = p
    d.rhoc_is_albedo, d.shell, d.cos_irradiance, d.usealldepth = rhoc_is_albedo, shell, cos, usealldepth
    d.hpk_scl, d.f0, d.rgb_padding = hpk_scl, K.F0, pad
    d.lambda_rgb, d.lambda_ds, d.lambda_hs = lam
    d.irr, d.irr_stride = None, 0
    return d


def copy_desc(d):
    """A fresh L.ShadeDesc with d's fields and no irradiance pointer."""
    o = L.ShadeDesc()
    for k in _INT + _FLT:
        setattr(o, k, getattr(d, k))
    o.irr, o.irr_stride = None, 0
    return o


_MODEL_CFGS = {   # name -> (FieldConfig flags, apply_brdf, beta)
    "plain": (dict(), False, False),
    "normal_only": (dict(normal="learned"), False, False),
    "rpv111_nlr": (dict(funcM=1, funcF=1, funcH=1, normal="learned"), True, False),
    "rpv_m1f1h2_nan": (dict(funcM=1, funcF=1, funcH=2, normal="analystic"), True, False),
    "rpv_f1_nanlr": (dict(funcF=1, normal="analystic_learned"), True, False),
    "hapke_bct": (dict(b=1, c=1, theta=1, normal="learned"), True, False),
    "hapke_b_beta": (dict(b=1, normal="analystic", beta=True), True, True),
    "hapke_shell3_nobrdf": (dict(shell_hapke=3, normal="learned"), False, False),
    "microfacet": (dict(roughness=True, normal="analystic"), True, False),
}


def model_desc(name, cos=1, usealldepth=0, lam=(LAM_RGB, LAM_DS, LAM_HS)):
    """rendering.shade_desc of a model built on the CPU (the descriptor reads the model's flags and its spec's layout alone)."""
    from oracle.config import FieldConfig
    from test_gpu_parity import make_args
    from brdf_nerf_amd import load_model
    kw, brdf, beta = _MODEL_CFGS[name]
    cfg = FieldConfig(feat=64, n_samples=16, guided_samples=16, **kw)
    args = make_args(cfg)
    model = load_model(args)
    spec = model.spec(brdf, brdf, cfg.normal in ("learned", "analystic_learned"), cfg.normal in ("analystic", "analystic_learned"), beta=beta)
    return shade_desc(model, args, spec, brdf, bool(cos), lam[0], lam[1], lam[2], bool(usealldepth))


def kind_of(d):
    return KIND_NAME[d.kind]


def groups_of(d):
    """{group: (first channel, width)} of the composited channels the kind reads, in slot order."""
    kind = kind_of(d)
    g = {"albedo": (0, 3)}
    if kind == "lambert":
        return g
    g["normal"] = (d.ch_normal, 3)
    heads = {"rpv": (("k", 3), ("theta", 3), ("rhoc", 3)), "hapke": (("b", 3), ("c", 3), ("theta", 1)), "microfacet": (("rough", 1),)}[kind]
    for (name, w), ch in zip(heads, (d.ch_p0, d.ch_p1, d.ch_p2)):
        if ch >= 0 and not (name == "rhoc" and d.rhoc_is_albedo):
            g[name] = (ch, w)
    return g


def unread_channels(d):
    """The channels of d_acc that must be exactly 0: sigma, the losing normal field, beta, heads the kind does not read."""
    read = {c for c0, w in groups_of(d).values() for c in range(c0, c0 + w)}
    return [c for c in range(d.C) if c not in read]


def variant_of(d):
    """The brdf_cases variant that a descriptor selects (None: Lambert)."""
    kind, g = kind_of(d), groups_of(d)
    if kind == "lambert":
        return None
    if kind == "microfacet":
        return "microfacet"
    if kind == "rpv":
        return "rpv/" + ("".join(h for h, n in zip("ktr", ("k", "theta", "rhoc")) if n in g) or "none")
    scl = round(d.hpk_scl, 4)
    heads = "".join(h for h, n in zip("bct", ("b", "c", "theta")) if n in g)
    return f"hapke/{heads}/{scl}" if "b" in g else f"hapke/s{d.shell}{'t' if 'theta' in g else ''}/{scl}"


# ------------------------------------------------------------------------------------------------ the reference
def ray_tail_ref(d, acc, wsum, depth, var, rays_d, sun_d, irr, rgbs, prior, extra_loss, dtype, zw=None, slots=1):
    """What bn_ray_shade_loss computes, as torch statements in `dtype`.  d: an L.ShadeDesc or anything with its fields.  prior:
    (valid, target_depth, target_weight, target_std) or None.  zw = (z, w) [R][S] with sum_s w_s z_s = depth: the HardSurfaceLoss
    gradient is that of the per-sample statement sum_s w_s (z_s - depth)^2; without it the closed form -2 lambda_hs / R (depth -
    depth wsum) that this identity gives.  The term's VALUE is lambda_hs / R * var of the given var, as the kernel reads it.
    -> rgb, x (before the clamp), ray_loss, loss, loss_acc [slots], d_acc, d_wsum, d_depth, and normal_s / albedo_s / brdf."""
    c = lambda t: None if t is None else t.detach().to(dtype)
    acc, wsum, depth = (c(t).clone().requires_grad_(True) for t in (acc, wsum, depth))
    var, rays_d, sun_d, irr, rgbs, extra = (c(t) for t in (var, rays_d, sun_d, irr, rgbs, extra_loss))
    R, kind, pad = acc.shape[0], kind_of(d), d.rgb_padding
    albedo_s = acc[:, :3] * (1 + 2 * pad) - pad * wsum.unsqueeze(-1)
    has_n = d.ch_normal >= 0
    sun = torch.ones(R, 3, dtype=dtype) if sun_d is None else sun_d
    irr_ray = sun[:, 2:3].abs() if (d.cos_irradiance and has_n) else (None if irr is None else irr.unsqueeze(-1))
    normal_s = None
    with K._float32_infinities():
        if kind == "lambert":
            brdf = albedo_s
        else:
            variant = variant_of(d)
            assert abs(d.f0 - K.F0) < 1e-8 and abs(d.hpk_scl - K.VARIANTS[variant].get("hpk_scl", d.hpk_scl)) < 1e-6
            normal_s = l2_normalize(acc[:, d.ch_normal:d.ch_normal + 3])          # FP32_EPS is the clamp in every dtype
            x = {"n": normal_s, ("albedo" if kind == "microfacet" else "w"): albedo_s}
            for g, (c0, w) in groups_of(d).items():
                if g not in ("albedo", "normal"):
                    x[g] = acc[:, c0] if (kind == "hapke" and g == "theta") else acc[:, c0:c0 + w]
            brdf, _ = K._call(variant, sun, -rays_d, x, bool(d.rhoc_is_albedo))
        xr = brdf if irr_ray is None else irr_ray * brdf
        rgb = xr.clamp(0.0, 1.0)
        total = losses.snerf_loss(rgb, rgbs, d.lambda_rgb)
        ray_loss = d.lambda_rgb * ((rgb - rgbs) ** 2).sum(-1) / (3.0 * R)
        if prior is not None and d.lambda_ds > 0:
            valid, td, tw, ts = (c(t) for t in prior)
            # losses.depth_loss forms std = sqrt(sum_s w_s (z_s - depth)^2): one sample at depth + 1 with weight var makes that
            # sqrt(var) of the GIVEN var (exactly so in float64, and in float32 wherever depth + 1 is exact: the on-branch rows)
            total = total + losses.depth_loss((depth.detach() + 1).unsqueeze(-1), depth, var.unsqueeze(-1), td, tw, valid, ts,
                                              d.lambda_ds, bool(d.usealldepth))
            apply = valid > 0
            if not d.usealldepth:
                apply = apply & ((((depth - td).abs() - ts) > 0) | (ts < var.sqrt()))
            ray_loss = ray_loss + torch.where(apply, (d.lambda_ds / 3.0 / R) * tw * (depth - td) ** 2, torch.zeros_like(td))
        if d.lambda_hs > 0:
            k = d.lambda_hs / R
            if zw is not None:
                z, w = c(zw[0]), c(zw[1])
                per = k * (w * (z - depth.unsqueeze(-1)) ** 2).sum(-1)
            else:
                per = -2 * k * (depth.detach() - depth.detach() * wsum.detach()) * depth
            hs = k * var + (per - per.detach())              # the value of the given var, the gradient of the per-sample statement
            total, ray_loss = total + hs.sum(), ray_loss + hs
        if extra is not None:
            total, ray_loss = total + extra.sum(), ray_loss + extra
        gr = torch.autograd.grad(total, [acc, wsum, depth], allow_unused=True)
    d_acc, d_wsum, d_depth = (torch.zeros_like(t) if g_ is None else g_ for g_, t in zip(gr, (acc, wsum, depth)))
    loss_acc = torch.zeros(slots, dtype=dtype).index_add_(0, torch.arange(R) % slots, ray_loss.detach())
    det = lambda t: None if t is None else t.detach()
    return {"rgb": rgb.detach(), "x": xr.detach(), "ray_loss": ray_loss.detach(), "loss": total.detach(), "loss_acc": loss_acc,
            "d_acc": d_acc, "d_wsum": d_wsum, "d_depth": d_depth, "normal_s": det(normal_s), "albedo_s": albedo_s.detach(),
            "brdf": brdf.detach()}


# ------------------------------------------------------------------------------------------------ error scaling
_worse = lambda a, b: a if (a[0] != a[0] or (b[0] == b[0] and a[0] >= b[0])) else b


def compare(got, ref, d, masks=None):
    """-> {quantity: (scaled error, row)} of whatever `got` holds among rgb, ray_loss, loss, loss_acc, d_acc (one entry per input
    group: d_albedo, d_normal, d_<head>), d_wsum, d_depth.  masks: {quantity: bool tensor}, the entries to compare (on-branch rows:
    what is finite in float64)."""
    m = lambda q: None if masks is None else masks.get(q)
    col = lambda t: t.reshape(-1, 1)
    e = {}
    if "rgb" in got:
        e["rgb"] = K.err_rows(got["rgb"], ref["rgb"], m("rgb"))
    for q in ("ray_loss", "loss", "loss_acc", "d_wsum", "d_depth"):
        if got.get(q) is not None:
            e[q] = K.err_rows(col(got[q]), col(ref[q]), None if m(q) is None else col(m(q)))
    if "d_acc" in got:
        for g, (c0, w) in groups_of(d).items():
            e["d_" + g] = K.err_rows(got["d_acc"][:, c0:c0 + w], ref["d_acc"][:, c0:c0 + w], None if m("d_acc") is None else m("d_acc")[:, c0:c0 + w])
    return e


def finite_masks(ref):
    fin = torch.isfinite
    return {q: fin(ref[q]) for q in ("rgb", "ray_loss", "loss", "loss_acc", "d_acc", "d_wsum", "d_depth")}


def nonzero_unread(d_acc, d):
    """How many entries of the channels the kind does not read are not exactly 0 (NaN counts)."""
    ch = unread_channels(d)
    return int((d_acc.detach().cpu()[:, ch] != 0).sum()) if ch else 0


# ------------------------------------------------------------------------------------------------ the well-posed tables
_F32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
DRAW_BATCH = 512


def _candidates(d, g, n, sun_none, lambert_wide=True):
    """n candidate rays for descriptor d, float32: directions, normal and parameters as brdf_cases._draw draws them, the composited
    normal n * s, everything else at random."""
    U = lambda *shape: torch.rand(*shape, generator=g)
    kind = kind_of(d)
    fam = "microfacet" if kind == "lambert" else kind
    t = K._draw(fam, g, n)
    if sun_none:
        t["l"] = torch.ones(n, 3)
    alb = t["albedo" if fam == "microfacet" else "w"]
    if kind == "lambert":
        alb = 1.6 * alb - 0.3                                    # a Lambertian colour reaches both sides of the clamp
    wsum = 0.3 + 0.65 * U(n)
    acc = U(n, d.C)
    pad = d.rgb_padding
    acc[:, :3] = (alb + pad * wsum[:, None]) / (1 + 2 * pad)
    if d.ch_normal >= 0:
        acc[:, d.ch_normal:d.ch_normal + 3] = t["n"] * (0.05 + 0.95 * U(n, 1))
    for name, (c0, w) in groups_of(d).items():
        if name not in ("albedo", "normal"):
            acc[:, c0:c0 + w] = t[name].reshape(n, -1)
    depth = 1 + 2 * U(n)
    # a real (z, w) pair per ray with sum w = wsum and sum w z = depth, in float64 (the third sample closes both sums)
    w12 = wsum.double()[:, None] * (0.1 + 0.3 * U(n, 2).double())
    z12 = depth.double()[:, None] + 0.6 * (U(n, 2).double() - 0.5)
    w3 = wsum.double() - w12.sum(-1)
    z3 = (depth.double() - (w12 * z12).sum(-1)) / w3
    w, z = torch.cat([w12, w3[:, None]], -1), torch.cat([z12, z3[:, None]], -1)
    var = (w * (z - depth.double()[:, None]) ** 2).sum(-1).float()
    rays = U(n, 11)
    rays[:, 3:6], rays[:, 8:11] = -t["v"], t["l"]
    # (sum w z = depth with sum w < 1 puts the closing sample far out: sqrt(var) is of the order of depth, and so is the prior's spread)
    ptab = torch.stack([torch.ones(n), depth + torch.randn(n, generator=g), U(n), 0.02 + 2.5 * U(n)], -1)
    irr = torch.stack([0.5 + 0.7 * U(n), U(n)], -1)
    return dict(acc=acc, wsum=wsum, depth=depth, var=var, rays=rays, ptab=ptab, irr=irr, rgbs=U(n, 3), extra=0.01 * U(n), z=z, w=w,
                params={k: a for k, a in t.items() if k not in ("l", "v", "n", "d_brdf")})


def case_margins(d, rows, sun_none, use_irr):
    """bool [n]: the margin predicate of the module docstring on `rows`, judged in float64 alone."""
    r = ray_tail_ref(d, rows["acc"], rows["wsum"], rows["depth"], rows["var"], rows["rays"][:, 3:6], None if sun_none else rows["rays"][:, 8:11],
                     rows["irr"][:, 0] if use_irr else None, rows["rgbs"], None, None, torch.float64)
    x = r["x"]
    ok = torch.isfinite(x).all(-1) & (x.abs() >= M).all(-1) & ((x - 1).abs() >= M).all(-1)
    kind = kind_of(d)
    if kind != "lambert":
        n = x.shape[0]
        tab = dict(rows["params"], l=torch.ones(n, 3) if sun_none else rows["rays"][:, 8:11], v=-rows["rays"][:, 3:6], n=r["normal_s"])
        tab["albedo" if kind == "microfacet" else "w"] = r["albedo_s"]
        if d.rhoc_is_albedo:
            tab["rhoc"] = r["albedo_s"]
        ok &= K.margins(kind, tab)
    depth, td, ts = rows["depth"].double(), rows["ptab"][:, 1].double(), rows["ptab"][:, 3].double()
    ok &= (((depth - td).abs() - ts).abs() >= M) & ((ts - rows["var"].double().sqrt()).abs() >= M)
    return ok


def _take(rows, idx):
    return {k: ({q: a[idx] for q, a in v.items()} if isinstance(v, dict) else v[idx]) for k, v in rows.items()}


def build_case(name, d, R, seed, prior="off", irr=None, sun_none=False, strided=True, extra=False, slots=1):
    """The first R rays of the seeded draw that keep the margin.  prior: off / strided / contiguous (the four operands as column
    views of one [R][4] table, or as vectors); irr: None / strided / contiguous; strided: rays_d / sun_d as columns of the [R][11]
    ray table, or contiguous copies."""
    g = torch.Generator().manual_seed(seed)
    kept, drawn = None, 0
    while kept is None or kept["acc"].shape[0] < R:
        rows = _candidates(d, g, DRAW_BATCH, sun_none)
        ok = case_margins(d, rows, sun_none, irr is not None)
        drawn += DRAW_BATCH
        assert drawn <= 200 * DRAW_BATCH, name
        rows = _take(rows, ok)
        kept = rows if kept is None else {k: ({q: torch.cat([kept[k][q], a]) for q, a in v.items()} if isinstance(v, dict) else torch.cat([kept[k], v]))
                                          for k, v in rows.items()}
    c = {k: ({q: a.contiguous() for q, a in v.items()} if isinstance(v, dict) else v.contiguous()) for k, v in _take(kept, slice(0, R)).items()}
    c["ptab"][:, 0] = torch.tensor([1.0, 0.0, -1.0, 1.0, 2.5])[torch.arange(R) % 5]       # valid: 0, 1, a negative value
    c.update(name=name, desc=d, R=R, prior=prior, irr_form=irr, sun_none=sun_none, strided=strided, use_extra=extra, slots=slots, drawn=drawn)
    return c


def ref_args(c):
    """The operands of ray_tail_ref for a case (float32 CPU tensors), after the descriptor."""
    p = c["ptab"]
    return dict(acc=c["acc"], wsum=c["wsum"], depth=c["depth"], var=c["var"], rays_d=c["rays"][:, 3:6], sun_d=None if c["sun_none"] else c["rays"][:, 8:11],
                irr=None if c["irr_form"] is None else c["irr"][:, 0], rgbs=c["rgbs"], prior=None if c["prior"] == "off" else (p[:, 0], p[:, 1], p[:, 2], p[:, 3]),
                extra_loss=c["extra"] if c["use_extra"] else None)


def case_reference(c, dtype, **over):
    a = dict(ref_args(c), **over)
    return ray_tail_ref(c["desc"], a["acc"], a["wsum"], a["depth"], a["var"], a["rays_d"], a["sun_d"], a["irr"], a["rgbs"], a["prior"],
                        a["extra_loss"], dtype, zw=(c["z"], c["w"]), slots=c["slots"])


NO_DS, NO_HS = (LAM_RGB, 0.0, LAM_HS), (LAM_RGB, LAM_DS, 0.0)


def _specs():
    """name -> (descriptor factory, build_case keywords).  The ray count stands at the end of each name."""
    H, Md, I = hand_desc, model_desc, identity_desc
    s = {
        # ---- Lambert, identity
        "lambert_plain_R1": (lambda: Md("plain", lam=(LAM_RGB, 0.0, 0.0)), dict(strided=False)),
        "lambert_ncos_R63": (lambda: Md("normal_only"), dict(prior="strided", slots=8)),
        "lambert_ncos_sunnone_R64": (lambda: Md("normal_only", usealldepth=1), dict(prior="contiguous", sun_none=True, slots=64)),
        "identity_R65": (lambda: I(7, LAM_RGB, LAM_DS, LAM_HS), dict(prior="strided", extra=True, slots=7)),
        "lambert_irr_R130": (lambda: H("lambert", 5, lam=NO_HS), dict(prior="contiguous", irr="strided", extra=True, slots=8, strided=False)),
        # ---- RPV
        "rpv_none_far_R64": (lambda: H("rpv", 32, 29, lam=(LAM_RGB, 0.0, 0.0)), dict()),
        "rpv_k_beta_unread_R65": (lambda: H("rpv", 16, 8, (11, -1, -1), cos=1), dict(prior="strided", slots=8)),   # 4-6 losing normal, 7 beta, 14-15 unread
        "rpv_kt_far_R63": (lambda: H("rpv", 32, 20, (29, 26, -1), lam=NO_HS), dict(prior="contiguous", strided=False)),
        "rpv_ktr_model_R130": (lambda: Md("rpv111_nlr"), dict(prior="strided", extra=True, slots=64)),
        "rpv_ktr_far_R65": (lambda: H("rpv", 32, 29, (23, 26, 20), usealldepth=1), dict(prior="contiguous", irr="contiguous", slots=3)),
        "rpv_kt_h2_model_R64": (lambda: Md("rpv_m1f1h2_nan"), dict(prior="strided", slots=8)),
        "rpv_kt_h2_p2set_R63": (lambda: H("rpv", 16, 4, (7, 10, 13), rhoc_is_albedo=1, lam=NO_DS), dict(irr="strided")),
        "rpv_t_bothnormals_model_R65": (lambda: Md("rpv_f1_nanlr", lam=NO_HS), dict(prior="strided", extra=True)),
        "rpv_ktr_sunnone_R63": (lambda: Md("rpv111_nlr", lam=NO_DS), dict(sun_none=True, slots=8)),
        # ---- Hapke
        "hapke_b_beta_model_R65": (lambda: Md("hapke_b_beta"), dict(prior="strided", slots=8)),
        "hapke_bc_far_R64": (lambda: H("hapke", 32, 29, (26, 22, -1), lam=NO_HS), dict(prior="contiguous", irr="strided", strided=False)),
        "hapke_bct_model_R130": (lambda: Md("hapke_bct", usealldepth=1), dict(prior="strided", extra=True, slots=64)),
        "hapke_bct_far_scl13_R63": (lambda: H("hapke", 32, 28, (22, 25, 31), hpk_scl=1.3, cos=1), dict(prior="strided", slots=5)),
        "hapke_s1_R1": (lambda: H("hapke", 7, 4, shell=1, lam=NO_DS), dict(strided=False)),
        "hapke_s2_R65": (lambda: H("hapke", 8, 5, shell=2, cos=1), dict(prior="contiguous", extra=True)),
        "hapke_s3_model_R64": (lambda: Md("hapke_shell3_nobrdf", lam=NO_HS), dict(prior="strided", slots=8)),
        # ---- microfacet
        "microfacet_model_R130": (lambda: Md("microfacet"), dict(prior="strided", extra=True, slots=64)),
        "microfacet_far_R65": (lambda: H("microfacet", 32, 28, (31, -1, -1), usealldepth=1), dict(prior="contiguous", irr="strided", slots=8, strided=False)),
    }
    return s


SPECS = _specs()
CASE_NAMES = list(SPECS)
_CACHE = {}


def case(name):
    """The shared, unchanged well-posed case `name`, built once."""
    if name not in _CACHE:
        f, kw = SPECS[name]
        _CACHE[name] = build_case(name, f(), int(name.rsplit("_R", 1)[1]), 9000 + CASE_NAMES.index(name), **kw)
    return _CACHE[name]


def reference(name):
    """The float64 reference of a well-posed case, computed once."""
    if ("ref", name) not in _CACHE:
        _CACHE[("ref", name)] = case_reference(case(name), torch.float64)
    return _CACHE[("ref", name)]


# ------------------------------------------------------------------------------------------------ bn_lambert_loss
LL_CASES = {f"S{S}_C{C}_R{R}_{p}": dict(S=S, C=C, R=R, prior=p) for S, C, R, p in
            ((1, 3, 1, "off"), (63, 4, 7, "on"), (64, 7, 65, "all"), (65, 32, 7, "on"), (130, 3, 65, "off"), (130, 32, 1, "all"), (65, 4, 65, "on"),
             (1, 7, 7, "all"))}


def ll_desc(c):
    """The fields of a Lambertian descriptor that states bn_lambert_loss: floats as the C entry point receives them."""
    on = c["prior"] != "off"
    return SimpleNamespace(kind=L.BN_SHADE_LAMBERT, C=c["C"], ch_normal=-1, ch_p0=-1, ch_p1=-1, ch_p2=-1, rhoc_is_albedo=0, shell=0, cos_irradiance=0,
                           usealldepth=int(c["prior"] == "all"), hpk_scl=1.0, f0=K.F0, rgb_padding=_F32(PAD), lambda_rgb=_F32(LAM_RGB),
                           lambda_ds=_F32(LAM_DS) if on else 0.0, lambda_hs=0.0)


def ll_reference(c, dtype):
    """ray_tail_ref's Lambert arm on wsum and var formed from the samples in `dtype`."""
    w, z, depth = c["weights"].to(dtype), c["z"].to(dtype), c["depth"].to(dtype)
    p = c["ptab"]
    return ray_tail_ref(ll_desc(c), c["acc"], w.sum(-1), depth, (w * (z - depth.unsqueeze(-1)) ** 2).sum(-1), None, None, None, c["rgbs"],
                        None if c["prior"] == "off" else (p[:, 0], p[:, 1], p[:, 2], p[:, 3]), None, dtype)


def ll_case(name):
    """R rays of S samples that keep the margin (the colour from 0 and 1, both gate clauses), from a fixed seed."""
    if ("ll", name) in _CACHE:
        return _CACHE[("ll", name)]
    c = dict(LL_CASES[name], name=name)
    S, C, R = c["S"], c["C"], c["R"]
    g = torch.Generator().manual_seed(9500 + list(LL_CASES).index(name))
    U = lambda *shape: torch.rand(*shape, generator=g)
    kept, drawn = None, 0
    while kept is None or kept["acc"].shape[0] < R:
        n = 256
        w = U(n, S) + 0.05
        w = w / w.sum(-1, keepdim=True) * (0.3 + 0.65 * U(n, 1))
        z = torch.sort(1 + 2 * U(n, S), -1)[0]
        depth = (w * z).sum(-1) / w.sum(-1) + 0.2 * (U(n) - 0.5)
        acc = U(n, C)
        acc[:, :3] = (1.6 * U(n, 3) - 0.3 + PAD * w.sum(-1, keepdim=True)) / (1 + 2 * PAD)
        ptab = torch.stack([torch.ones(n), depth + 0.5 * torch.randn(n, generator=g), U(n), 0.02 + 0.8 * U(n)], -1)
        rows = dict(acc=acc, weights=w, z=z, depth=depth, ptab=ptab, rgbs=U(n, 3))
        r = ll_reference(dict(c, **rows), torch.float64)
        var = (w.double() * (z.double() - depth.double()[:, None]) ** 2).sum(-1)
        td, ts = ptab[:, 1].double(), ptab[:, 3].double()
        ok = (r["x"].abs() >= M).all(-1) & ((r["x"] - 1).abs() >= M).all(-1)
        ok &= (((depth.double() - td).abs() - ts).abs() >= M) & ((ts - var.sqrt()).abs() >= M)
        drawn += n
        rows = _take(rows, ok)
        kept = rows if kept is None else {k: torch.cat([kept[k], v]) for k, v in rows.items()}
    c.update({k: v[:R].contiguous() for k, v in kept.items()}, drawn=drawn)
    c["ptab"][:, 0] = torch.tensor([1.0, 0.0, -1.0, 1.0, 2.5])[torch.arange(R) % 5]
    _CACHE[("ll", name)] = c
    return c


def ll_reference64(name):
    if ("llref", name) not in _CACHE:
        _CACHE[("llref", name)] = ll_reference(ll_case(name), torch.float64)
    return _CACHE[("llref", name)]


# ------------------------------------------------------------------------------------------------ the on-branch tables
_E = 2.0 ** -20
# (row name, x = the colour before the clamp, depth, target depth, target std, var, valid): a clamp row keeps the gate far off, a
# gate row keeps the colour inside
_OB_LAMBERT_ROWS = [
    ("x_on_0_and_1", (0.0, 1.0, 0.5), 2.0, 1.0, 0.5, 0.0625, 1.0),        # the gradient passes, as torch.clamp's does
    ("x_just_outside", (-_E, 1.0 + _E, 0.5), 2.0, 1.0, 0.5, 0.0625, 1.0),
    ("x_just_inside", (_E, 1.0 - _E, 0.5), 2.0, 1.0, 0.5, 0.0625, 1.0),
    ("gate1_at_0_std_below", (0.25, 0.5, 0.75), 2.0, 1.5, 0.5, 0.0625, 1.0),   # |depth - td| - ts == 0, ts = 0.5 > 0.25: not applied
    ("gate2_at_equal", (0.25, 0.5, 0.75), 2.0, 1.75, 0.5, 0.25, 1.0),          # ts == sqrt(var), |depth - td| - ts < 0: not applied
    ("gate1_alone", (0.25, 0.5, 0.75), 2.0, 1.0, 0.5, 0.0625, 1.0),            # 1 - 0.5 > 0, ts > sqrt(var)
    ("gate2_alone", (0.25, 0.5, 0.75), 2.0, 1.75, 0.25, 0.25, 1.0),            # 0.25 - 0.25 == 0, ts = 0.25 < 0.5
    ("valid_0", (0.25, 0.5, 0.75), 2.0, 1.0, 0.25, 0.25, 0.0),                 # both clauses on, no valid prior
    ("valid_negative", (0.25, 0.5, 0.75), 2.0, 1.0, 0.25, 0.25, -1.0),
]
EXPECTED_TRACE = {
    "x_on_0_and_1": {"x0 == 0": True, "x1 == 1": True, "passes": (True, True, True), "applied": True},
    "x_just_outside": {"x0 < 0": True, "x1 > 1": True, "passes": (False, False, True), "applied": True},
    "x_just_inside": {"x0 > 0": True, "x1 < 1": True, "passes": (True, True, True), "applied": True},
    "gate1_at_0_std_below": {"|depth - td| - ts == 0": True, "ts > std": True, "applied": False},
    "gate2_at_equal": {"|depth - td| - ts < 0": True, "ts == std": True, "applied": False},
    "gate1_alone": {"|depth - td| - ts > 0": True, "ts > std": True, "applied": True},
    "gate2_alone": {"|depth - td| - ts == 0": True, "ts < std": True, "applied": True},
    "valid_0": {"|depth - td| - ts > 0": True, "ts < std": True, "valid > 0": False, "applied": False},
    "valid_negative": {"|depth - td| - ts > 0": True, "ts < std": True, "valid > 0": False, "applied": False},
    "n_zero": {"|n|^2 == 0": True, "clamped": True, "normal_s == 0": True},
    "n_below_eps": {"|n|^2 < eps": True, "clamped": True, "|normal_s| < 1": True},
    "n_control": {"|n|^2 < eps": False, "clamped": False, "|normal_s| == 1": True},
}
_OB_NORMAL_ROWS = [("n_zero", (0.0, 0.0, 0.0)), ("n_below_eps", (0.0, 0.0, 2.0 ** -12)), ("n_control", (0.0, 0.0, 0.5))]
_OB_BRDF = {"ob_rpv": ("rpv", (7, 10, 13)), "ob_hapke": ("hapke", (7, 10, 13)), "ob_microfacet": ("microfacet", (7, -1, -1))}
ON_BRANCH = ("ob_identity", "ob_lambert_pad") + tuple(_OB_BRDF)


def on_branch(name):
    """-> (case, row names).  ob_identity: identity_desc, x = acc.  ob_lambert_pad: rgb_padding = 0.5 and wsum = 1, x = 2 acc - 0.5
    exactly.  ob_<kind>: the dyadic geometry and parameters of brdf_cases (_L0, _V0, _BASE), the composited normal of the row."""
    if ("ob", name) in _CACHE:
        return _CACHE[("ob", name)]
    T = lambda rows: torch.tensor(rows, dtype=torch.float32)
    if name in ("ob_identity", "ob_lambert_pad"):
        names = [r[0] for r in _OB_LAMBERT_ROWS]
        R = len(names)
        pad = 0.0 if name == "ob_identity" else 0.5
        d = identity_desc(5, LAM_RGB, LAM_DS, LAM_HS) if pad == 0 else hand_desc("lambert", 5, pad=0.5)
        acc = torch.full((R, 5), 0.375)
        acc[:, :3] = T([r[1] for r in _OB_LAMBERT_ROWS]) / (1 + 2 * pad) + pad / (1 + 2 * pad)
        cols = [T([r[i] for r in _OB_LAMBERT_ROWS]) for i in (2, 3, 4, 5, 6)]
        depth, td, ts, var, valid = cols
        wsum = torch.ones(R)
        rays = torch.full((R, 11), 0.5)
    else:
        kind, p = _OB_BRDF[name]
        names = [r[0] for r in _OB_NORMAL_ROWS]
        R = len(names)
        d = hand_desc(kind, 16, 4, p, pad=0.0)
        acc = torch.full((R, 16), 0.375)
        base = K._BASE[kind]
        acc[:, :3] = T(base["albedo" if kind == "microfacet" else "w"])
        acc[:, 4:7] = T([r[1] for r in _OB_NORMAL_ROWS])
        for g, (c0, w) in groups_of(d).items():
            if g not in ("albedo", "normal"):
                acc[:, c0:c0 + w] = T(base[g])
        depth, td, ts, var, valid = (torch.full((R,), v) for v in (2.0, 1.0, 0.5, 0.0625, 1.0))
        wsum = torch.full((R,), 0.75)
        rays = torch.full((R, 11), 0.5)
        rays[:, 3:6], rays[:, 8:11] = -T(K._V0), T(K._L0)
    c = dict(name=name, desc=d, R=R, acc=acc, wsum=wsum, depth=depth, var=var, rays=rays.contiguous(),
             ptab=torch.stack([valid, td, T([0.5] * R), ts], -1).contiguous(), irr=torch.ones(R, 2), rgbs=T([[0.5, 0.25, 0.625]] * R),
             extra=torch.zeros(R), prior="strided", irr_form=None, sun_none=False, strided=True, use_extra=False, slots=1, z=None, w=None)
    _CACHE[("ob", name)] = (c, names)
    return c, names


def ob_reference(c, dtype):
    a = ref_args(c)
    return ray_tail_ref(c["desc"], a["acc"], a["wsum"], a["depth"], a["var"], a["rays_d"], a["sun_d"], a["irr"], a["rgbs"], a["prior"],
                        a["extra_loss"], dtype, slots=c["slots"])


def branch_trace(name, dtype):
    """{row: {fact: value}}: the intermediates that prove which arm each on-branch row takes, from the statements of ray_tail_ref
    in `dtype`."""
    c, names = on_branch(name)
    r = ob_reference(c, dtype)
    B = lambda t: bool(t)
    out = {}
    if name in ("ob_identity", "ob_lambert_pad"):
        x, g = r["x"], r["d_acc"][:, :3]
        depth, var = c["depth"].to(dtype), c["var"].to(dtype)
        valid, td, ts = (c["ptab"][:, i].to(dtype) for i in (0, 1, 3))
        g1, std = (depth - td).abs() - ts, var.sqrt()
        applied = r["d_depth"] != (-2 * (c["desc"].lambda_hs / c["R"]) * (depth - depth * c["wsum"].to(dtype)))   # the depth term is there
        for i, nm in enumerate(names):
            f = {"applied": B(applied[i])}
            if nm.startswith("x_"):
                f["passes"] = tuple(B(v != 0) for v in g[i])
                f.update({"x_on_0_and_1": {"x0 == 0": B(x[i, 0] == 0), "x1 == 1": B(x[i, 1] == 1)},
                          "x_just_outside": {"x0 < 0": B(x[i, 0] < 0), "x1 > 1": B(x[i, 1] > 1)},
                          "x_just_inside": {"x0 > 0": B(x[i, 0] > 0), "x1 < 1": B(x[i, 1] < 1)}}[nm])
            else:
                want = EXPECTED_TRACE[nm]
                for fact in want:
                    if fact.startswith("|depth"):
                        f[fact] = B({"==": g1[i] == 0, "<": g1[i] < 0, ">": g1[i] > 0}[fact.split()[-2]])
                    elif fact.startswith("ts "):
                        f[fact] = B({"==": ts[i] == std[i], "<": ts[i] < std[i], ">": ts[i] > std[i]}[fact.split()[1]])
                    elif fact == "valid > 0":
                        f[fact] = B(valid[i] > 0)
            out[nm] = f
        return out
    n = c["acc"][:, 4:7].to(dtype)
    nn = (n * n).sum(-1)
    ns = r["normal_s"].norm(dim=-1)
    eps = torch.tensor(FP32_EPS, dtype=dtype)
    for i, nm in enumerate(names):
        f = {"clamped": B(nn[i] < eps)}
        if nm == "n_zero":
            f.update({"|n|^2 == 0": B(nn[i] == 0), "normal_s == 0": B((r["normal_s"][i] == 0).all())})
        elif nm == "n_below_eps":
            f.update({"|n|^2 < eps": B(nn[i] < eps), "|normal_s| < 1": B(ns[i] < 0.9)})
        else:
            f.update({"|n|^2 < eps": B(nn[i] < eps), "|normal_s| == 1": B(ns[i] == 1)})
        out[nm] = f
    return out


def on_branch_bound(name, row, quantity):
    """The bound of one quantity on one on-branch row: TOL unless the triple is in ILL."""
    c, _ = on_branch(name)
    return ILL[(name, row, quantity)][2] if (name, row, quantity) in ILL else TOL[(kind_of(c["desc"]), quantity)]


def compare_rows(c, names, got, ref, masks):
    """compare, one on-branch row at a time (the batch values loss and loss_acc as they are).  -> {(row, quantity): error}."""
    d, out = c["desc"], {}
    cpu = {k: v.detach().cpu() for k, v in got.items() if torch.is_tensor(v)}
    for i, nm in enumerate(names):
        sel = torch.zeros(len(names), dtype=torch.bool)
        sel[i] = True
        cut = {q: (m & sel.reshape([-1] + [1] * (m.dim() - 1))) if q not in ("loss", "loss_acc") else m for q, m in masks.items()}
        part = {k: v for k, v in cpu.items() if k not in ("loss", "loss_acc")}
        out.update({(nm, q): v for q, (v, _) in compare(part, ref, d, cut).items()})
    for q in ("loss", "loss_acc"):
        if q in cpu and bool(masks[q].all()):
            out[("*", q)] = compare({q: cpu[q]}, ref, d)[q][0]
    return out


def round_up(x):
    p = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / p - 1e-9) * p
