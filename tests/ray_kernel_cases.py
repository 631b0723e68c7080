"""Shared by tests/test_ray_kernels_cpu.py and tests/test_gpu_ray_kernels_f64.py: the fixed inputs of the lean step's per-ray
kernels (csrc/render_kernels.hip: composite_guided_kernel, merged_composite_kernel<MODE, C4>, normal_spv_reduce_kernel) and a
plain torch statement of what they compute, dtype-generic: every function here runs in float64 (the reference of the GPU
comparison) and in float32 (whose distance from float64 fixes the tolerances, see TOL).

The kernels give one wave a ray and one lane cpl = ceil(S / 64) consecutive samples, S <= 512.  The shapes below are the
smallest that reach the lane layouts of the S2 list: cpl 1, 2, 3 and 8, a ragged last lane (65, 129, 449), a single sample, both sources of the merged
row set down to one row, C = 4 on aligned and on 4-byte-misaligned blocks, and C up to BN_MAX_CH = 32.

How errors are scaled (err_* below), for the CPU measurement and the GPU comparison alike:
  per-sample arrays [R][S]     |err| / (|ref| + s), s = the array's largest magnitude in that ray
  per-ray values [R], [R][K]   |err| / (|ref| + s), s = the quantity's largest magnitude in that ray (a single value: itself).  acc
                               takes its density channel (sum_s w_s sigma_s, up to 1e5) apart from the others; var alone has a
                               floor, the ray's largest z^2 (where the weight sits on one sample it cancels to ~0)
  batch-wide values            spv_tot, spv_loss, loss_acc: every entry relative to itself
  gradient rows                |err| / (largest magnitude in the ray's gradient rows, both sources)
A zero error counts as 0 whatever the scale; a non-zero error on a zero scale is infinite.
"""
import torch

from oracle import render as ORD
from brdf_nerf_amd import losses

FAR = 0.5                 # depths lie in [0, FAR]: |z| + max |z| <= 1, so a z2 / z_all error bound of TOL is absolute
PAD, LAMBDA_RGB, LAMBDA_DS = 0.01, 0.7, 10.0
NOISE_STD = 0.4
LAM_AN, LAM_LR, LAM_SPV = 0.2, 0.1, 0.3
HS = 0.05

# Tolerances of the GPU comparison.  Each is 4 x the largest float32-vs-float64 error of the reference itself over every case
# below (the measurement stands beside it), rounded up to one significant digit; test_ray_kernels_cpu.py asserts that the float32
# reference stays within HALF of each.  The other half is for what the kernels do differently from torch: per-lane serial product
# + 6-step wave scan against torch.cumprod, the device's expf, 64-lane butterfly sums against torch's pairwise sums.
TOL = {
    "alphas": 7e-5,       # measured 1.66e-05 (S449_allbut1448_C32_R11, noise on the empty ray: every alpha <= 2e-3 there, and
                          #                    1 - exp(-x) carries an absolute 6e-8 in float32)
    "trans": 3e-6,        # measured 6.52e-07
    "weights": 7e-5,      # measured 1.60e-05 (the same ray)
    # the per-ray sums of those weights inherit their relative error on rays whose weight is small (each ray has its own scale):
    "depth": 4e-5,        # measured 9.57e-06 (S2_identity2_C4a_R13)
    "wsum": 4e-5,         # measured 9.56e-06 (the same ray)
    "var": 2e-6,          # measured 4.06e-07
    "acc": 7e-5,          # measured 1.50e-05 (S512_none512_C13_R9)
    "reg": 6e-5,          # measured 1.26e-05 (S192_identity192_C20_R13)
    "spv_ray": 3e-5,      # measured 7.36e-06 (S512_one1_C13_R11 under noise: its first entry is wsum)
    "spv_tot": 6e-7,      # measured 1.41e-07
    "spv_loss": 5e-7,     # measured 1.10e-07
    "rgb": 4e-5,          # measured 9.52e-06 (S2_identity2_C4a_R13)
    "ray_loss": 7e-6,     # measured 1.69e-06
    "loss_acc": 7e-6,     # measured 1.69e-06 (slot r % 16 holds ray r's term: R <= 13)
    "grad_tail": 9e-4,    # measured 2.15e-04 (S449_allbut1448_C32_R11 under noise)
    "grad_bwd": 3e-5,     # measured 7.15e-06 (S65_allbut164_C20_R10; every entry of TERMS but the hard-surface term alone)
    "grad_hs": 3e-3,      # measured 5.61e-04 (S2_identity2_C4a_R13: the hard-surface term alone, (z - depth)^2 of a ray whose
                          #                    weight sits on one sample, scaled by a gradient that is itself ~0)
    "z2": 3e-5,           # measured 6.86e-06 (S449_G63_noprior_R13 under noise)
    "z_all": 7e-6,        # measured 1.53e-06
}
# Gradient entries left out of the comparison: none (share 0 in every case, so the 1 % cap and the no-whole-ray rule hold
# trivially).  Instead two density patterns were softened until every ray's gradient is well-conditioned in the float64
# reference itself: see _sigma_pattern.
EXCLUDED_SHARE = 0.0

PATTERNS = ("zero", "opaque_first", "opaque_last", "negative", "spikes", "moderate")


# ------------------------------------------------------------------------------------------------ the reference
def composite_ref(z, sigma, noise=None, noise_std=0.0, rows=None):
    """oracle/render.py:composite restated (same statements, same order: bitwise equal in float32), + wsum, var and - with the
    samples' rows [R][S][C] - acc = sum_s w_s row_s."""
    deltas = torch.cat([z[:, 1:] - z[:, :-1], 1e10 * torch.ones_like(z[:, :1])], -1)
    s = sigma if noise is None else sigma + noise * noise_std
    alphas = 1 - torch.exp(-deltas * torch.relu(s))
    shifted = torch.cat([torch.ones_like(alphas[:, :1]), 1 - alphas + 1e-10], -1)
    T = torch.cumprod(shifted, -1)[:, :-1]
    w = alphas * T
    depth = (w * z).sum(-1)
    o = {"alphas": alphas, "trans": T, "weights": w, "depth": depth, "wsum": w.sum(-1),
         "var": (w * (z - depth.unsqueeze(-1)) ** 2).sum(-1)}
    if rows is not None:
        o["acc"] = (w.unsqueeze(-1) * rows).sum(-2)
    return o


def merged_rows(idx, out1, out2):
    """Sample s of ray r is row idx[r][s] of cat[out1[r], out2[r]] (idx None: out1 as it is)."""
    if idx is None:
        return out1
    cat = out1 if out2 is None else torch.cat([out1, out2], 1)
    return cat.gather(1, idx.unsqueeze(-1).expand(-1, -1, cat.shape[-1]))


def _leaves(out1, out2):
    a = out1.detach().clone().requires_grad_(True)
    b = None if out2 is None else out2.detach().clone().requires_grad_(True)
    return a, b


def _grads(total, a, b):
    if not total.requires_grad:
        return torch.zeros_like(a), (None if b is None else torch.zeros_like(b))
    g = torch.autograd.grad(total, [a] if b is None else [a, b], allow_unused=True)
    z0 = lambda gi, t: torch.zeros_like(t) if gi is None else gi
    return z0(g[0], a), (None if b is None else z0(g[1], b))


def forward_ref(z, idx, out1, out2, nreg=None, noise=None, noise_std=0.0):
    """bn_merged_composite_forward + bn_normal_spv_reduce: the compositing outputs, the rays' NormalRegLoss terms (`reg`), the
    rays' NormalLoss sums (`spv_ray`) and the batch-wide terms the reduce derives from them (`spv_tot`, `spv_loss`)."""
    rows = merged_rows(idx, out1, out2)
    o = composite_ref(z, rows[..., 3], noise, noise_std, rows)
    w = o["weights"]
    if nreg is not None:
        view = nreg["view"].to(z.dtype)
        reg = torch.zeros_like(o["depth"])
        for ch, lam in ((nreg.get("ch_an", -1), nreg.get("lam_an", 0.0)), (nreg.get("ch_lr", -1), nreg.get("lam_lr", 0.0))):
            if ch >= 0 and lam > 0:
                ndv = (rows[..., ch:ch + 3] * view[:, None, :]).sum(-1)
                reg = reg + lam * (w * torch.clamp_max(ndv, 0.0) ** 2).sum(-1)
        o["reg"] = reg
        if nreg.get("lam_spv", 0.0):
            ca, cl, lam = nreg["spv_an"], nreg["spv_lr"], nreg["lam_spv"]
            dn = (rows[..., ca:ca + 3] - rows[..., cl:cl + 3]).abs()
            o["spv_ray"] = torch.stack([w.sum(-1), dn.sum((-1, -2))], -1)
            o["spv_tot"] = spv_tot_ref(o["spv_ray"], z.shape[0], z.shape[1], lam)
            o["spv_loss"] = losses.normal_loss(w, rows[..., ca:ca + 3], rows[..., cl:cl + 3], lam)
    return o


def spv_tot_ref(spv_ray, R, S, lam):
    """bn_normal_spv_reduce: (d loss / d w_s, d loss / d n per unit sign, loss term) from the rays' sums."""
    n = float(R) * float(S)
    mean_w, mean_d = spv_ray[:, 0].sum() / n, spv_ray[:, 1].sum() / (3.0 * n)
    return torch.stack([lam * mean_d / n, lam * mean_w / (3.0 * n), lam * mean_w * mean_d])


def tail_ref(z, idx, out1, out2, rgbs, pad, lambda_rgb, prior=None, lambda_ds=0.0, usealldepth=False, noise=None, noise_std=0.0):
    """bn_lambert_tail: x = acc[:3] (1 + 2 pad) - pad wsum, clamp to [0, 1], losses.snerf_loss + losses.depth_loss, and the
    gradient rows of their sum in the source layouts by autograd.  prior = (valid, target_depth, target_weight, target_std)."""
    a, b = _leaves(out1, out2)
    rows = merged_rows(idx, a, b)
    o = composite_ref(z, rows[..., 3], noise, noise_std, rows)
    R = z.shape[0]
    x = o["acc"][:, :3] * (1 + 2 * pad) - pad * o["wsum"].unsqueeze(-1)
    rgb = x.clamp(0.0, 1.0)
    total = losses.snerf_loss(rgb, rgbs, lambda_rgb)
    ray_loss = lambda_rgb * ((rgb - rgbs) ** 2).sum(-1) / (3.0 * R)
    if prior is not None and lambda_ds > 0:
        valid, td, tw, ts = prior
        total = total + losses.depth_loss(z, o["depth"], o["weights"], td, tw, valid, ts, lambda_ds, usealldepth)
        apply = valid > 0
        if not usealldepth:
            apply = apply & ((((o["depth"] - td).abs() - ts) > 0) | (ts < o["var"].sqrt()))
        ray_loss = ray_loss + torch.where(apply, (lambda_ds / 3.0 / R) * tw * (o["depth"] - td) ** 2, torch.zeros_like(td))
    d1, d2 = _grads(total, a, b)
    loss_acc = torch.zeros(16, dtype=z.dtype).index_add_(0, torch.arange(R) % 16, ray_loss.detach())
    return {"rgb": rgb.detach(), "weights": o["weights"].detach(), "depth": o["depth"].detach(), "ray_loss": ray_loss.detach(),
            "loss_acc": loss_acc, "total": total.detach(), "grad_tail": (d1, d2)}


def backward_ref(z, idx, out1, out2, d_w=None, d_depth=None, d_acc=None, d_wsum=None, hs_scale=0.0, nreg=None, noise=None,
                 noise_std=0.0):
    """bn_merged_composite_backward: autograd of ONE scalar made of the terms that are given - sum(w d_w) + sum(depth d_depth)
    + sum(acc d_acc) (d_acc[:, 3] = 0) + sum(wsum d_wsum) + hs_scale sum_s w_s (z_s - depth)^2 with that depth detached (the
    kernel takes it as an input) + losses.normal_reg_loss on one or both normal fields + losses.normal_loss 'an_lr'."""
    a, b = _leaves(out1, out2)
    rows = merged_rows(idx, a, b)
    o = composite_ref(z, rows[..., 3], noise, noise_std, rows)
    w = o["weights"]
    total = torch.zeros((), dtype=z.dtype)
    if d_w is not None:
        total = total + (w * d_w).sum()
    if d_depth is not None:
        total = total + (o["depth"] * d_depth).sum()
    if d_acc is not None:
        da = d_acc.clone()
        da[:, 3] = 0
        total = total + (o["acc"] * da).sum()
    if d_wsum is not None:
        total = total + (o["wsum"] * d_wsum).sum()
    if hs_scale:
        total = total + hs_scale * (w * (z - o["depth"].detach().unsqueeze(-1)) ** 2).sum()
    if nreg is not None:
        view = nreg["view"].to(z.dtype)
        for ch, lam in ((nreg.get("ch_an", -1), nreg.get("lam_an", 0.0)), (nreg.get("ch_lr", -1), nreg.get("lam_lr", 0.0))):
            if ch >= 0 and lam > 0:
                total = total + losses.normal_reg_loss(rows[..., ch:ch + 3], w, view, lam)[0]
        if nreg.get("lam_spv", 0.0):
            ca, cl = nreg["spv_an"], nreg["spv_lr"]
            total = total + losses.normal_loss(w, rows[..., ca:ca + 3], rows[..., cl:cl + 3], nreg["lam_spv"])
    return _grads(total, a, b)


def guided_ref(z, sigma, G, near0, far0, d_range, u, use_target=None, target_depth=None, target_std=None, u_target=None,
               noise=None, noise_std=0.0):
    """bn_composite_guided: pass-1 compositing, oracle.render.guided_samples on the given uniforms (u, u_target: one row per
    ray), stable sort and merge."""
    o = composite_ref(z, sigma, noise, noise_std)
    w1, d1 = o["weights"], o["depth"]
    train = use_target is not None
    replay = [u] + ([u_target[use_target > 0]] if train else [])
    z2, _, _ = ORD.guided_samples(d1, w1, z, G, torch.as_tensor(near0, dtype=z.dtype), torch.as_tensor(far0, dtype=z.dtype),
                                  ORD.Randoms(replay=replay), d_range, "train" if train else "test",
                                  use_target if train else None, target_depth.unsqueeze(-1) if train else None,
                                  target_std if train else None)
    z2 = torch.sort(z2, -1)[0]
    z_all, idx = torch.sort(torch.cat([z, z2], -1), dim=-1, stable=True)
    return {"weights": w1, "depth": d1, "z2": z2, "z_all": z_all, "idx": idx}


# ------------------------------------------------------------------------------------------------ error scaling
def _ratio(err, den):
    r = torch.where(err == 0, torch.zeros_like(err), err / den)       # NaN stays NaN: a comparison with it fails
    return float(r.max()) if r.numel() else 0.0


def err_samples(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double()
    return _ratio((got - ref).abs(), ref.abs() + ref.abs().amax(-1, keepdim=True))


def err_rays(got, ref, floor=None):
    """ref [R] or [R][K] (or one batch-wide number / vector, each entry then its own scale): |err| / (|ref| + s), s = the largest
    magnitude of the quantity in that ray, and at least `floor` [R] where one is given."""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    s = ref.abs().amax(-1, keepdim=True).expand_as(ref) if ref.dim() == 2 else ref.abs()
    if floor is not None:
        s = torch.maximum(s, floor.double().reshape([-1] + [1] * (ref.dim() - 1)).expand_as(ref))
    return _ratio((got - ref).abs(), ref.abs() + s)


def err_grads(got, ref):
    """got, ref: (d_out1 [R][S1][C], d_out2 [R][Sg][C] or None)."""
    R = ref[0].shape[0]
    flat = lambda p: torch.cat([t.detach().double().cpu().reshape(R, -1) for t in p if t is not None], -1)
    g, r = flat(got), flat(ref)
    assert g.shape == r.shape
    return _ratio((g - r).abs(), r.abs().amax(-1, keepdim=True).expand_as(r))


def compare(got, ref, case):
    """-> {quantity: scaled error} for every entry of `ref` (forward_ref / tail_ref style dicts; `got` must hold them all)."""
    missing = set(ref) - set(got) - {"total", "idx"}
    assert not missing, f"not computed: {sorted(missing)}"
    e = {}
    for k, r in ref.items():
        if k in ("total", "idx"):
            continue
        if k in ("alphas", "trans", "weights", "z2", "z_all"):
            e[k] = err_samples(got[k], r)
        elif k in ("grad_tail", "grad_bwd", "grad_hs"):
            e[k] = err_grads(got[k], r)
        elif k == "spv_ray":
            e[k] = max(err_rays(got[k][:, i], r[:, i]) for i in range(2))
        elif k == "acc":
            # the density channel (sum_s w_s sigma_s, up to 1e5 behind an opaque sample) on its own, the others by their own largest
            oth = [c for c in range(r.shape[-1]) if c != 3]
            e[k] = max(err_rays(got[k][:, oth], r[:, oth]), err_rays(got[k][:, 3], r[:, 3]))
        elif k == "var":
            # (z_s - depth)^2 carries the absolute rounding of z^2: where the weight sits on one sample var cancels to ~0
            e[k] = err_rays(got[k], r, case["z_all"].abs().amax(-1) ** 2)
        elif k in ("spv_tot", "loss_acc"):
            e[k] = err_rays(got[k].reshape(-1), r.reshape(-1))
        else:
            e[k] = err_rays(got[k].reshape(r.shape), r)
    return e


# ------------------------------------------------------------------------------------------------ inputs
def _sigma_pattern(name, z, g):
    """One ray's densities on its sorted depths z [S]."""
    S = z.shape[0]
    delta = torch.cat([z[1:] - z[:-1], torch.full((1,), 1e10)])
    # optical depth ~ 2 over the ray and an EMPTY last sample (S >= 2): with a dense last sample (delta = 1e10) wsum is 1 to
    # within 1e-10 whatever the densities, and the gradient of a d_wsum term alone is a difference of equal terms in every ray
    # (ill-conditioned in the float64 reference itself, beyond what per-entry exclusions may cover).  The dense last sample is
    # covered by "opaque_last", by S = 1 and by the noise runs, where the last sample's density takes either sign.
    moderate = (0.5 + 7.0 * torch.rand(S, generator=g)) * (torch.arange(S) < max(S - 1, 1))
    if name == "zero":
        return torch.zeros(S)
    if name == "opaque_first":
        s = moderate.clone()
        # optical depth 3 (alpha 0.95; S = 1: the 1e10 step, alpha 1).  Softened from 30: float32 knows u = 1 - alpha + 1e-10 to
        # 6e-8 / u only, so everything behind a sample with u ~ 1e-10 carries a relative error of ~1e-3 in ANY float32 evaluation,
        # and with the colours clamped those entries are the ray's largest - a whole ray would have had to be excluded.
        s[0] = 3.0 / float(delta[0]) if S > 1 and float(delta[0]) > 0 else 1.0
        return s
    if name == "opaque_last":
        s = torch.zeros(S)
        s[-1] = 1.0
        return s
    if name == "negative":
        neg = torch.rand(S, generator=g) < 0.7
        return torch.where(neg, -0.1 - 5.0 * torch.rand(S, generator=g), moderate)
    if name == "spikes":                                             # _field_like of test_gpu_lean.py, on a ray a quarter as long
        r = torch.rand(S, generator=g)
        return torch.where(r < 0.5, torch.zeros(S), 160.0 * (r - 0.5) ** 2) * (torch.arange(S) < max(S - 1, 1))
    return moderate


def _split(S2, split):
    return {"none": S2, "identity": S2, "one": 1, "allbut1": S2 - 1, "even": S2 // 2}[split]


def _normal_channels(C):
    """(ch_an, ch_lr) of the two normal fields, or None where the row is too short for both."""
    return None if C < 10 else (4, C - 3 if C > 13 else 7)


def build_case(S2, split, cvar, R, seed, first_pattern=0):
    g = torch.Generator().manual_seed(seed)
    C = 4 if cvar in ("4a", "4m") else int(cvar)
    S1 = _split(S2, split)
    Sg = S2 - S1
    z1 = torch.sort(torch.rand(R, S1, generator=g) * FAR, -1)[0]
    if S1 >= 4:
        z1[:, S1 // 2] = z1[:, S1 // 2 - 1]                          # equal neighbours inside one source
    if Sg:
        zg = torch.sort(torch.rand(R, Sg, generator=g) * FAR, -1)[0]
        if Sg >= 2 and S1 >= 3:
            zg[:, Sg // 2] = z1[:, 2 * S1 // 3]                       # and across the two (stable order: out1's row first)
            zg = torch.sort(zg, -1)[0]
        z_all, idx = torch.sort(torch.cat([z1, zg], -1), dim=-1, stable=True)
    else:
        z_all, idx = z1, (torch.arange(S2).expand(R, -1).contiguous() if split == "identity" else None)
    pats = [PATTERNS[(first_pattern + r) % len(PATTERNS)] for r in range(R)]
    rows = torch.rand(R, S2, C, generator=g)
    # colour sums below 0, inside [0, 1] and above 1, by density pattern, so that each sign falls on rays that carry weight
    pidx = torch.tensor([PATTERNS.index(p) for p in pats])
    rows[..., :3] *= torch.tensor([1.0, 4.0, 1.0, 1.0, 4.0, -1.0])[pidx].view(R, 1, 1)
    for r in range(R):
        rows[r, :, 3] = _sigma_pattern(pats[r], z_all[r], g)
    if C > 4:
        rows[..., 4:] = torch.randn(R, S2, C - 4, generator=g)
    nch = _normal_channels(C)
    if nch is not None and S2 >= 2:
        rows[:, ::5, nch[1]:nch[1] + 3] = rows[:, ::5, nch[0]:nch[0] + 3]          # equal normals: the sign term is 0 there
    if idx is None:
        out1, out2 = rows.contiguous(), None
    else:
        cat = torch.zeros(R, S2, C).scatter_(1, idx.unsqueeze(-1).expand(-1, -1, C), rows)
        out1, out2 = cat[:, :S1].contiguous(), (cat[:, S1:].contiguous() if Sg else None)
    rays_d = torch.nn.functional.normalize(torch.tensor([0.15, 0.2, -0.96]) + 0.2 * torch.randn(R, 3, generator=g), dim=-1)
    case = dict(S2=S2, S1=S1, C=C, cvar=cvar, R=R, split=split, seed=seed, patterns=pats, z_all=z_all.contiguous(), idx=idx,
                out1=out1, out2=out2, rays_d=rays_d, normals=nch,
                rgbs=torch.rand(R, 3, generator=g), noise=torch.randn(R, S2, generator=g),
                d_w=torch.randn(R, S2, generator=g), d_depth=torch.randn(R, generator=g), d_acc=torch.randn(R, C, generator=g),
                d_wsum=torch.randn(R, generator=g))
    # depth priors placed from the float64 compositing of these inputs, far from each clause's threshold:
    # by density pattern -> 0 (zero): no valid prior; 1, 4 (opaque_first, moderate): |d - td| - ts > 0 only; 2 (negative, spikes):
    # ts < std only (where the ray has a spread); 3 (opaque_last): neither clause
    o = composite_ref(z_all.double(), merged_rows(idx, out1, out2)[..., 3].double())
    d, std = o["depth"], o["var"].sqrt()
    k = torch.tensor([0, 1, 3, 2, 2, 4])[pidx]
    wide = 2.0 * std + 0.05
    ts = torch.where((k == 2) & (std > 1e-3), 0.5 * std, wide)
    td = torch.where((k == 1) | (k == 4), d + 2.0 * ts, d + 0.25 * ts)
    case["valid"] = (k != 0).float()
    case["depths"] = torch.stack([td.float(), 0.5 + torch.rand(R, generator=g)], -1).contiguous()     # [R][2]: target depth, weight
    case["tstd"] = ts.float()
    return case


def nreg_of(case, an=True, lr=True, spv=False):
    """The regulariser description of a case (None where its rows hold no normal fields)."""
    if case["normals"] is None:
        return None
    ca, cl = case["normals"]
    return dict(view=-case["rays_d"], ch_an=ca if an else -1, ch_lr=cl if lr else -1, lam_an=LAM_AN if an else 0.0,
                lam_lr=LAM_LR if lr else 0.0, lam_spv=LAM_SPV if spv else 0.0, spv_an=ca, spv_lr=cl)


def prior_of(case, dtype):
    return (case["valid"].to(dtype), case["depths"][:, 0].to(dtype), case["depths"][:, 1].to(dtype), case["tstd"].to(dtype))


def inputs(case, dtype):
    cv = lambda t: None if t is None else t.to(dtype)
    return cv(case["z_all"]), case["idx"], cv(case["out1"]), cv(case["out2"])


# name -> which of the backward's terms are on
TERMS = {
    "d_w": dict(d_w=True), "d_depth": dict(d_depth=True), "d_acc": dict(d_acc=True), "d_wsum": dict(d_wsum=True),
    "hs": dict(hs=True), "nreg_an": dict(an=True), "nreg_lr": dict(lr=True), "nreg_both": dict(an=True, lr=True),
    "spv": dict(spv=True), "nreg_both_spv": dict(an=True, lr=True, spv=True),
    "all": dict(d_w=True, d_depth=True, d_acc=True, d_wsum=True, hs=True, an=True, lr=True, spv=True),
}


def grad_key(term):
    """The hard-surface term alone is held to a bound of its own (TOL["grad_hs"]); every other entry of TERMS to TOL["grad_bwd"]."""
    return "grad_hs" if term == "hs" else "grad_bwd"


def backward_args(case, term, dtype):
    """Keyword arguments of backward_ref for one entry of TERMS (None where the case has no normal fields for it)."""
    t = TERMS[term]
    wants_n = t.get("an") or t.get("lr") or t.get("spv")
    if wants_n and case["normals"] is None and term != "all":
        return None
    cv = lambda k: case[k].to(dtype) if t.get(k) else None
    nreg = nreg_of(case, bool(t.get("an")), bool(t.get("lr")), bool(t.get("spv"))) if wants_n else None
    return dict(d_w=cv("d_w"), d_depth=cv("d_depth"), d_acc=cv("d_acc"), d_wsum=cv("d_wsum"), hs_scale=HS if t.get("hs") else 0.0,
                nreg=nreg)


TAIL_CONFIGS = {"noprior": dict(prior=False), "prior": dict(prior=True, usealldepth=False), "alldepth": dict(prior=True, usealldepth=True)}


def reference_all(case, dtype):
    """Every compared quantity of a merged-set case, evaluated in `dtype`: {"fwd": ..., "fwd_noise": ..., "tail/<config>": ...,
    "bwd/<term>": {"grad_bwd": (d_out1, d_out2)}}."""
    z, idx, o1, o2 = inputs(case, dtype)
    res = {"fwd": forward_ref(z, idx, o1, o2, nreg_of(case, spv=True)),
           "fwd_noise": forward_ref(z, idx, o1, o2, nreg_of(case, spv=True), case["noise"].to(dtype), NOISE_STD)}
    for name, cfg in TAIL_CONFIGS.items():
        res["tail/" + name] = tail_ref(z, idx, o1, o2, case["rgbs"].to(dtype), PAD, LAMBDA_RGB,
                                       prior_of(case, dtype) if cfg["prior"] else None, LAMBDA_DS if cfg["prior"] else 0.0,
                                       cfg.get("usealldepth", False))
    res["tail/noise"] = tail_ref(z, idx, o1, o2, case["rgbs"].to(dtype), PAD, LAMBDA_RGB, prior_of(case, dtype), LAMBDA_DS, True,
                                 case["noise"].to(dtype), NOISE_STD)
    for term in TERMS:
        kw = backward_args(case, term, dtype)
        if kw is not None:
            res["bwd/" + term] = {grad_key(term): backward_ref(z, idx, o1, o2, **kw)}
    kw = backward_args(case, "all", dtype)
    res["bwd/all_noise"] = {"grad_bwd": backward_ref(z, idx, o1, o2, noise=case["noise"].to(dtype), noise_std=NOISE_STD, **kw)}
    return res


S2_LIST = (1, 2, 63, 64, 65, 128, 129, 192, 449, 512)
SPLITS = ("none", "identity", "one", "allbut1", "even")
CVARS = ("4a", "4m", "5", "13", "20", "32")
_RAYS = (6, 7, 9, 10, 11, 13)


def _table():
    """Every S2 with every split, and every S2 with every C variant (the other axis rotating), without repeats; R rotates over
    _RAYS (each >= 6: every density pattern on a ray of its own), and each S2 has one single-ray case."""
    keys = []
    for i, S2 in enumerate(S2_LIST):
        for j, sp in enumerate(SPLITS):
            keys.append((S2, sp, CVARS[(i + j) % len(CVARS)]))
        for k, cv in enumerate(CVARS):
            keys.append((S2, SPLITS[(i + k) % len(SPLITS)], cv))
    cases, seen = {}, set()
    for S2, sp, cv in keys:
        S1 = _split(S2, sp)
        if S1 < 1 or (sp in ("one", "allbut1", "even") and S1 == S2):
            sp, S1 = "none", S2
        if (S2, S1, sp in ("none",), cv) in seen:
            continue
        seen.add((S2, S1, sp in ("none",), cv))
        n = len(cases)
        cases[f"S{S2}_{sp}{S1}_C{cv}_R{_RAYS[n % 6]}"] = build_case(S2, sp, cv, _RAYS[n % 6], 1000 + n, first_pattern=n)
    for i, S2 in enumerate(S2_LIST):                                  # R = 1: one pattern each, the opaque and the moderate ones first
        pat = (1, 5, 2, 4, 3, 0)[i % 6]
        sp = "none" if S2 < 3 else SPLITS[2 + i % 3]
        cv = ("4a", "13", "4m", "32")[i % 4]
        cases[f"S{S2}_{sp}{_split(S2, sp)}_C{cv}_R1"] = build_case(S2, sp, cv, 1, 3000 + i, first_pattern=pat)
    return cases


CASES = _table()
# the C = 4 pairs that differ only in the alignment of their blocks: same seed, same numbers expected bitwise
ALIGN_PAIRS = {S2: build_case(S2, "even" if S2 > 1 else "none", "4a", 7, 4000 + S2, first_pattern=S2) for S2 in (1, 65, 449)}

REDUCE_R = (1, 1023, 1025, 3000)


def reduce_case(R):
    """spv_ray [R][2] for the reduce alone, S2 = 2: sums of weights in [0, 1], sums of |n_an - n_lr| over 2 samples x 3 channels."""
    g = torch.Generator().manual_seed(5000 + R)
    return torch.stack([torch.rand(R, generator=g), 6.0 * torch.rand(R, generator=g)], -1).contiguous()


# bn_composite_guided: (S, G) -> n2g 64 / 128 / 256 and merge sizes up to BN_MAX_SG = 512
GUIDED_SG = ((1, 3), (63, 3), (65, 64), (128, 65), (256, 256), (449, 63), (509, 3))


def build_guided(S, G, prior, R, seed, first_pattern=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.sort(torch.rand(R, S, generator=g) * FAR, -1)[0]
    if S >= 4:
        z[:, S // 2] = z[:, S // 2 - 1]
    pats = [PATTERNS[(first_pattern + r) % len(PATTERNS)] for r in range(R)]
    sigma = torch.stack([_sigma_pattern(pats[r], z[r], g) for r in range(R)])
    case = dict(S=S, G=G, R=R, prior=prior, patterns=pats, z=z.contiguous(), sigma=sigma.contiguous(), z_all=z,
                u=torch.rand(R, G, generator=g), u_t=torch.rand(R, G, generator=g), noise=torch.randn(R, S, generator=g),
                out1=sigma, out2=None)
    if prior:
        case["valid"] = (torch.arange(R) % 3 != 1).float()
        # [R][2] tables: the kernel takes depths[:, 0] and the valid flags as strided views
        case["depths"] = torch.stack([0.1 + 0.3 * torch.rand(R, generator=g), torch.rand(R, generator=g)], -1).contiguous()
        case["tstd"] = torch.stack([0.005 + 0.02 * torch.rand(R, generator=g), torch.rand(R, generator=g)], -1).contiguous()
    return case


def guided_reference(case, dtype, u=None, u_t=None, noise=None):
    cv = lambda t: t.to(dtype)
    kw = {}
    if case["prior"]:
        kw = dict(use_target=cv(case["valid"]), target_depth=cv(case["depths"][:, 0]), target_std=cv(case["tstd"][:, 0]),
                  u_target=cv(case["u_t"] if u_t is None else u_t))
    return guided_ref(cv(case["z"]), cv(case["sigma"]), case["G"], 0.0, FAR, 3.0, cv(case["u"] if u is None else u),
                      noise=None if noise is None else cv(noise), noise_std=NOISE_STD if noise is not None else 0.0, **kw)


GUIDED_CASES = {f"S{S}_G{G}_{'prior' if p else 'noprior'}_R{_RAYS[(i + p) % 6]}":
                build_guided(S, G, bool(p), _RAYS[(i + p) % 6], 6000 + 2 * i + p, first_pattern=i + p)
                for i, (S, G) in enumerate(GUIDED_SG) for p in (0, 1)}
GUIDED_CASES["S65_G64_prior_R1"] = build_guided(65, 64, True, 1, 6100, first_pattern=5)


def idx_mismatches(idx, ref, gap):
    """Sort indices that differ from the reference's where no reference neighbour is closer than `gap` (near-tie rule of
    test_random_composite_and_guided_shapes_against_oracle), and the share of entries that rule skips."""
    z_all_ref, idx_ref = ref["z_all"].double(), ref["idx"]
    near = (z_all_ref[:, 1:] - z_all_ref[:, :-1]).abs() <= gap
    loose = torch.zeros_like(z_all_ref, dtype=torch.bool)
    loose[:, 1:] |= near
    loose[:, :-1] |= near
    return int(((idx.cpu() != idx_ref) & ~loose).sum()), float(loose.double().mean())
