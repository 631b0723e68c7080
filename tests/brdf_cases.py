"""Shared by tests/test_brdf_cpu.py and tests/test_gpu_brdf_f64.py: the fixed inputs of the closed-form BRDF code
(csrc/brdf_eval.h: rpv_eval, hapke_eval, microfacet_eval over float and Dual<N>, as instantiated in brdf.hip and in
sample_brdf.hip) and its float64 reference, oracle/brdf.py evaluated in float64 on the float32 inputs cast exactly, Jacobians by
autograd with d_brdf = e_0, e_1, e_2 (the full 3 x slots Jacobian of every row) and one random d_brdf.  The same evaluation in
float32 fixes the tolerances (TOL).

Two tables per family:
  well-posed  N_ROWS rows drawn from seeds and kept only where a margin predicate (margins, M = 0.02) holds in float64: every
              clamp, the i <= e arms and every NaN replacement are at least M away, so float32 and float64 take the same arms
  on-branch   rows that sit EXACTLY on a branch, built from dyadic / axis-aligned vectors so that the deciding dot products are
              exact in both precisions (ON_BRANCH_ROWS; branch_trace names the intermediates that prove the arm).  Held to TOL
              but for the (row, quantity) pairs of ILL; where a factor is NaN-replaced: REPLACED_ZERO, SUBSTITUTED

How errors are scaled (err_values / err_aux / err_jac / err_rnd), for the CPU measurement and the GPU comparison alike:
  values brdf [N][3]           |err| / (|ref| + s), s = the row's largest |brdf|
  aux quantities [N][w]        |err| / (|ref| + s), s = the row's largest magnitude of that quantity (a scalar: itself)
  Jacobian entries             |err| / (|ref| + B), B = the largest magnitude in that input group's 3 x width block of the row
  the random-d_brdf row        |err| / (|ref| + B sum_c |d_brdf_c|): a combination of the block's rows with those coefficients
A zero error counts as 0 whatever the scale; a non-zero error on a zero scale is infinite.  Entries whose reference is exactly 0
(cross-channel entries, inputs that do not reach the value, clamped or replaced factors) must be exactly 0 (structural_zero_errors).
"""
import math
from unittest import mock

import torch

from oracle import brdf as OB

M = 0.02
N_ROWS = 512
F32MAX = float(torch.finfo(torch.float32).max)
F0 = 0.04

# Tolerances of the GPU comparison, per (family, quantity).  Each is 4 x the largest float32-oracle-against-float64-oracle error
# over the well-posed table, every variant of the family (the measurement, its variant and row stand beside it), rounded up to one
# significant digit; test_brdf_cpu.py asserts that the float32 oracle stays within HALF of each.  The other half is for what the
# kernels do differently: the device's powf, tanf, acosf, expf and logf, and forward-mode against reverse-mode order.
TOL = {
    ("rpv", "brdf"): 3e-6,             # measured 5.77e-07 (rpv/k, row 343)
    ("rpv", "aux"): 4e-6,              # measured 8.36e-07 (rpv/none, row 343: ci of a grazing sun)
    ("rpv", "d_n"): 6e-6,              # measured 1.49e-06 (rpv/k, row 343)
    ("rpv", "d_w"): 3e-6,              # measured 5.69e-07 (rpv/k, row 343)
    ("rpv", "d_k"): 2e-4,              # measured 4.18e-05 (rpv/kt, row 436: log(base) with base within 2e-3 of 1)
    ("rpv", "d_theta"): 9e-6,          # measured 2.16e-06 (rpv/tr, row 435)
    ("rpv", "d_rhoc"): 4e-6,           # measured 8.22e-07 (rpv/tr, row 343)
    ("hapke", "brdf"): 6e-6,           # measured 1.45e-06 (hapke/bc/1.3, row 169)
    ("hapke", "aux"): 5e-6,            # measured 1.10e-06 (hapke/bt/4.0, row 169)
    ("hapke", "d_n"): 8e-5,            # measured 1.99e-05 (hapke/b/1.3, row 169)
    ("hapke", "d_w"): 6e-6,            # measured 1.37e-06 (hapke/bc/1.3, row 169)
    ("hapke", "d_b"): 3e-4,            # measured 5.29e-05 (hapke/bct/4.0, row 156)
    ("hapke", "d_c"): 3e-4,            # measured 5.52e-05 (hapke/bc/1.3, row 403)
    ("hapke", "d_theta"): 6e-5,        # measured 1.38e-05 (hapke/s3t/4.0, row 280)
    ("microfacet", "brdf"): 3e-6,      # measured 6.83e-07 (row 490)
    ("microfacet", "aux"): 5e-5,       # measured 1.08e-05 (row 225: d, the GGX lobe at alpha = 0.003)
    ("microfacet", "d_n"): 7e-5,       # measured 1.62e-05 (row 225)
    ("microfacet", "d_albedo"): 0.0,   # measured 0: brdf = albedo + glossy, the block is the identity in every precision
    ("microfacet", "d_rough"): 2e-3,   # measured 4.03e-04 (row 105)
}
# Entries left out of the comparison on the well-posed table: none.  The margin predicate and the parameter ranges keep every
# group's Jacobian block well-conditioned in the float64 reference itself.
EXCLUDED_SHARE = 0.0
# On-branch (family, row, quantity) triples where the float32 ORACLE ITSELF misses TOL / 2 against the float64 oracle, each with
# the measurement (the worst variant beside it) and the derived bound it is held to instead.  Everything else on every on-branch
# row is held to TOL.  test_brdf_cpu.py asserts that each listed triple does exceed TOL / 2 (the list cannot grow by default),
# that no unlisted one does, and that the float32 oracle keeps half of each bound.  Three mechanisms, three bounds:
#   ACOS_TOL = 2e-2   ci (or cv) = 1e-5: sza = acos(ci) lies 1e-5 below pi / 2 where float32 numbers are 1.19e-7 apart, so
#                     cos(sza) and 1 / tan(sza) come back with up to 1.19e-7 / 1e-5 = 1.2e-2 of themselves.  RPV reads tan(sza)
#                     only in G (aux G and d_rhoc = -w M1 F / (1 + G); H = 1 + O(1 / G) does not notice); Hapke divides every value by cos(sza), and S carries cos(sza) / eta_i.  The same bound
#                     holds G on l_eq_v: cp = (1 - c^2) / (si sv) is 1 to within two float32 spacings (2.4e-7), and
#                     G^2 = 2 tan^2 (1 - cp) + 1e-5 with tan^2 = 0.78 moves by up to 3.7e-2 of itself, G by 1.9e-2, which on
#                     the scale |ref| + s = 2 G is 0.93e-2.
#   G_TOL = 4e-5      l_eq_v, what reads G through H = 1 + (1 - rhoc) / (1 + G + 1e-5): G = 3.2e-3 moves by up to 1.9e-2 of
#                     itself, 5.8e-5 absolute, so H (>= 1) and d_rhoc = -w M1 F / (1 + G) move by up to 5.8e-5 of themselves,
#                     which on the scale |ref| + B >= 2 |ref| of the block's largest entry is 2.9e-5; TOL comes on top.
#   PHI_TOL = 1e-3    Hapke l_eq_v: phi = acos(cp) is 0 in float64 and up to sqrt(2 x 2.4e-7) = 6.9e-4 in float32.  d / d theta
#                     is first order in phi (the phi / pi E1 term of mu0, mu and f(phi) = exp(-2 tan(phi / 2)), slope -1 at 0),
#                     so it moves by up to 6.9e-4 of itself; the values see phi only through sums that the i == e arm keeps
#                     second order.
ACOS_TOL, G_TOL, PHI_TOL = 2e-2, 4e-5, 1e-3
ILL = {  # (family, row, quantity): (measured float32 oracle vs float64 oracle, its variant, bound)
    ("hapke", "l_eq_v", "d_theta"): (1.55e-04, "hapke/bct/4.0", PHI_TOL),
    ("hapke", "sun_back", "aux:S"): (1.51e-03, "hapke/bt/4.0", ACOS_TOL),
    ("hapke", "sun_back", "brdf"): (1.51e-03, "hapke/b/4.0", ACOS_TOL),
    ("hapke", "sun_back", "d_b"): (1.51e-03, "hapke/bc/1.3", ACOS_TOL),
    ("hapke", "sun_back", "d_c"): (1.51e-03, "hapke/bc/1.3", ACOS_TOL),
    ("hapke", "sun_back", "d_n"): (1.51e-03, "hapke/b/1.3", ACOS_TOL),
    ("hapke", "sun_back", "d_w"): (1.51e-03, "hapke/b/1.3", ACOS_TOL),
    ("rpv", "k_03_back", "aux:G"): (1.51e-03, "rpv/r", ACOS_TOL),
    ("rpv", "k_03_back", "d_rhoc"): (1.51e-03, "rpv/kr", ACOS_TOL),
    ("rpv", "l_eq_v", "aux:G"): (5.93e-03, "rpv/r", ACOS_TOL),
    ("rpv", "l_eq_v", "aux:H"): (7.98e-06, "rpv/r", G_TOL),
    ("rpv", "l_eq_v", "brdf"): (7.98e-06, "rpv/ktr", G_TOL),
    ("rpv", "l_eq_v", "d_n"): (7.95e-06, "rpv/ktr", G_TOL),
    ("rpv", "l_eq_v", "d_rhoc"): (1.87e-05, "rpv/kr", G_TOL),
    ("rpv", "l_eq_v", "d_theta"): (7.96e-06, "rpv/tr", G_TOL),
    ("rpv", "l_eq_v", "d_w"): (8.01e-06, "rpv/kr", G_TOL),
    ("rpv", "sun_back", "aux:G"): (1.51e-03, "rpv/r", ACOS_TOL),
    ("rpv", "sun_back", "d_rhoc"): (1.51e-03, "rpv/tr", ACOS_TOL),
    ("rpv", "view_back", "aux:G"): (1.51e-03, "rpv/r", ACOS_TOL),
    ("rpv", "view_back", "d_rhoc"): (1.51e-03, "rpv/tr", ACOS_TOL),
}


def on_branch_bound(family, row, quantity, rhoc_is_albedo=False):
    """The bound of one quantity ("brdf", "aux:<name>", "d_<group>") on one on-branch row: TOL unless the triple is in ILL.
    rhoc_is_albedo: d_w is the sum of the albedo's and rhoc's slots and takes the larger of their two bounds."""
    one = lambda q: ILL[(family, row, q)][2] if (family, row, q) in ILL else TOL[(family, q.split(":")[0])]
    return max(one("d_w"), one("d_rhoc")) if rhoc_is_albedo and quantity == "d_w" else one(quantity)


# NaN replacement and gradients.  Forward mode drops the derivative of a replaced value together with the value (nan_to returns
# the replacement, nan_to_num_ a constant); reverse-mode autograd of oracle/brdf.py multiplies the zero it sends into the replaced
# graph by that graph's infinite local derivatives and returns NaN, so on exactly these entries autograd is no reference.  What
# must hold instead is stated here and asserted on the device for both instantiations, whatever autograd says:
#   REPLACED_ZERO   (row, groups) where the replaced factor is the group's ONLY path to the value: the gradient is exactly 0
#     microfacet l_eq_mv, n_0       d = nan_to_num(alpha^2 chi / (pi cm^4 (alpha^2 + tan^2)^2)) with cm = 0 is 0 / (0 * inf),
#                                   replaced by 0: glossy = 0.04 d / (4 l.n v.n) is 0 with no derivative to the normal or the
#                                   roughness.  (cm = 0 also makes chi = 0 and d cm^2 = 0, so the kernel reaches this zero by
#                                   its structural-zero rule as well: the assertion holds the result, not one way to it.)
#     Hapke b + theta, mirror       f(phi = pi) = exp(-2 tan(pi / 2 + 5e-6)) = inf, S = temp / (1 - inf + inf ...) is NaN, replaced
#                                   by 0: brdf = (w / scl) t1 (P + Hi Hv - 1) * S is 0 with no derivative to any group
#   SUBSTITUTED     rows where the replacement has a derivative of its own: v_eq_n, l_eq_n of Hapke with theta, where phi is
#                   0 / 0 and mu0 -> cos i, mu -> cos e, f(phi) -> 0.  replaced_hapke restates the function with the replacements
#                   put in BEFORE differentiating; d / d theta of the rows comes from there.  (d / d n stays as it comes on
#                   those rows: acos' is infinite at ci = 1 or cv = 1 with or without the substitution.)
REPLACED_ZERO = {"microfacet": {"l_eq_mv": ("n", "rough"), "n_0": ("n", "rough")},
                 "hapke": {"mirror": ("n", "w", "b", "c", "theta")}}
SUBSTITUTED = {"hapke": ("v_eq_n", "l_eq_n")}


def replaced_zero(variant):
    """[(row name, group)] whose gradient must be exactly 0 in this variant."""
    s = VARIANTS[variant]
    if s["family"] == "hapke" and not ("b" in s["heads"] and "t" in s["heads"]):
        return []                                   # S exists only with theta, and reaches the value only with b
    gs = groups(variant)
    return [(nm, g) for nm, gg in REPLACED_ZERO.get(s["family"], {}).items() for g in gg if g in gs]


# ------------------------------------------------------------------------------------------------ the reference
class _TorchF32Inf:
    """`torch` as oracle/brdf.py sees it during a reference run: nan_to_num replaces +-inf by float32's largest value in every
    dtype (what the kernel's nan_to_num_ does; torch's default is the largest value of the tensor's own dtype)."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def nan_to_num(x, nan=0.0, posinf=None, neginf=None):
        return torch.nan_to_num(x, nan=nan, posinf=F32MAX, neginf=-F32MAX)


def _float32_infinities():
    """Context: oracle/brdf.py sees _TorchF32Inf as its `torch`.  It patches the module global, so it is not reentrant across
    threads: whatever calls the oracle inside the context sees the proxy (branch_trace does so on purpose)."""
    return mock.patch.object(OB, "torch", _TorchF32Inf())


def _variants():
    v = {}
    for bits in range(8):
        heads = "".join(h for i, h in enumerate("ktr") if bits >> i & 1)
        v["rpv/" + (heads or "none")] = dict(family="rpv", heads=heads)
    for scl in (4.0, 1.3):
        for heads in ("b", "bc", "bt", "bct"):
            v[f"hapke/{heads}/{scl}"] = dict(family="hapke", heads=heads, shell=0, hpk_scl=scl)
        for shell in (1, 2, 3):
            v[f"hapke/s{shell}/{scl}"] = dict(family="hapke", heads="", shell=shell, hpk_scl=scl)
        v[f"hapke/s3t/{scl}"] = dict(family="hapke", heads="t", shell=3, hpk_scl=scl)
    v["microfacet"] = dict(family="microfacet", heads="r")
    return v


VARIANTS = _variants()
FAMILIES = ("rpv", "hapke", "microfacet")
HEAD_GROUP = {"rpv": dict(k="k", t="theta", r="rhoc"), "hapke": dict(b="b", c="c", t="theta"), "microfacet": dict(r="rough")}
# the documented aux columns of the per-point kernels: quantity -> (first column, width)
AUX_COLS = {"rpv": dict(M1=(0, 3), G=(3, 1), H=(4, 3), ci=(7, 1), cv=(8, 1)),
            "hapke": dict(P=(0, 3), Hi=(3, 3), Hv=(6, 3), S=(9, 1), ci=(10, 1), cv=(11, 1)),
            "microfacet": dict(glossy=(0, 1), d=(3, 1), ldn=(4, 1), vdn=(5, 1), h=(6, 3), nh=(9, 1))}


def groups(variant, rhoc_is_albedo=False):
    """The differentiable input groups of a variant, in slot order."""
    s = VARIANTS[variant]
    if s["family"] == "microfacet":
        return ["n", "albedo", "rough"]
    g = ["n", "w"] + [HEAD_GROUP[s["family"]][h] for h in s["heads"]]
    return [x for x in g if not (rhoc_is_albedo and x == "rhoc")]


def _call(variant, l, v, x, rhoc_is_albedo=False):
    """oracle/brdf.py on one variant.  x: group -> tensor.  -> brdf [N][3], {aux quantity: [N][w]}."""
    s = VARIANTS[variant]
    col = lambda t: t.reshape(t.shape[0], -1)
    if s["family"] == "rpv":
        rhoc = x["w"] if rhoc_is_albedo else x.get("rhoc")
        brdf, M1, G, H, ci, cv = OB.rpv(l, v, x["n"], x["w"], x.get("k"), x.get("theta"), rhoc)
        aux = dict(M1=M1.expand(-1, 3), G=G, H=H.expand(-1, 3), ci=ci, cv=cv)
    elif s["family"] == "hapke":
        brdf, P, _, Hi, Hv, S, ci, cv = OB.hapke(l, v, x["n"], x["w"], x.get("b"), x.get("c"), x.get("theta"), s["hpk_scl"], s["shell"])
        aux = dict(P=P, Hi=Hi, Hv=Hv, S=S, ci=ci, cv=cv)
    else:
        glossy, brdf, _, _, d, ldn, vdn, h, nh = OB.microfacet(l, v, x["n"], x["albedo"], x["rough"], F0)
        aux = dict(glossy=glossy, d=d, ldn=ldn, vdn=vdn, h=h, nh=nh)
    return brdf, {k: col(a).detach() for k, a in aux.items()}


def replaced_hapke(variant, tab, rows, dtype):
    """Hapke with theta on rows where phi is NaN (SUBSTITUTED), the replacements put in before differentiating: mu0 = cos i,
    mu = cos e, f(phi) = 0, so S = (mu / eta_e) (cos i / eta_i) chi / (1 - 0 + 0).  Built from the oracle's own _eta, _chi, _HF,
    _PF.  -> brdf [R][3], d brdf / d theta [R][3][1], J_theta^T d_brdf [R][1]."""
    s = VARIANTS[variant]
    x = {g: tab[g][rows].to(dtype) for g in groups(variant)}
    th = x["theta"].clone().requires_grad_(True)
    with _float32_infinities():
        _, sza, _, _, vza, _, cg, _, phi = OB.calc_angles(tab["l"][rows].to(dtype), tab["v"][rows].to(dtype), x["n"])
        assert bool(torch.isnan(phi).all())
        mu0, mu = torch.cos(sza), torch.cos(vza)
        S = ((mu / OB._eta(vza, th)) * (mu0 / OB._eta(sza, th)) * OB._chi(th)).unsqueeze(-1)
        Hi, Hv = OB._HF(mu0.unsqueeze(-1), x["w"]), OB._HF(mu.unsqueeze(-1), x["w"])
        if "b" not in s["heads"]:
            assert s["shell"] == 3
            brdf = x["w"] * (Hi * Hv) / ((mu0 + mu) * s["hpk_scl"] + 1e-6).unsqueeze(-1) + 0 * th.unsqueeze(-1)
        else:
            cgx = cg.unsqueeze(-1)
            P = OB._PF(cgx, x["b"], x["c"]) if "c" in s["heads"] else OB.henyey_greenstein(cgx, x["b"])
            brdf = x["w"] / s["hpk_scl"] * (mu0 / (mu0 + mu) / torch.cos(sza)).unsqueeze(-1) * (P + Hi * Hv - 1) * S
        R = brdf.shape[0]
        vjp = lambda d: torch.autograd.grad(brdf, th, grad_outputs=d, retain_graph=True)[0].reshape(R, 1)
        eye = torch.eye(3, dtype=dtype)
        jac = torch.stack([vjp(eye[c].expand(R, 3)) for c in range(3)], 1)
        return brdf.detach(), jac, vjp(tab["d_brdf"][rows].to(dtype))


def evaluate(variant, tab, dtype, rhoc_is_albedo=False, jac=True, names=None):
    """The oracle on the table's rows in `dtype`: {"brdf": [N][3], "aux": {quantity: [N][w]}, "jac": {group: [N][3][w]},
    "rnd": {group: [N][w]}} - jac[g][r][c] = d brdf_c / d g of row r, rnd = J^T d_brdf for tab["d_brdf"].  names (the on-branch
    table's row names): d / d theta of the SUBSTITUTED rows is taken from replaced_hapke."""
    gs = groups(variant, rhoc_is_albedo)
    x = {g: tab[g].to(dtype).clone().requires_grad_(jac) for g in gs}
    l, v = tab["l"].to(dtype), tab["v"].to(dtype)
    with _float32_infinities():
        brdf, aux = _call(variant, l, v, x, rhoc_is_albedo)
        out = {"brdf": brdf.detach(), "aux": aux}
        if not jac:
            return out
        N = brdf.shape[0]
        leaves = [x[g] for g in gs]

        def vjp(d_brdf):
            if not brdf.requires_grad:
                return [torch.zeros_like(t).reshape(N, -1) for t in leaves]
            gr = torch.autograd.grad(brdf, leaves, grad_outputs=d_brdf, retain_graph=True, allow_unused=True)
            return [(torch.zeros_like(t) if g_ is None else g_).reshape(N, -1) for g_, t in zip(gr, leaves)]

        rows = []
        for c in range(3):
            e = torch.zeros(N, 3, dtype=dtype)
            e[:, c] = 1
            rows.append(vjp(e))
        out["jac"] = {g: torch.stack([rows[c][i] for c in range(3)], 1) for i, g in enumerate(gs)}
        out["rnd"] = dict(zip(gs, vjp(tab["d_brdf"].to(dtype))))
    s = VARIANTS[variant]
    if names is not None and s["family"] == "hapke" and "t" in s["heads"]:
        rows = torch.tensor([names.index(nm) for nm in SUBSTITUTED["hapke"]])
        b, j, r = replaced_hapke(variant, tab, rows, dtype)
        out["replaced_brdf"] = (rows, b)
        out["jac"]["theta"][rows], out["rnd"]["theta"][rows] = j, r
    return out


# ------------------------------------------------------------------------------------------------ error scaling
def _ratio(err, den, mask=None):
    r = torch.where(err == 0, torch.zeros_like(err), err / den)       # NaN stays NaN: a comparison with it fails
    if mask is not None:
        r = r[mask]
    if not r.numel():
        return 0.0, -1
    i = int(torch.argmax(torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)))
    return float(r.reshape(-1)[i]), i


def _amax(t, dims, mask=None):
    a = t.abs() if mask is None else torch.where(mask, t.abs(), torch.zeros_like(t))
    return torch.nan_to_num(a, nan=0.0).amax(dims, keepdim=True)


def _worst_row(i, shape, mask):
    """Row of flat index i (into the masked entries where a mask is given)."""
    if i < 0:
        return -1
    per_row = int(torch.tensor(shape[1:]).prod()) if len(shape) > 1 else 1
    if mask is not None:
        i = int(mask.reshape(-1).nonzero()[i])
    return i // per_row


def err_rows(got, ref, mask=None):
    """[N][w] quantity (brdf, an aux quantity): each row scaled by its own largest magnitude.  -> (error, row)."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.detach().double()
    e, i = _ratio((got - ref).abs(), ref.abs() + _amax(ref, -1, mask), mask)
    return e, _worst_row(i, ref.shape, mask)


err_values = err_aux = err_rows


def err_jac(got, ref, mask=None):
    """[N][3][w] Jacobian blocks of one input group.  -> (error, row)."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.detach().double()
    e, i = _ratio((got - ref).abs(), ref.abs() + _amax(ref, (1, 2), mask), mask)
    return e, _worst_row(i, ref.shape, mask)


def err_rnd(got, ref, jac_ref, d_brdf, mask=None, jac_mask=None):
    """[N][w] J^T d_brdf of one input group against the reference's, on the block scale times sum_c |d_brdf_c|."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.detach().double()
    s = _amax(jac_ref.double(), (1, 2), jac_mask).reshape(-1, 1) * d_brdf.double().abs().sum(-1, keepdim=True)
    e, i = _ratio((got - ref).abs(), ref.abs() + s, mask)
    return e, _worst_row(i, ref.shape, mask)


def structural_zero_errors(got, ref, mask=None):
    """Entries whose reference is exactly 0 and whose kernel value is not."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.detach().double()
    z = ref == 0
    if mask is not None:
        z = z & mask
    return int((z & (got != 0)).sum()), int(z.sum())


def compare(variant, got, ref, tab, masks=None, rhoc_is_albedo=False, split_aux=False):
    """-> {quantity: (scaled error, row)} for brdf, "aux" (the worst of the aux quantities `got` holds; split_aux: each of them as
    "aux:<name>") and d_<group> (the worst of the three Jacobian rows and the random row), and the count of structural zeros that
    are not zero.  masks (on-branch rows): {"jac": {group: bool [N][3][w]}, "rnd": {group: bool [N][w]}}: the entries that are
    finite in float64."""
    fam = VARIANTS[variant]["family"]
    e = {"brdf": err_values(got["brdf"], ref["brdf"], None if masks is None else masks["brdf"])}
    if got.get("aux") is not None:
        each = {q: err_aux(got["aux"][q], r, None if masks is None else masks["aux"][q]) for q, r in ref["aux"].items()}
        if split_aux:
            e.update({"aux:" + q: t for q, t in each.items()})
        else:
            e["aux"] = max(each.values(), key=lambda t: math.inf if t[0] != t[0] else t[0])
    bad = 0
    for g in groups(variant, rhoc_is_albedo):
        mj = None if masks is None else masks["jac"][g]
        mr = None if masks is None else masks["rnd"][g]
        a = err_jac(got["jac"][g], ref["jac"][g], mj)
        b = err_rnd(got["rnd"][g], ref["rnd"][g], ref["jac"][g], tab["d_brdf"], mr, mj)
        e["d_" + g] = max(a, b, key=lambda t: math.inf if t[0] != t[0] else t[0])
        bad += structural_zero_errors(got["jac"][g], ref["jac"][g], mj)[0]
    return e, bad, fam


def finite_masks(ref):
    """What of an on-branch reference is finite in float64 (test_brdf_cpu.py records it, the GPU comparison keeps to it)."""
    fin = torch.isfinite
    return {"brdf": fin(ref["brdf"]), "aux": {q: fin(a) for q, a in ref["aux"].items()},
            "jac": {g: fin(j) for g, j in ref["jac"].items()}, "rnd": {g: fin(j) for g, j in ref["rnd"].items()}}


def compare_rows(variant, got, ref, tab, names, masks, rhoc_is_albedo=False):
    """compare, one on-branch row at a time, every aux quantity on its own.  -> {(row name, quantity): scaled error}, the count
    of structural zeros that are not zero."""
    cpu = lambda t: t.detach().cpu() if torch.is_tensor(t) else {k: cpu(a) for k, a in t.items()}
    got = {k: cpu(got[k]) for k in ("brdf", "aux", "jac", "rnd") if got.get(k) is not None}
    out, bad = {}, 0
    for r, nm in enumerate(names):
        rows = torch.zeros(len(names), dtype=torch.bool)
        rows[r] = True
        e, b, _ = compare(variant, got, ref, tab, row_masks(masks, rows), rhoc_is_albedo, split_aux=True)
        out.update({(nm, q): v for q, (v, _) in e.items()})
        bad += b
    return out, bad


def row_masks(masks, rows):
    """finite_masks restricted to the rows where `rows` (bool [N]) is set."""
    cut = lambda m: m & rows.reshape([-1] + [1] * (m.dim() - 1))
    return {k: cut(v) if torch.is_tensor(v) else {q: cut(m) for q, m in v.items()} for k, v in masks.items()}


# ------------------------------------------------------------------------------------------------ the well-posed table
def geometry(l, v, n):
    """calc_angles' deciding intermediates in float64, before any clamp."""
    l, v, n = l.double(), v.double(), n.double()
    ci, cv, cg = (l * n).sum(-1), (v * n).sum(-1), (v * l).sum(-1)
    si, sv = torch.sqrt((1 - ci * ci).clamp_min(0)), torch.sqrt((1 - cv * cv).clamp_min(0))
    cp = (cg - ci * cv) / (si * sv)
    return ci, cv, cg, cp, torch.acos(ci.clamp(-1, 1)), torch.acos(cv.clamp(-1, 1))


def margins(family, tab):
    """bool [N]: the margin predicate, judged in float64 alone."""
    l, v, n = tab["l"], tab["v"], tab["n"]
    ci, cv, cg, cp, sza, vza = geometry(l, v, n)
    inside = lambda t, lo, hi: ((t.double() >= lo) & (t.double() <= hi)).reshape(t.shape[0], -1).all(-1)
    ok = inside(ci, M, 1 - M) & inside(cv, M, 1 - M) & (cg.abs() <= 1 - M) & (cp.abs() <= 1 - M) & ((sza - vza).abs() >= M)
    if family == "rpv":
        ok &= inside(tab["w"], 0.05, 0.95) & inside(tab["k"], 0.3, 1.8) & ((tab["k"].double() - 1).abs() >= M).all(-1)
        ok &= inside(tab["theta"], -0.8, 0.8) & inside(tab["rhoc"], 0.05, 0.95)
    elif family == "hapke":
        ok &= inside(tab["w"], 0.05, 0.95) & inside(tab["b"], 0.0, 0.8) & inside(tab["c"], 0.0, 1.0) & inside(tab["theta"], 0.05, 0.5)
    else:
        nrm = lambda t: t.double() / t.double().norm(dim=-1, keepdim=True)
        ld, vd, nd = nrm(l), nrm(v), nrm(n)
        h = nrm(ld + vd)
        ok &= ((h * nd).sum(-1) >= M) & ((ld * nd).sum(-1).abs() >= 0.001 + M) & ((vd * nd).sum(-1).abs() >= 0.001 + M)
        ok &= inside(tab["albedo"], 0.05, 0.95) & inside(tab["rough"], 0.05, 1.0)
    return ok


def _draw(family, g, n, lv=None):
    """n candidate rows: sun and view over the upper hemisphere (the fuzz test's distribution), normals from nadir to a 60 degree
    tilt, parameters strictly inside their ranges."""
    U = lambda *shape: torch.rand(*shape, generator=g)

    def hemi(spread):
        return torch.nn.functional.normalize(torch.cat([spread * torch.randn(n, 2, generator=g), torch.ones(n, 1)], -1), dim=-1)

    l, v = (hemi(0.6), hemi(0.8)) if lv is None else lv
    tilt, az = U(n) * (math.pi / 3), U(n) * (2 * math.pi)
    t = dict(l=l, v=v, n=torch.stack([torch.sin(tilt) * torch.cos(az), torch.sin(tilt) * torch.sin(az), torch.cos(tilt)], -1))
    if family == "rpv":
        k = 0.3 + U(n, 3) * (1.5 - 2 * M)
        t.update(w=0.05 + 0.9 * U(n, 3), k=torch.where(k > 1 - M, k + 2 * M, k), theta=1.6 * U(n, 3) - 0.8, rhoc=0.05 + 0.9 * U(n, 3))
    elif family == "hapke":
        t.update(w=0.05 + 0.9 * U(n, 3), b=0.8 * U(n, 3), c=U(n, 3), theta=0.05 + 0.45 * U(n))
    else:
        t.update(albedo=0.05 + 0.9 * U(n, 3), rough=0.05 + 0.95 * U(n, 1))
    t["d_brdf"] = 2 * U(n, 3) - 1
    return t


SEEDS = {"rpv": 7101, "hapke": 7102, "microfacet": 7103}
DRAW_BATCH = 1024


def well_posed(family):
    """The first N_ROWS rows of the seeded draw that keep the margin.  -> (table, rows drawn)."""
    g = torch.Generator().manual_seed(SEEDS[family])
    kept, drawn = None, 0
    while kept is None or kept["l"].shape[0] < N_ROWS:
        t = _draw(family, g, DRAW_BATCH)
        ok = margins(family, t)
        drawn += DRAW_BATCH
        t = {k: a[ok] for k, a in t.items()}
        kept = t if kept is None else {k: torch.cat([kept[k], t[k]]) for k in t}
    return {k: a[:N_ROWS].contiguous() for k, a in kept.items()}, drawn


TWO_BLOCK = dict(R=37, S1=3, S2=2)


def two_block(family):
    """Rows for the two-block layout of the per-sample launch: R rays of S1 rows, then R rays of S2 rows, every row's normal and
    parameters drawn until the row keeps the margin under ITS ray's sun and view.  -> table whose l, v are per row (gathered),
    with "ray_l", "ray_v" [R][3] and "row_ray" beside them."""
    R, S1, S2 = TWO_BLOCK["R"], TWO_BLOCK["S1"], TWO_BLOCK["S2"]
    g = torch.Generator().manual_seed(SEEDS[family] + 50)
    per, rows, ray_l, ray_v = S1 + S2, [], [], []
    while len(rows) < R:
        lv = _draw(family, g, 1)
        cand = _draw(family, g, 64, (lv["l"].expand(64, 3), lv["v"].expand(64, 3)))
        ok = margins(family, cand)
        if int(ok.sum()) < per:
            continue
        rows.append({k: a[ok][:per] for k, a in cand.items()})
        ray_l.append(lv["l"][0])
        ray_v.append(lv["v"][0])
    # row order of the launch: block 1 = rows [0, S1) of every ray, block 2 = rows [S1, S1 + S2)
    t = {k: torch.cat([r[k][:S1] for r in rows] + [r[k][S1:] for r in rows]).contiguous() for k in rows[0]}
    ar = torch.arange(R)
    t.update(ray_l=torch.stack(ray_l), ray_v=torch.stack(ray_v), row_ray=torch.cat([ar.repeat_interleave(S1), ar.repeat_interleave(S2)]))
    assert torch.equal(t["l"], t["ray_l"][t["row_ray"]]) and torch.equal(t["v"], t["ray_v"][t["row_ray"]])
    return t


# ------------------------------------------------------------------------------------------------ the on-branch table
_Z = (0.0, 0.0, 1.0)
_L0, _V0 = (0.5, 0.0, 0.75), (0.25, 0.5, 0.5)           # a dyadic geometry away from every branch: ci 0.75, cv 0.5, cg 0.5
_BASE = {"rpv": dict(w=(0.25, 0.5, 0.75), k=(0.5, 0.75, 1.5), theta=(-0.5, 0.25, 0.5), rhoc=(0.25, 0.5, 0.75)),
         "hapke": dict(w=(0.25, 0.5, 0.75), b=(0.25, 0.5, 0.75), c=(0.25, 0.5, 0.75), theta=0.25),
         "microfacet": dict(albedo=(0.25, 0.5, 0.75), rough=(0.5,))}
_GEOMETRY_ROWS = [
    ("sun_back", dict(l=(0.5, 0.5, -0.5), v=(0.0, 0.5, 0.75), n=_Z)),          # l.n = -0.5: ci clamps to 1e-5
    ("view_back", dict(l=(0.0, 0.5, 0.75), v=(0.5, 0.5, -0.5), n=_Z)),         # v.n = -0.5: cv clamps to 1e-5
    ("v_eq_n", dict(l=_L0, v=_Z, n=_Z)),                                       # sv = 0, phi = acos(0 / 0)
    ("l_eq_n", dict(l=_Z, v=_L0, n=_Z)),                                       # si = 0, phi = acos(0 / 0)
    ("l_eq_v", dict(l=_Z, v=_Z, n=(0.5, 0.0, 0.75))),                          # cg = 1 exactly, i == e exactly
    ("mirror", dict(l=(0.75, 0.0, 0.75), v=(-0.75, 0.0, 0.75), n=_Z)),         # i == e, cp = -0.5625 / 0.4375 clamps to -1: phi = pi
]
ON_BRANCH_ROWS = {
    "rpv": _GEOMETRY_ROWS + [
        ("k_1", dict(k=(1.0, 1.0, 1.0))),                                      # exponent 0
        ("k_03_back", dict(l=(0.5, 0.5, -0.5), v=(0.0, 0.5, 0.75), k=(0.3, 0.3, 0.3))),   # a tiny base under a negative exponent
        ("theta_0", dict(theta=(0.0, 0.0, 0.0))),
        ("theta_p1", dict(theta=(1.0, 1.0, 1.0))),
        ("theta_m1", dict(theta=(-1.0, -1.0, -1.0))),
    ],
    "hapke": _GEOMETRY_ROWS + [
        ("theta_0", dict(theta=0.0)),
        ("w_1", dict(w=(1.0, 1.0, 1.0))),                                      # gamma = 0
        ("w_0", dict(w=(0.0, 0.0, 0.0))),
    ],
    "microfacet": _GEOMETRY_ROWS + [
        ("hn_neg", dict(l=(0.5, 0.0, -0.75), v=(0.25, 0.5, -0.5))),            # h.n < 0: chi = 0
        ("l_eq_mv", dict(l=(0.5, 0.0, 0.75), v=(-0.5, 0.0, -0.75))),           # l = -v: the half-vector is zero
        ("n_0", dict(n=(0.0, 0.0, 0.0))),
        ("rough_0", dict(rough=(0.0,))),
    ],
}


def on_branch(family):
    """-> (table, row names).  Rows without a geometry of their own take (_L0, _V0, nadir), rows without parameters _BASE."""
    names = [nm for nm, _ in ON_BRANCH_ROWS[family]]
    base = dict(l=_L0, v=_V0, n=_Z, **_BASE[family])
    cols = {k: torch.tensor([dict(base, **over)[k] for _, over in ON_BRANCH_ROWS[family]], dtype=torch.float32) for k in base}
    g = torch.Generator().manual_seed(SEEDS[family] + 90)
    cols["d_brdf"] = 2 * torch.rand(len(names), 3, generator=g) - 1
    return cols, names


# What each on-branch row must show (branch_trace returns the same dictionary in float32 and in float64).
EXPECTED_TRACE = {
    "sun_back": {"ci == 1e-5": True, "cv == 1e-5": False, "isnan(phi)": False},
    "view_back": {"ci == 1e-5": False, "cv == 1e-5": True, "isnan(phi)": False},
    "v_eq_n": {"cv == 1": True, "sv == 0": True, "isnan(phi)": True, "rpv G == 0": True, "hapke mu0 == cos i": True, "hapke mu == cos e": True},
    "l_eq_n": {"ci == 1": True, "si == 0": True, "isnan(phi)": True, "rpv G == 0": True, "hapke mu0 == cos i": True, "hapke mu == cos e": True},
    "l_eq_v": {"cg == 1": True, "i == e": True, "isnan(phi)": False},
    "mirror": {"i == e": True, "phi == pi": True},
    "k_1": {"k - 1 == 0": True, "M1 == 1": True},
    "k_03_back": {"ci == 1e-5": True, "base < 2e-5": True, "M1 > 1e3": True},
    "theta_0": {"theta == 0": True},
    "theta_p1": {"1 - theta^2 == 0": True, "brdf == 0": True},
    "theta_m1": {"1 - theta^2 == 0": True, "brdf == 0": True},
    "w_1": {"gamma == 0": True},
    "w_0": {"brdf == 0": True},
    "hn_neg": {"chi == 0": True, "d == 0": True},
    "l_eq_mv": {"h == 0": True, "d == 0": True},
    "n_0": {"n.h == 0": True, "l.n == 0.001": True, "v.n == 0.001": True, "d == 0": True},
    "rough_0": {"alpha == 0": True, "d == 0": True},
}


def branch_trace(dtype):
    """{family: {row: {fact: bool}}}: the intermediates that prove which arm each on-branch row takes, computed from the oracle's
    own statements in `dtype`."""
    out = {}
    for fam in FAMILIES:
        tab, names = on_branch(fam)
        c = {k: a.to(dtype) for k, a in tab.items()}
        ci, sza, si, cv, vza, sv, cg, g_, phi = OB.calc_angles(c["l"], c["v"], c["n"])
        eps = torch.tensor(1e-5, dtype=dtype)
        rows = {}
        with _float32_infinities():
            if fam == "rpv":
                brdf, M1, G, _, _, _ = OB.rpv(c["l"], c["v"], c["n"], c["w"], c["k"], c["theta"], c["rhoc"])
            elif fam == "hapke":
                brdf, _, _, _, _, _, mu0, mu = OB.hapke(c["l"], c["v"], c["n"], c["w"], c["b"], c["c"], c["theta"], 4.0, 0)
            else:
                _, brdf, _, _, d, ldn, vdn, h, nh = OB.microfacet(c["l"], c["v"], c["n"], c["albedo"], c["rough"], F0)
        for r, nm in enumerate(names):
            f = {}
            B = lambda t: bool(t)
            if nm in ("sun_back", "view_back"):
                f = {"ci == 1e-5": B(ci[r] == eps), "cv == 1e-5": B(cv[r] == eps), "isnan(phi)": B(torch.isnan(phi[r]))}
            elif nm in ("v_eq_n", "l_eq_n"):
                f = {"cv == 1": B(cv[r] == 1), "sv == 0": B(sv[r] == 0)} if nm == "v_eq_n" else {"ci == 1": B(ci[r] == 1), "si == 0": B(si[r] == 0)}
                f["isnan(phi)"] = B(torch.isnan(phi[r]))
                if fam == "rpv":
                    f["rpv G == 0"] = B((G[r] == 0).all())
                if fam == "hapke":
                    f["hapke mu0 == cos i"] = B(mu0[r] == torch.cos(sza[r]))
                    f["hapke mu == cos e"] = B(mu[r] == torch.cos(vza[r]))
            elif nm == "l_eq_v":
                f = {"cg == 1": B(cg[r] == 1), "i == e": B(sza[r] == vza[r]), "isnan(phi)": B(torch.isnan(phi[r]))}
            elif nm == "mirror":
                f = {"i == e": B(sza[r] == vza[r]), "phi == pi": B(phi[r] == torch.acos(torch.tensor(-1.0, dtype=dtype)))}
            elif nm == "k_1":
                f = {"k - 1 == 0": B((c["k"][r] - 1 == 0).all()), "M1 == 1": B((M1[r] == 1).all())}
            elif nm == "k_03_back":
                f = {"ci == 1e-5": B(ci[r] == eps), "base < 2e-5": B(ci[r] * cv[r] * (ci[r] + cv[r]) + 1e-5 < 2e-5), "M1 > 1e3": B((M1[r] > 1e3).all())}
            elif nm == "theta_0":
                f = {"theta == 0": B((c["theta"][r] == 0).all())}
            elif nm in ("theta_p1", "theta_m1"):
                f = {"1 - theta^2 == 0": B((1 - c["theta"][r] ** 2 == 0).all()), "brdf == 0": B((brdf[r] == 0).all())}
            elif nm == "w_1":
                f = {"gamma == 0": B((torch.sqrt(1 - c["w"][r]) == 0).all())}
            elif nm == "w_0":
                f = {"brdf == 0": B((brdf[r] == 0).all())}
            elif nm == "hn_neg":
                f = {"chi == 0": B(nh[r] < 0), "d == 0": B(d[r] == 0)}
            elif nm == "l_eq_mv":
                f = {"h == 0": B((h[r] == 0).all()), "d == 0": B(d[r] == 0)}
            elif nm == "n_0":
                f = {"n.h == 0": B(nh[r] == 0), "l.n == 0.001": B(ldn[r] == torch.tensor(0.001, dtype=dtype)),
                     "v.n == 0.001": B(vdn[r] == torch.tensor(0.001, dtype=dtype)), "d == 0": B(d[r] == 0)}
            elif nm == "rough_0":
                f = {"alpha == 0": B(c["rough"][r] ** 2 == 0), "d == 0": B(d[r] == 0)}
            rows[nm] = f
        out[fam] = rows
    return out


def expected_trace(family):
    """EXPECTED_TRACE restricted to the facts that exist in a family (rpv G / hapke mu only there)."""
    keep = lambda fact: not ((fact.startswith("rpv ") and family != "rpv") or (fact.startswith("hapke ") and family != "hapke"))
    return {nm: {k: v for k, v in EXPECTED_TRACE[nm].items() if keep(k)} for nm, _ in ON_BRANCH_ROWS[family]}


_CACHE = {}


def table(family, kind="well_posed"):
    """The shared, unchanged tables: kind in well_posed / on_branch / two_block."""
    key = (family, kind)
    if key not in _CACHE:
        _CACHE[key] = {"well_posed": lambda: well_posed(family)[0], "on_branch": lambda: on_branch(family)[0],
                       "two_block": lambda: two_block(family)}[kind]()
    return _CACHE[key]


def reference(variant, kind="well_posed", rhoc_is_albedo=False):
    """The float64 reference of a variant on one of the tables, computed once."""
    key = (variant, kind, rhoc_is_albedo, "ref")
    if key not in _CACHE:
        fam = VARIANTS[variant]["family"]
        _CACHE[key] = evaluate(variant, table(fam, kind), torch.float64, rhoc_is_albedo,
                               names=on_branch(fam)[1] if kind == "on_branch" else None)
    return _CACHE[key]


def variants_of(family):
    return [v for v, s in VARIANTS.items() if s["family"] == family]
