"""CPU side of tests/test_gpu_ray_kernels_f64.py: the float64 reference of the lean step's per-ray kernels
(tests/ray_kernel_cases.py) checked against the oracle, its tolerances derived from its own float32 evaluation, the coverage
of the case table, and a strength check: references perturbed the way the kernels could be wrong leave the tolerances."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_kernel_cases as K  # noqa: E402
from oracle import losses as OL, render as ORD  # noqa: E402


# ------------------------------------------------------------------------------------------------ restatement vs oracle
@pytest.mark.parametrize("name", list(K.CASES)[::7])
def test_composite_ref_is_the_oracles_composite_bitwise(name):
    c = K.CASES[name]
    z, idx, o1, o2 = K.inputs(c, torch.float32)
    rows = K.merged_rows(idx, o1, o2)
    for noise, std in ((None, 0.0), (c["noise"], K.NOISE_STD)):
        o = K.composite_ref(z, rows[..., 3], noise, std, rows)
        a, T, w, d = ORD.composite(z, rows[..., 3], noise, std)
        assert torch.equal(o["alphas"], a) and torch.equal(o["trans"], T) and torch.equal(o["weights"], w) and torch.equal(o["depth"], d)
        assert torch.equal(o["wsum"], w.sum(-1)) and torch.equal(o["acc"], (w.unsqueeze(-1) * rows).sum(-2))
        assert torch.equal(o["var"], ORD.depth_std(z, d, w) ** 2) or float((o["var"].sqrt() - ORD.depth_std(z, d, w)).abs().max()) == 0.0


@pytest.mark.parametrize("name", list(K.CASES)[3::9])
def test_loss_terms_are_the_oracles(name):
    """The tail's total and per-ray terms, the regulariser terms and the NormalLoss term against oracle/losses.py (held to the
    reference's goldens in test_oracle_golden.py), in float64."""
    c = K.CASES[name]
    z, idx, o1, o2 = K.inputs(c, torch.float64)
    rows = K.merged_rows(idx, o1, o2)
    rgbs = c["rgbs"].double()
    for cfg in K.TAIL_CONFIGS.values():
        prior = K.prior_of(c, torch.float64) if cfg["prior"] else None
        t = K.tail_ref(z, idx, o1, o2, rgbs, K.PAD, K.LAMBDA_RGB, prior, K.LAMBDA_DS if prior else 0.0, cfg.get("usealldepth", False))
        res = {"rgb_coarse": t["rgb"], "z_vals_coarse": z, "depth_coarse": t["depth"], "weights_coarse": t["weights"]}
        want = OL.snerf_loss(res, rgbs, K.LAMBDA_RGB)
        if prior is not None:
            valid, td, tw, ts = prior
            want = want + OL.depth_loss(res, td, tw, valid, ts, K.LAMBDA_DS, cfg.get("usealldepth", False))
        assert abs(float(t["total"]) - float(want)) <= 1e-13 * abs(float(want))
        assert abs(float(t["ray_loss"].sum()) - float(want)) <= 1e-13 * abs(float(want))
    nreg = K.nreg_of(c, spv=True)
    if nreg is not None:
        f = K.forward_ref(z, idx, o1, o2, nreg)
        res = {"weights_coarse": f["weights"], "rays_d_coarse": nreg["view"].double()}
        want = 0.0
        for key, ch, lam in (("an", nreg["ch_an"], K.LAM_AN), ("lr", nreg["ch_lr"], K.LAM_LR)):
            res[key + "_coarse"] = rows[..., ch:ch + 3]
            want = want + OL.normal_reg_loss(res, key, lam)[0]
        assert abs(float(f["reg"].sum()) - float(want)) <= 1e-13 * abs(float(want))
        spv = OL.normal_loss(f["weights"], rows[..., nreg["spv_an"]:nreg["spv_an"] + 3], rows[..., nreg["spv_lr"]:nreg["spv_lr"] + 3], K.LAM_SPV)
        assert abs(float(f["spv_loss"]) - float(spv)) <= 1e-13 * abs(float(spv))
        assert abs(float(f["spv_tot"][2]) - float(spv)) <= 1e-13 * abs(float(spv))


def test_guided_ref_is_the_oracles_guided_samples():
    c = K.GUIDED_CASES["S65_G64_prior_R9"] if "S65_G64_prior_R9" in K.GUIDED_CASES else next(v for v in K.GUIDED_CASES.values() if v["prior"])
    r = K.guided_reference(c, torch.float64)
    z = c["z"].double()
    _, _, w, d = ORD.composite(z, c["sigma"].double())
    sel = c["valid"] > 0
    rnd = ORD.Randoms(replay=[c["u"].double(), c["u_t"].double()[sel]])
    z2, _, _ = ORD.guided_samples(d, w, z, c["G"], torch.tensor(0.0, dtype=torch.float64), torch.tensor(K.FAR, dtype=torch.float64), rnd, 3.0,
                                  "train", c["valid"].double(), c["depths"][:, :1].double(), c["tstd"][:, 0].double())
    assert torch.equal(r["z2"], torch.sort(z2, -1)[0])
    assert bool((r["z_all"][:, 1:] >= r["z_all"][:, :-1]).all())
    assert torch.equal(torch.cat([z, r["z2"]], -1).gather(1, r["idx"]), r["z_all"])


# ------------------------------------------------------------------------------------------------ the table
def test_case_table_covers_the_lane_layouts():
    cpl, seen = set(), set()
    for c in K.CASES.values():
        assert 1 <= c["R"] <= 13 and c["R"] % 4 != 0
        cpl.add((c["S2"] + 63) // 64)
        seen.add((c["S2"], c["split"] if c["S1"] == c["S2"] else c["S1"]))
        seen.add((c["S2"], "C" + c["cvar"]))
        if c["idx"] is not None and c["out2"] is not None:            # a real interleave with exact ties
            assert bool((c["idx"][:, 1:] < c["idx"][:, :-1]).any()) or c["S2"] <= 2
        if c["S1"] >= 4:                                              # rows with delta = 0
            assert bool((c["z_all"][:, 1:] == c["z_all"][:, :-1]).any())
    assert cpl == {1, 2, 3, 8}          # the S2 list: full lanes at 1, 2, 3 and 8 samples per lane, ragged at 2, 3 and 8
    assert any(c["R"] == 1 for c in K.CASES.values())
    for S2 in K.S2_LIST:
        for cv in K.CVARS:
            assert (S2, "C" + cv) in seen, (S2, cv)
        assert (S2, "none") in seen and (S2, "identity") in seen
        if S2 >= 2:
            assert (S2, 1) in seen and (S2, S2 - 1) in seen and (S2, S2 // 2) in seen
    pats = {p for c in K.CASES.values() if c["R"] >= 6 for p in c["patterns"]}
    assert pats == set(K.PATTERNS)
    assert {(c["S"], c["G"]) for c in K.GUIDED_CASES.values()} == set(K.GUIDED_SG)


def test_tail_cases_reach_every_clamp_side_and_prior_clause():
    """Every case that holds all six density patterns has rays with a colour sum below 0, inside [0, 1] and above 1, and a prior
    on each clause of the `apply` condition."""
    n = 0
    for name, c in K.CASES.items():
        if c["R"] < 6:
            continue
        n += 1
        z, idx, o1, o2 = K.inputs(c, torch.float64)
        rows = K.merged_rows(idx, o1, o2)
        o = K.composite_ref(z, rows[..., 3], None, 0.0, rows)
        x = o["acc"][:, :3] * (1 + 2 * K.PAD) - K.PAD * o["wsum"].unsqueeze(-1)
        assert bool((x < 0).any()) and bool(((x > 0) & (x < 1)).any()) and bool((x > 1).any()), name
        valid, td, tw, ts = K.prior_of(c, torch.float64)
        a = ((o["depth"] - td).abs() - ts) > 0
        b = ts < o["var"].sqrt()
        v = valid > 0
        assert bool((v & a & ~b).any()) and bool((v & ~a & ~b).any()) and bool((~v).any()), name
        if c["S2"] >= 3:                                             # (one or two samples: no ray with a spread)
            assert bool((v & ~a & b).any()), name
        # the decisions sit far from their thresholds: float32 takes the same ones
        assert float((((o["depth"] - td).abs() - ts).abs() / ts).min()) > 0.2 and float(((ts - o["var"].sqrt()).abs() / ts)[v].min()) > 0.2, name
    assert n >= 90


# ------------------------------------------------------------------------------------------------ the tolerances
def _case_errors(c):
    r64, r32 = K.reference_all(c, torch.float64), K.reference_all(c, torch.float32)
    e = {}
    for part in r64:
        for q, v in K.compare(r32[part], r64[part], c).items():
            e[q] = max(e.get(q, 0.0), v) if v == v else float("nan")
    return e


def _guided_errors(c):
    e = {}
    for noise in (None, c["noise"]):
        r64, r32 = K.guided_reference(c, torch.float64, noise=noise), K.guided_reference(c, torch.float32, noise=noise)
        for q, v in K.compare(r32, r64, c).items():
            e[q] = max(e.get(q, 0.0), v)
        assert K.idx_mismatches(r32["idx"], r64, 4 * K.TOL["z2"])[0] == 0
    return e


def _reduce_error(R):
    sr = K.reduce_case(R)
    a, b = K.spv_tot_ref(sr, R, 2, K.LAM_SPV), K.spv_tot_ref(sr.double(), R, 2, K.LAM_SPV)
    return max(K.err_rays(a[i], b[i]) for i in range(3))


@pytest.fixture(scope="module")
def measured():
    worst = {}
    def upd(e):
        for q, v in e.items():
            worst[q] = max(worst.get(q, 0.0), v) if v == v else float("nan")
    per_case = {name: _case_errors(c) for name, c in K.CASES.items()}
    for e in per_case.values():
        upd(e)
    for c in K.ALIGN_PAIRS.values():
        upd(_case_errors(c))
    for c in K.GUIDED_CASES.values():
        upd(_guided_errors(c))
    upd({"spv_tot": max(_reduce_error(R) for R in K.REDUCE_R)})
    return worst, per_case


@pytest.mark.parametrize("name", list(K.CASES))
def test_float32_reference_within_half_the_tolerance(name, measured):
    for q, v in measured[1][name].items():
        assert v <= 0.5 * K.TOL[q], f"{name}: {q} float32 vs float64 {v:.2e} > TOL/2 = {0.5 * K.TOL[q]:.1e}"


def _round_up(x):
    p = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / p - 1e-9) * p


def test_tolerances_are_four_times_the_measurement(measured):
    worst = measured[0]
    assert set(worst) == set(K.TOL)
    for q, v in worst.items():
        print(f"{q:10s} measured {v:.2e}  TOL {K.TOL[q]:.0e}")
        assert v <= 0.5 * K.TOL[q]
        assert math.isclose(K.TOL[q], _round_up(4.0 * v), rel_tol=1e-9), f"{q}: TOL {K.TOL[q]:.0e}, 4 x measured = {4 * v:.2e}"
    assert K.EXCLUDED_SHARE == 0.0          # nothing is left out of any comparison: the caps hold trivially


# ------------------------------------------------------------------------------------------------ strength of the comparison
def _last_delta_wrong(z, sigma, rows):
    """composite_ref with the 1e10 step taken one sample early."""
    zz = torch.cat([z[:, :-1], z[:, -2:-1] + 1e10], -1) if z.shape[1] > 1 else z
    o = K.composite_ref(zz, sigma, None, 0.0, rows)
    o["depth"] = (o["weights"] * z).sum(-1)
    return o


def _first_sample_of_lane_1_dropped(c, rows, o):
    """acc without sample cpl, the first one of lane 1: what a wrong lane * cpl + j bound would lose."""
    cpl = (c["S2"] + 63) // 64
    return dict(o, acc=o["acc"] - o["weights"][:, cpl, None] * rows[:, cpl])


def _analytic_dsigma(z, sigma, g, inclusive):
    """The kernels' backward formula, d alpha_s = g_s T_s - (1 / u_s) sum_{k > s} g_k w_k, as torch statements."""
    o = K.composite_ref(z, sigma)
    deltas = torch.cat([z[:, 1:] - z[:, :-1], 1e10 * torch.ones_like(z[:, :1])], -1)
    u = 1 - o["alphas"] + 1e-10
    gw = g * o["weights"]
    suffix = torch.flip(torch.cumsum(torch.flip(gw, [-1]), -1), [-1])
    if not inclusive:
        suffix = suffix - gw
    dad = torch.where(sigma > 0, deltas * torch.exp(-deltas * torch.relu(sigma)), torch.zeros_like(sigma))
    return (g * o["trans"] - suffix / u) * dad


def test_perturbed_references_leave_the_tolerances():
    """Each way the kernels could be wrong, applied to the float32 reference, exceeds TOL against float64 on at least one case
    (and the unperturbed formula does not)."""
    caught = {"dropped_sample": [], "last_delta": [], "suffix_inclusive": [], "noise_without_ray_offset": [], "spv_over_R": []}
    for name, c in K.CASES.items():
        z, idx, o1, o2 = K.inputs(c, torch.float32)
        rows = K.merged_rows(idx, o1, o2)
        ref = K.forward_ref(*K.inputs(c, torch.float64), K.nreg_of(c, spv=True))
        if c["S2"] > 64:
            r64 = K.merged_rows(idx, *K.inputs(c, torch.float64)[2:])
            e = K.compare(_first_sample_of_lane_1_dropped(c, r64, ref), ref, c)
            assert all(e[q] == 0 for q in e if q != "acc")
            if e["acc"] > K.TOL["acc"]:
                caught["dropped_sample"].append(name)
        if c["S2"] > 1:
            wrong = _last_delta_wrong(z, rows[..., 3], rows)
            e = K.compare(wrong, {q: ref[q] for q in wrong}, c)
            if any(e[q] > K.TOL[q] for q in e):
                caught["last_delta"].append(name)
        # backward of sum(w d_w) in the kernels' closed form
        g64 = K.backward_ref(*K.inputs(c, torch.float64), d_w=c["d_w"].double())
        for inclusive in (False, True):
            ds = _analytic_dsigma(z, rows[..., 3], c["d_w"], inclusive)
            rows_g = torch.zeros_like(rows)
            rows_g[..., 3] = ds
            if idx is None:
                got = (rows_g, None)
            else:
                cat = torch.zeros_like(rows_g).scatter_(1, idx.unsqueeze(-1).expand(-1, -1, c["C"]), rows_g)
                got = (cat[:, :c["S1"]], cat[:, c["S1"]:] if o2 is not None else None)
            e = K.err_grads(got, g64)
            if inclusive and e > K.TOL["grad_bwd"]:
                caught["suffix_inclusive"].append(name)
            if not inclusive:
                assert e <= K.TOL["grad_bwd"], f"{name}: the closed-form backward in float32 misses the tolerance ({e:.2e})"
        # noise rows of rays 0.. instead of ray_offset..: the draws of (R + 7) rays, the reference takes rows 7:
        g = torch.Generator().manual_seed(c["seed"])
        draws = torch.randn(c["R"] + 7, c["S2"], generator=g)
        z64, _, a64, b64 = K.inputs(c, torch.float64)
        refn = K.forward_ref(z64, idx, a64, b64, None, draws[7:].double(), K.NOISE_STD)
        e = K.compare(K.forward_ref(z, idx, o1, o2, None, draws[:c["R"]], K.NOISE_STD), refn, c)
        if any(e[q] > K.TOL[q] for q in e):
            caught["noise_without_ray_offset"].append(name)
        if "spv_ray" in ref and c["S2"] > 1:
            wrong = K.spv_tot_ref(ref["spv_ray"].float(), c["R"], 1, K.LAM_SPV)
            if max(K.err_rays(wrong[i], ref["spv_tot"][i]) for i in range(3)) > K.TOL["spv_tot"]:
                caught["spv_over_R"].append(name)
    for k, v in caught.items():
        print(f"{k}: caught by {len(v)} cases, e.g. {v[:3]}")
        assert v, k
    # a sample lost from acc shows in every case that has a lane 1 and all six density patterns (a single ray may be empty there)
    assert {n for n, c in K.CASES.items() if c["S2"] > 64 and c["R"] >= 6} <= set(caught["dropped_sample"])
