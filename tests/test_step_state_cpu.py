"""tests/step_state_cases.py held to what is published and to itself, without a GPU: the Philox known answers, the two forms
of the generator, the layout facts the draw table relies on, the measured tolerance constants, every condition placed on an
input of tests/test_gpu_step_state.py, and - by mutating the REFERENCE - that each comparison of the GPU test moves past its
tolerance for the mistakes a kernel could make (test_mutation_*)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_kernel_cases as K  # noqa: E402
import step_state_cases as SC  # noqa: E402

U64 = np.uint64


def _idx(n):
    return np.arange(n, dtype=U64)


# ------------------------------------------------------------------------------------------------ draws
def test_philox_known_answers():
    for counter, key, out in SC.KNOWN_ANSWERS:
        assert SC.philox_scalar(counter, key) == out
        assert tuple(int(w) for w in SC.philox(*counter, *key)) == out


def test_scalar_and_vector_forms_agree():
    r = np.random.default_rng(1)
    words = r.integers(0, 2 ** 32, (64, 6), dtype=np.uint64)
    words[0], words[1, :4], words[2, 4:] = 0xFFFFFFFF, 0, 0
    vec = np.stack(SC.philox(*words.T))
    for i, w in enumerate(words.tolist()):
        assert tuple(int(x) for x in vec[:, i]) == SC.philox_scalar(w[:4], w[4:])
    # and the state's layout on top: counter = (index lo, index hi, stream, step lo), key = (seed lo, seed hi ^ step hi)
    seed, step, stream = 0x0123456789ABCDEF, 0xFEDCBA9876543210, 0xDEADBEEF
    for block in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3):
        want = SC.philox_scalar((block & 0xFFFFFFFF, block >> 32, stream, step & 0xFFFFFFFF),
                                (seed & 0xFFFFFFFF, (seed >> 32) ^ (step >> 32)))
        assert tuple(int(x) for x in SC.state_words(seed, step, stream, np.array([block], dtype=U64))[:, 0]) == want


def test_uniforms_and_normals_take_their_words_as_documented():
    seed, step, stream = 5, 6, 7
    w = SC.state_words(seed, step, stream, _idx(8))                   # [4][8]
    u = SC.uniform_ref(seed, step, stream, _idx(32))
    assert u.dtype == np.float32
    for i in range(32):
        assert float(u[i]) == (int(w[i & 3, i >> 2]) >> 8) * 2.0 ** -24
    a, b = SC.normal_words(seed, step, stream, _idx(16))
    x, rad = SC.normal_ref(seed, step, stream, _idx(16))
    for i in range(16):
        assert (int(a[i]), int(b[i])) == (int(w[2 * (i & 1), i >> 1]) >> 8, int(w[2 * (i & 1) + 1, i >> 1]) >> 8)
        u1, u2 = (int(a[i]) + 1) * 2.0 ** -24, int(b[i]) * 2.0 ** -24
        assert x[i] == np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    # the first known answer through the table's first entry
    kseed, kstep, kstream, _ = SC.DRAW_TABLE["known_answer"]
    assert [float(v) * 2 ** 24 for v in SC.uniform_ref(kseed, kstep, kstream, _idx(4))] == [o >> 8 for o in SC.KNOWN_ANSWERS[0][2]]


def test_draw_table_covers_what_it_claims():
    T = SC.DRAW_TABLE
    assert T["known_answer"][:3] == (0, 0, 0)
    assert T["seed_hi"][0] >> 32 and T["seed_hi"][0] >> 63
    assert {T[k][1] for k in ("step_2p32m1", "step_2p32", "step_2p32p1")} == {2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1}
    assert {v[2] for v in T.values()} >= {1, 2, 3, 4, 5, 6, 0xFFFFFFFF}
    s, t = T["hi_cancel"][:2]
    assert s >> 32 and (s >> 32) == (t >> 32)                          # the high words cancel in the key
    assert T["hi_cancel_next"][1] >> 32 == (t >> 32) + 1
    assert SC.N_DRAWS % 4 and SC.N_DRAWS % 256 and SC.N_DRAWS > 256
    u = {k: SC.uniform_ref(*v[:3], _idx(v[3])) for k, v in T.items()}
    for a, b in SC.DISTINCT:
        assert float(np.mean(u[a] == u[b])) < 1e-3, (a, b)              # 24-bit words: equal by chance once in 2^24
    assert np.array_equal(u["hi_cancel"], u["hi_cancel_off"])           # the layout folds step hi into the key: documented
    for v in u.values():
        assert v.min() >= 0.0 and v.max() < 1.0


def test_reference_normals_are_standard_normal():
    """2^20 reference normals: mean, variance, skewness, excess kurtosis and the correlation of the two normals of a block
    within 5 standard errors of a standard normal's."""
    n = 2 ** 20
    x, _ = SC.normal_ref(2024, 3, SC.RNG_NOISE_MERGED, _idx(n))
    se = 1.0 / np.sqrt(n)
    assert abs(x.mean()) < 5 * se
    assert abs(x.var() - 1.0) < 5 * np.sqrt(2.0) * se
    assert abs((x ** 3).mean()) < 5 * np.sqrt(15.0) * se
    assert abs((x ** 4).mean() - 3.0) < 5 * np.sqrt(96.0) * se
    assert abs((x[0::2] * x[1::2]).mean()) < 5 * np.sqrt(2.0) * se
    assert abs((x[:-2:2] * x[2::2]).mean()) < 5 * np.sqrt(2.0) * se
    u = SC.uniform_ref(2024, 3, SC.RNG_COARSE, _idx(n)).astype(np.float64)
    assert abs(u.mean() - 0.5) < 5 * se / np.sqrt(12.0) and abs(u.var() - 1.0 / 12) < 5 * se / np.sqrt(180.0)


def _all_normal_words():
    parts = [SC.normal_words(*v[:3], _idx(v[3])) for v in SC.DRAW_TABLE.values()]
    parts.append(tuple(w.reshape(-1) for w in SC.normal_words(SC.NOISE_HI_SEED, SC.NOISE_HI_STEP, SC.RNG_NOISE_MERGED,
                                                               SC.noise_hi_index(SC.noise_hi_case()))))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def test_normal_tolerance_is_four_times_the_float32_error():
    a, b = _all_normal_words()
    x, r = SC.box_muller(a, b)
    x32, _ = SC.box_muller(a, b, np.float32)
    assert x32.dtype == np.float32
    e = SC.normal_err(x32, x, r)
    print(f"float32 Box-Muller vs float64 over {a.size} words: {e:.3e}")
    assert SC.NORMAL_TOL / 8 < e <= SC.NORMAL_TOL / 4
    assert np.isfinite(x).all() and np.isfinite(x32).all()


def test_u1_edges_are_planted_in_the_table():
    for (entry, elem), target, rad in ((SC.U1_MIN, 0, np.sqrt(48.0 * np.log(2.0))), (SC.U1_ONE, 0xFFFFFF, 0.0)):
        seed, step, stream, n = entry
        assert entry in SC.DRAW_TABLE.values() and elem < n
        a, _ = SC.normal_words(seed, step, stream, _idx(n))
        assert int(a[elem]) == target
        x, r = SC.normal_ref(seed, step, stream, _idx(n))
        assert np.isfinite(x).all() and abs(r[elem] - rad) < 1e-12
        # the bounded search finds it again, and nothing in the steps just before it
        assert SC.find_u1_edge(target, seed, stream, n, step - 8, 16) == (step, elem)


def test_high_index_cases_lie_beyond_32_bits():
    (R, S, off), (R2, S2, off2) = SC.STRAT_HI
    assert off * S >= 2 ** 32 and (off * S) % 4 != 0 and off % 2 == 1
    assert off2 * S2 < 2 ** 32 < (off2 + R2) * S2
    idx = SC.noise_hi_index(SC.noise_hi_case())
    assert int(idx.min()) < 2 ** 32 < int(idx[0].max()) and int(idx[1:].min()) > 2 ** 32
    # a dropped high word would show: the draws of the truncated indices differ
    for R_, S_, off_ in SC.STRAT_HI:
        i = _idx(R_ * S_) + U64(off_ * S_)
        hi, lo = SC.uniform_ref(SC.STRAT_SEED, SC.STRAT_STEP, SC.RNG_COARSE, i), SC.uniform_ref(SC.STRAT_SEED, SC.STRAT_STEP, SC.RNG_COARSE, i & U64(0xFFFFFFFF))
        assert float(np.mean((hi == lo)[i >= U64(2 ** 32)])) < 0.01


def _noise_hi_refs():
    c = SC.noise_hi_case()
    a, b = SC.normal_words(SC.NOISE_HI_SEED, SC.NOISE_HI_STEP, SC.RNG_NOISE_MERGED, SC.noise_hi_index(c))
    x64, _ = SC.box_muller(a, b)
    x32, _ = SC.box_muller(a, b, np.float32)
    z, idx, o1, o2 = K.inputs(c, torch.float64)
    ref = lambda noise: K.forward_ref(z, idx, o1, o2, None, torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float64)), K.NOISE_STD)
    return c, x64, x32, ref


def test_noise_case_beyond_32_bits_is_well_conditioned():
    """The float64 reference fed float32 normals - the float64 ones rounded, and the float32 evaluation of Box-Muller - stays
    within HALF of K.TOL of the one fed the float64 normals: the other half is the kernel's."""
    c, x64, x32, ref = _noise_hi_refs()
    want = ref(x64)
    for name, noise in (("rounded", x64.astype(np.float32)), ("float32 Box-Muller", x32)):
        e = K.compare(ref(noise), want, c)
        print(name, {q: f"{v:.1e}" for q, v in e.items()})
        for q, v in e.items():
            assert v <= 0.5 * K.TOL[q], (name, q, v)


# ------------------------------------------------------------------------------------------------ Adam
def _torch_adam(p, grads, m, v, lrs, t0, wd, b1, b2):
    """torch.optim.Adam in float64 from a given state."""
    P = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.Adam([P], lr=lrs[0], betas=(b1, b2), eps=SC.f32(SC.EPS), weight_decay=wd)
    opt.state[P] = dict(step=torch.tensor(float(t0)), exp_avg=torch.from_numpy(m.astype(np.float64)),
                        exp_avg_sq=torch.from_numpy(v.astype(np.float64)))
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        P.grad = torch.from_numpy(g)
        opt.step()
    return P.detach().numpy(), opt.state[P]["exp_avg"].numpy(), opt.state[P]["exp_avg_sq"].numpy()


@pytest.mark.parametrize("wd", SC.WEIGHT_DECAYS)
@pytest.mark.parametrize("t", SC.ADAM_STEPS)
def test_adam_reference_is_torch_optim_adam(t, wd):
    """One float64 update of the reference against torch.optim.Adam (float64, the float32 betas as its betas, the scaled
    gradient as its gradient) from the same state at step t - 1."""
    n, gs = 1027, 0.5
    p, m, v, scale = SC.adam_state(n, 9)
    g = SC.adam_grad(scale, 9, t)
    ref = SC.adam_update(p, g, m, v, SC.lr_of(1), t, wd, gs)
    tp, tm, tv = _torch_adam(p, [g.astype(np.float64) * gs], m, v, [SC.lr_of(1)], t - 1, SC.f32(wd), SC.f32(SC.B1), SC.f32(SC.B2))
    e = SC.adam_errs({"p": tp, "m": tm, "v": tv}, ref)
    print(e)
    assert max(e.values()) < 1e-13


def test_float32_betas_against_double_betas_over_1000_steps():
    """How far the contract "the betas are the float32 values a `float` argument holds" moves a run from Adam with the
    double betas 0.9 / 0.999: 1000 steps of random gradients, float64 on both sides, lr 1e-3, parameters of size 1.

    Measured: a single update differs by up to 2.77e-7 of the largest update (1.4e-3), which is 4.65 ulp of a float32 update of
    that size; after 1000 steps the parameters have drifted by 8.74e-9, which is 104 ulp of such an update and 0.147 ulp of a
    float32 parameter of size 1.  So the drift is NOT far below one float32 ulp of the update:
    1 - beta2 differs by 1.3e-5 relative between the two (0.00099998713 against 0.001), and the bias correction cancels only
    the part of that which is common to all steps.  It stays below the rounding of the parameter the updates are added to.
    The contract is therefore stated in the header (the float32 betas ARE the betas; a float64 torch.optim.Adam run with
    betas=(0.9, 0.999) is reproduced to that drift, not to rounding), and every reference here takes the float32 values.
    Asserted: what follows from the betas alone - every weight beta2^k, k <= 1000, of the second moment moves by at most
    k |d beta2| / beta2 relative, so |drift| <= steps x lr x 1000 x |d beta2| / beta2 - and the measured figures to a factor 2."""
    STEP_REL, STEP_ULP, DRIFT_ABS, DRIFT_ULP_UPD, DRIFT_ULP_PAR = 2.77e-7, 4.65, 8.74e-9, 104, 0.147
    n, steps, lr = 4096, 1000, 1e-3
    r = np.random.default_rng(11)
    P = [r.standard_normal(n), None]
    P[1] = P[0].copy()
    M, V = [np.zeros(n), np.zeros(n)], [np.zeros(n), np.zeros(n)]
    betas = ((SC.f32(SC.B1), SC.f32(SC.B2)), (SC.B1, SC.B2))
    scale = 10.0 ** r.uniform(-3, 3, n)
    largest = step_diff = 0.0
    for t in range(1, steps + 1):
        g = r.standard_normal(n) * scale
        upd = [None, None]
        for k, (b1, b2) in enumerate(betas):
            M[k] = b1 * M[k] + (1 - b1) * g
            V[k] = b2 * V[k] + (1 - b2) * g * g
            upd[k] = lr / (1 - b1 ** t) * M[k] / (np.sqrt(V[k]) / np.sqrt(1 - b2 ** t) + 1e-8)
            P[k] = P[k] - upd[k]
        largest = max(largest, float(np.abs(upd[1]).max()))
        step_diff = max(step_diff, float(np.abs(upd[0] - upd[1]).max()))
    drift = float(np.abs(P[0] - P[1]).max())
    ulp_update, ulp_param = largest * 2.0 ** -24, 2.0 ** -24
    got = (step_diff / largest, step_diff / ulp_update, drift, drift / ulp_update, drift / ulp_param)
    print("largest update %.3e; STEP_REL %.3e STEP_ULP %.3g DRIFT_ABS %.3e DRIFT_ULP_UPD %.3g DRIFT_ULP_PAR %.3g" % ((largest,) + got))
    assert drift <= steps * lr * 1000 * abs(SC.f32(SC.B2) - SC.B2) / SC.B2
    for g_, want in zip(got, (STEP_REL, STEP_ULP, DRIFT_ABS, DRIFT_ULP_UPD, DRIFT_ULP_PAR)):
        assert 0.5 * want <= g_ <= 2 * want
    assert drift < 0.5 * ulp_param


def _check_inputs(state, g, ref, wd, gs):
    p, m, v = state
    assert all(a.dtype == np.float32 for a in (p, m, v, g))
    assert np.isfinite(p).all() and np.isfinite(g).all()
    assert (m != 0).all() and (v > 0).all()                                             # moments are non-zero
    tiny, big = SC.F32_MIN_NORMAL, float(np.finfo(np.float32).max)
    gp = ref["gp"]
    nz = gp != 0
    # no square leaves the float32 normal range: g'^2, (1 - b2) g'^2 in either association, the new v
    for sq in (gp * gp, (1.0 - SC.f32(SC.B2)) * gp * gp, ref["v"]):
        assert (sq[nz] >= tiny).all() and (sq < big).all()
    assert (np.abs((1.0 - SC.f32(SC.B2)) * gp)[nz] >= tiny).all() and (np.abs(ref["m"]) >= tiny).all()
    assert (np.abs(p[p != 0]) >= tiny).all() and (np.abs(g[g != 0]) >= tiny).all() and (v >= tiny).all() and (np.abs(m) >= tiny).all()
    assert all(np.isfinite(ref[k]).all() for k in ref)
    assert (ref["sm"] > 0).all() and (ref["sv"] > 0).all()
    _check_no_cancellation(p, g, ref, wd, gs)


def _check_no_cancellation(p, g, ref, wd, gs):
    """Neither g' = g gs + wd p nor m' = b1 m + (1 - b1) g' loses more than half of what enters it, and no parameter
    changes sign (adam_state)."""
    assert (np.abs(ref["gp"]) >= 0.5 * (np.abs(g.astype(np.float64) * SC.f32(gs)) + np.abs(SC.f32(wd) * p.astype(np.float64)))).all()
    assert (np.abs(ref["m"]) >= 0.5 * ref["sm"]).all()
    assert (ref["p"] * p >= 0).all()


def test_adam_inputs_meet_their_conditions_and_tolerances_are_measured():
    """Every launch of the GPU test, walked on the CPU: the conditions on its inputs, and the float32-vs-float64 error that
    ADAM_TOL is four times of."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    mags, zeros = [], 0

    def merge(w):
        for q in worst:
            worst[q] = max(worst[q], w[q])

    for n in SC.ADAM_SIZES:
        seen = set()

        def on_launch(i, args, state, g, ref, seen=seen):
            nonlocal zeros
            t, wd, gs = args
            seen.add((wd, gs))
            _check_inputs(state, g, ref, wd, gs)
            mags.append(np.abs(g[g != 0]))
            zeros += int((g == 0).sum())
        merge(SC.adam_step_reference(n, on_launch))
        assert n > 2048 or seen == set(SC.COMBOS)
    a = np.concatenate(mags)
    assert a.min() < 2e-12 and a.min() >= 1e-12 and 5e5 <= a.max() <= 1e6 and zeros > 0
    # (the first rng_step of a run does not enter its Adam inputs, and a run of 4 launches is the start of the run of 8)
    for layout, launches in sorted({(l, max(n for l2, _, n in SC.MULTI_RUNS if l2 == l)) for l, _, _ in SC.MULTI_RUNS}):
        L = SC.MULTI_LAYOUTS[layout]
        p, m, v, scale = SC.multi_state(layout)
        assert (m != 0).all() and (v > 0).all()
        touched = np.zeros(L["total"], dtype=int)

        def on_launch(i, mask, ref, p, g, m, v, touched=touched):
            touched += mask
            wd, gs, _ = SC.multi_args(i)
            _check_no_cancellation(p[mask], g[mask], {k: a[mask] for k, a in ref.items()}, wd, gs)
            assert (ref["gp"][mask] ** 2 * (1.0 - SC.f32(SC.B2)) >= SC.F32_MIN_NORMAL)[ref["gp"][mask] != 0].all()
            assert (ref["v"][mask] >= SC.F32_MIN_NORMAL).all() and (ref["v"][mask] < 3e38).all()
        merge(SC.multi_reference(layout, launches, on_launch))
        # the layout: multiples of 4, slack before, between and after, the inactive group and the slack never stepped
        edges = [0] + [x for lo_hi in L["groups"] for x in lo_hi] + [L["total"]]
        assert all(x % 4 == 0 for x in edges) and all(b - a >= 4 for a, b in zip(edges[0::2], edges[1::2]))
        for gi, (lo, hi) in enumerate(L["groups"]):
            want = launches if L["active"][gi] else (launches - SC.JOIN_LAUNCH if gi == L["joins"] else 0)
            assert (touched[lo:hi] == want).all()
        assert touched.sum() == sum(int((touched[lo:hi]).sum()) for lo, hi in L["groups"])
        most = max(hi - lo for gi, (lo, hi) in enumerate(L["groups"]) if SC.multi_active(layout, 0)[gi])
        assert min(max(-(-most // 1024), 1), 512) == L["workgroups"]
    assert SC.WRAP_N > 512 * 1024 and (SC.WRAP_N - 512 * 1024) % 1024 == 4
    assert {SC.multi_args(i)[:2] for i in range(8)} == set(SC.COMBOS) and {SC.multi_args(i)[2] for i in range(2)} == {True, False}
    print("float32 update vs float64 update:", {q: f"{e:.3e}" for q, e in worst.items()})
    for q, e in worst.items():
        assert SC.ADAM_TOL[q] / 8 < e <= SC.ADAM_TOL[q] / 4, (q, e)


def test_beta_powers_reference():
    for b in (SC.B1, SC.B2):
        fb = float(np.float32(b))
        for s in SC.POW_STEPS:
            run = 1.0
            for _ in range(s):
                run *= fb
            assert abs(run / SC.beta_pow(b, s) - 1.0) < SC.POW_RTOL / 5
    # the discrepancy the state's powers must not carry: the double beta's power is 1.3e-5 away at s = 1000
    assert abs(SC.B2 ** 1000 / SC.beta_pow(SC.B2, 1000) - 1.0) > 1e-5


def test_set_adam_steps_writes_the_float32_betas_powers():
    """The host side of a resume: the powers Fn.set_adam_steps writes are those bn_adam_multi's running product reaches."""
    from brdf_nerf_amd import functions as Fn
    st = torch.zeros(128, dtype=torch.int64)
    Fn.set_adam_steps(st, [1, 10, 1000], (SC.B1, SC.B2))
    assert st.view(torch.int32)[6:10].tolist() == [1, 10, 1000, 0]
    pw = st.view(torch.float64)[40:48].tolist()
    for k, b in enumerate((SC.B1, SC.B2)):
        for gi, s in enumerate((1, 10, 1000, 0)):
            assert abs(pw[4 * k + gi] / SC.beta_pow(b, s) - 1.0) <= SC.POW_RTOL, (b, s)


def test_nonfinite_size_wraps_its_grid():
    n = SC.NONFINITE_N
    assert -(-n // 2048) * 256 == SC.NONFINITE_PASS < 4096 * 256 and 2 * SC.NONFINITE_PASS < n - 1


def test_loss_partials_are_mixed():
    p = SC.loss_partials(1, 0)
    assert p.dtype == np.float32 and (p > 0).any() and (p < 0).any() and np.abs(p).max() / np.abs(p).min() > 1e6
    assert not np.array_equal(p, SC.loss_partials(1, 1))
    assert len(set(SC.ring_sentinel().tolist())) == SC.RING_SLOTS


# ------------------------------------------------------------------------------------------------ mutations of the reference
# Each stands for a mistake a kernel could make; the unmutated reference plays the kernel.  The comparison of the GPU test,
# applied to the pair, must fail.
def test_mutation_draw_indexing():
    seed, step, stream, n = SC.DRAW_TABLE["seed_hi"]
    i = _idx(n)
    u = SC.uniform_ref(seed, step, stream, i)
    w = SC.state_words(seed, step, stream, i >> U64(2))
    lane = lambda sel: ((np.take_along_axis(w, sel.astype(np.int64)[None], 0)[0] >> U64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    assert np.array_equal(lane(i & U64(3)), u)
    assert not np.array_equal(lane((i + U64(1)) & U64(3)), u)                                   # lane off by one
    assert not np.array_equal(SC.uniform_ref(seed, step, stream, i + U64(4)), u)                # block off by one
    assert not np.array_equal(SC.uniform_ref(seed, step, stream, (i >> U64(1)) << U64(1)), u)   # index >> 1 for the uniform block
    x, r = SC.normal_ref(seed, step, stream, i)
    for mutated in (SC.normal_ref(seed, step, stream, i ^ U64(1))[0],                           # the pair of a block swapped
                    SC.normal_ref(seed, step, stream, i + U64(2))[0],                           # block off by one
                    SC.box_muller(*SC.normal_words(seed, step, stream, i)[::-1])[0]):           # u1 and u2 exchanged
        assert SC.normal_err(mutated, x, r) > 1e3 * SC.NORMAL_TOL
    # a Box-Muller error that keeps the moments: sine for cosine
    a, b = SC.normal_words(seed, step, stream, i)
    sine = np.sqrt(-2.0 * np.log((a + 1) * 2.0 ** -24)) * np.sin(2.0 * np.pi * b * 2.0 ** -24)
    assert SC.normal_err(sine, x, r) > 1e3 * SC.NORMAL_TOL
    # u1 = a 2^-24 instead of (a + 1) 2^-24: infinite at the planted word, and beyond the bound elsewhere
    (entry, elem) = SC.U1_MIN
    a, b = SC.normal_words(*entry[:3], _idx(entry[3]))
    with np.errstate(divide="ignore", invalid="ignore"):
        assert not np.isfinite(SC.box_muller(a - 1, b)[0][elem])


def test_mutation_draw_words():
    ref = lambda name, **kw: SC.uniform_ref(*[kw.get(k, v) for k, v in zip(("seed", "step", "stream"), SC.DRAW_TABLE[name][:3])],
                                            _idx(SC.DRAW_TABLE[name][3]))
    lo = 0xFFFFFFFF
    for name, (seed, step, stream, n) in SC.DRAW_TABLE.items():
        u = ref(name)
        if seed >> 32 and not name.startswith("hi_cancel"):
            assert not np.array_equal(ref(name, seed=seed & lo), u), name                       # dropped high word of the seed
        if step >> 32:
            assert not np.array_equal(ref(name, step=step & lo), u), name                       # ... of the step
        if stream != step & lo:
            assert not np.array_equal(ref(name, stream=step & lo, step=(step & ~lo) | stream), u), name    # stream and step swapped
    # hi_cancel: dropping BOTH high words is the one change the layout cannot show; dropping either one shows
    seed, step, stream, n = SC.DRAW_TABLE["hi_cancel"]
    assert not np.array_equal(ref("hi_cancel", seed=seed & lo), ref("hi_cancel"))
    assert not np.array_equal(ref("hi_cancel", step=step & lo), ref("hi_cancel"))
    # dropped index >> 32 (the stratified-z and the noise case, see test_high_index_cases_lie_beyond_32_bits for the former)
    c, x64, _, fwd = _noise_hi_refs()
    i = SC.noise_hi_index(c)
    trunc, _ = SC.normal_ref(SC.NOISE_HI_SEED, SC.NOISE_HI_STEP, SC.RNG_NOISE_MERGED, i & U64(lo))
    e = K.compare(fwd(trunc), fwd(x64), c)
    assert e["alphas"] > 100 * K.TOL["alphas"] and e["weights"] > 100 * K.TOL["weights"]


def _mutated_errs(n, launch_of, mutate):
    """adam_errs of a float32 'kernel' that differs from the update by `mutate(out, p, g, m, v, args)` at one launch."""
    res = {}

    def on_launch(i, args, state, g, ref):
        if i == launch_of:
            p, m, v = state
            t, wd, gs = args
            out = SC.adam_update(p, g, m, v, SC.lr_of(i), t, wd, gs, np.float32)
            mutate(out, p, g, m, v, (i, t, wd, gs))
            res.update(SC.adam_errs(out, ref))
    SC.adam_step_reference(n, on_launch)
    return res


def _fails(errs):
    return any(errs[q] > SC.ADAM_TOL[q] for q in errs)


def _traversal_mutations(n, ranges):
    """For every launch of size n and every ("skip" | "repeat", lo, hi): does the comparison fail for a float32 'kernel' that
    leaves [lo, hi) untouched, or updates it twice?  (One walk; only the slice is compared: nothing else differs.)"""
    verdicts = []

    def on_launch(i, args, state, g, ref):
        p, m, v = state
        t, wd, gs = args
        for kind, lo, hi in ranges:
            sl = slice(lo, hi)
            if kind == "skip":
                got = {"p": p[sl], "m": m[sl], "v": v[sl]}
            else:
                once = SC.adam_update(p[sl], g[sl], m[sl], v[sl], SC.lr_of(i), t, wd, gs, np.float32)
                got = SC.adam_update(once["p"], g[sl], once["m"], once["v"], SC.lr_of(i), t, wd, gs, np.float32)
            verdicts.append(((i, kind, lo, hi), _fails(SC.adam_errs(got, {k: a[sl] for k, a in ref.items()}))))
        clean = SC.adam_update(p[-8:], g[-8:], m[-8:], v[-8:], SC.lr_of(i), t, wd, gs, np.float32)
        assert not _fails(SC.adam_errs(clean, {k: a[-8:] for k, a in ref.items()}))
    SC.adam_step_reference(n, on_launch)
    return verdicts


def test_mutation_adam_traversal():
    n = 2 ** 21 + 7
    first = 2048 * 256 * 4                                                                     # one pass of the grid
    verdicts = _traversal_mutations(n, (("skip", first, first + 4),                            # the second pass's vector chunk skipped
                                        ("skip", 1024, 2048),                                  # a workgroup's chunk skipped
                                        ("repeat", first - 1024, first),                       # the wrap repeats the last chunk
                                        ("skip", n - 3, n - 2),                                # the tail starts one element late
                                        ("skip", n - 1, n),                                    # ... or ends one early
                                        ("repeat", first + 3, first + 4)))                     # the tail starts one element early
    assert len(verdicts) == 18 and all(f for _, f in verdicts), [k for k, f in verdicts if not f]
    for small in (1, 3, 5, 1023, 1027):
        verdicts = _traversal_mutations(small, (("skip", small - 1, small), ("repeat", small - 1, small)))
        assert all(f for _, f in verdicts), (small, [k for k, f in verdicts if not f])
    # adam_multi's wrapping group: the second pass (1028 elements) skipped, or the last chunk of the first pass repeated
    lo, hi = SC.MULTI_LAYOUTS["wrap"]["groups"][2]
    seen = []

    def on_launch(i, mask, ref, p, g, m_, v_):
        wd, gs, _ = SC.multi_args(i)
        for kind, sl in (("skip", slice(lo + 512 * 1024, hi)), ("repeat", slice(lo + 512 * 1024 - 1024, lo + 512 * 1024)),
                         ("skip", slice(hi - 4, hi))):
            cnt = i + 1
            once = SC.adam_update(p[sl], g[sl], m_[sl], v_[sl], SC.lr_of(i), cnt, wd, gs, np.float32) if kind == "repeat" else None
            got = ({"p": p[sl], "m": m_[sl], "v": v_[sl]} if kind == "skip" else
                   SC.adam_update(once["p"], g[sl], once["m"], once["v"], SC.lr_of(i), cnt, wd, gs, np.float32))
            seen.append(_fails(SC.adam_errs(got, {k: a[sl] for k, a in ref.items()})))
    SC.multi_reference("wrap", 1, on_launch)
    assert len(seen) == 3 and all(seen)


def test_mutation_adam_terms():
    n = 1027

    def with_args(**kw):
        def f(out, p, g, m, v, a):
            i, t, wd, gs = a
            alt = SC.adam_update(p, g, m, v, kw.get("lr", SC.lr_of(i)), kw.get("t", t), kw.get("wd", wd), kw.get("gs", gs), np.float32,
                                 pow_of=kw.get("pow_of", SC.beta_pow))
            out.update(alt)
        return f
    for launch, (t, (wd, gs)) in enumerate(SC.ADAM_STEP_CASES[n]):
        if wd:
            assert _fails(_mutated_errs(n, launch, with_args(wd=0.0)))                          # weight decay dropped
            assert _fails(_mutated_errs(n, launch, with_args(wd=wd * gs))) or gs == 1.0         # ... or scaled with the gradient
        if gs != 1.0:
            assert _fails(_mutated_errs(n, launch, with_args(gs=1.0)))                          # gradient scale dropped
        assert _fails(_mutated_errs(n, launch, with_args(lr=SC.lr_of(launch + 1))))            # a stale learning rate
        if t == 2:
            assert _fails(_mutated_errs(n, launch, with_args(t=1)))                            # a stale beta power
    # decoupled (AdamW) instead of L2 weight decay
    def adamw(out, p, g, m, v, a):
        i, t, wd, gs = a
        alt = SC.adam_update(p, g, m, v, SC.lr_of(i), t, 0.0, gs, np.float32)
        alt["p"] = alt["p"] - np.float32(SC.lr_of(i) * wd) * p
        out.update(alt)
    assert _fails(_mutated_errs(n, 3, adamw)) and SC.ADAM_STEP_CASES[n][3][1][0] > 0
    # at step 1000 the parameters no longer see a power that is off by the double-vs-float32 beta (1.3e-5): the state's powers
    # are therefore compared directly, to POW_RTOL
    assert abs(SC.B2 ** 1000 / SC.beta_pow(SC.B2, 1000) - 1.0) > 1e6 * SC.POW_RTOL
