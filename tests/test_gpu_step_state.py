"""What the device step state drives, against the references of tests/step_state_cases.py: the in-kernel draws (Philox counter
and key layout, lane and block indexing, Box-Muller) word for word, bn_adam_step / bn_adam_multi in parameters AND moments at
the sizes where their grids wrap, the beta powers (running product, Fn.set_adam_steps, resume), the loss ring, the completion
ticket and the draw counter across slot 63 -> 0 and the 32-bit boundary, eagerly and on graph replay.  Tolerances and the
conditions on every input: tests/test_step_state_cpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_kernel_cases as K  # noqa: E402
import step_state_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U64 = np.uint64
BETAS = (SC.B1, SC.B2)


def _signed(v):
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _state(Fn, seed, step, lr=1e-3):
    st = Fn.new_step_state(DEV, 0, lr)
    st[0], st[1] = _signed(seed), _signed(step)
    return st


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------------ draws
@pytest.mark.parametrize("name", list(SC.DRAW_TABLE))
def test_draws_are_the_reference_words(name):
    """Fn.rng_uniform is the reference bit for bit ((w >> 8) 2^-24 is exact in float32); Fn.rng_normal lies within NORMAL_TOL
    of the float64 Box-Muller of the same words, relative to |x| + sqrt(-2 ln u1), and is finite everywhere - at the planted
    u1 = 2^-24 and u1 = 1 (u1_min, u1_one) too.  The draws leave the state as it is."""
    from brdf_nerf_amd import functions as Fn
    seed, step, stream, n = SC.DRAW_TABLE[name]
    st = _state(Fn, seed, step)
    before = st.clone()
    idx = np.arange(n, dtype=U64)
    u = _np(Fn.rng_uniform(st, stream, n))
    assert np.array_equal(_bits(u), _bits(SC.uniform_ref(seed, step, stream, idx)))
    x = _np(Fn.rng_normal(st, stream, n))
    ref, rad = SC.normal_ref(seed, step, stream, idx)
    assert np.isfinite(x).all()
    e = SC.normal_err(x, ref, rad)
    print(name, f"normal error {e:.2e}")
    assert e <= SC.NORMAL_TOL
    assert torch.equal(st, before)
    if name == "known_answer":
        assert [int(v * 2 ** 24) for v in u[:4].tolist()] == [w >> 8 for w in SC.KNOWN_ANSWERS[0][2]]
    for (entry, elem), want in ((SC.U1_MIN, np.sqrt(48.0 * np.log(2.0))), (SC.U1_ONE, 0.0)):
        if SC.DRAW_TABLE[name] == entry:
            assert rad[elem] == pytest.approx(want, abs=1e-12) and abs(x[elem]) <= want * (1 + SC.NORMAL_TOL)


@pytest.mark.parametrize("R,S,ray_offset", SC.STRAT_HI)
def test_stratified_z_draws_beyond_the_32_bit_index(R, S, ray_offset):
    """bn_rng_* cannot reach the index's high word (n would be 2^34); bn_stratified_z_rng at a ray offset can: its depths are
    those of bn_stratified_z on the reference uniforms of elements (ray_offset + r) S + s, bit for bit."""
    from brdf_nerf_amd import functions as Fn
    st = _state(Fn, SC.STRAT_SEED, SC.STRAT_STEP)
    g = torch.Generator().manual_seed(R)
    nf = torch.stack([0.1 + torch.rand(R, generator=g), 2.0 + torch.rand(R, generator=g)], -1).contiguous().to(DEV)
    idx = np.arange(R * S, dtype=U64) + U64(ray_offset * S)
    u = torch.from_numpy(SC.uniform_ref(SC.STRAT_SEED, SC.STRAT_STEP, SC.RNG_COARSE, idx)).reshape(R, S).to(DEV)
    got = Fn.stratified_z_rng(None, S, st, ray_offset=ray_offset, near_far=nf, stream_id=SC.RNG_COARSE)
    assert torch.equal(got, Fn.stratified_z(nf[:, :1], nf[:, 1:], u))
    low = torch.from_numpy(SC.uniform_ref(SC.STRAT_SEED, SC.STRAT_STEP, SC.RNG_COARSE, idx & U64(0xFFFFFFFF))).reshape(R, S).to(DEV)
    assert not torch.equal(got, Fn.stratified_z(nf[:, :1], nf[:, 1:], low))


def test_merged_composite_noise_beyond_the_32_bit_index():
    """bn_merged_composite_forward under in-kernel noise whose element index (ray + ray_offset) S2 + s crosses 2^32 inside
    ray 0: K.forward_ref fed the float64 reference normals of those elements, at K.TOL."""
    from brdf_nerf_amd import functions as Fn
    c = SC.noise_hi_case()
    st = _state(Fn, SC.NOISE_HI_SEED, SC.NOISE_HI_STEP)
    dev = lambda t: None if t is None else t.to(DEV).contiguous()
    want = ("alphas", "trans", "weights", "depth", "acc", "wsum", "var")
    noise = Fn.noise_arg(st, K.NOISE_STD, SC.RNG_NOISE_MERGED, ray_offset=SC.NOISE_HI_OFFSET)
    got = Fn.merged_composite_forward(dev(c["z_all"]), dev(c["idx"]), dev(c["out1"]), dev(c["out2"]), want=want, noise=noise)
    x, _ = SC.normal_ref(SC.NOISE_HI_SEED, SC.NOISE_HI_STEP, SC.RNG_NOISE_MERGED, SC.noise_hi_index(c))
    ref = K.forward_ref(*K.inputs(c, torch.float64), None, torch.from_numpy(x), K.NOISE_STD)
    e = K.compare(got, ref, c)
    print({q: f"{v:.1e}" for q, v in e.items()})
    for q, v in e.items():
        assert v <= K.TOL[q], (q, v)


# ------------------------------------------------------------------------------------------------ bn_adam_step
GUARD = 8


def _guarded(a):
    """The array on the device with GUARD sentinel elements behind it (the buffer stays 16-byte aligned)."""
    buf = torch.full((a.shape[0] + GUARD,), -7.25, dtype=torch.float32, device=DEV)
    buf[:a.shape[0]] = torch.from_numpy(a)
    return buf


def _assert_adam(tag, got, ref):
    e = SC.adam_errs(got, ref)
    print(tag, {q: f"{v:.2e}" for q, v in e.items()})
    for q, v in e.items():
        assert v <= SC.ADAM_TOL[q], f"{tag}: {q} error {v:.2e} > {SC.ADAM_TOL[q]:.1e}"


@pytest.mark.parametrize("n", SC.ADAM_SIZES)
def test_adam_step_parameters_and_moments(n):
    """Every launch of ADAM_STEP_CASES[n] (steps 1, 2, 1000; weight decay and gradient scale in every combination) from the
    device's own float32 state, copied out before the launch: p, m and v element-wise within ADAM_TOL of one float64 update.
    The gradient and the elements behind the buffers stay as they were."""
    from brdf_nerf_amd import functions as Fn
    p, m, v, scale = SC.adam_state(n, 100 + n)
    P, M, V = _guarded(p), _guarded(m), _guarded(v)
    for i, (t, (wd, gs)) in enumerate(SC.ADAM_STEP_CASES[n]):
        g = SC.adam_grad(scale, 200 + n, i)
        G = _guarded(g)
        p0, m0, v0 = _np(P[:n]), _np(M[:n]), _np(V[:n])
        ref = SC.adam_update(p0, g, m0, v0, SC.lr_of(i), t, wd, gs)
        Fn.adam_step(P[:n], G[:n], M[:n], V[:n], t, SC.lr_of(i), betas=BETAS, eps=SC.EPS, weight_decay=wd, grad_scale=gs)
        _assert_adam(f"n={n} launch {i} step {t} wd {wd} gs {gs}", {"p": _np(P[:n]), "m": _np(M[:n]), "v": _np(V[:n])}, ref)
        assert np.array_equal(_bits(_np(G[:n])), _bits(g))
        for B in (P, M, V, G):
            assert bool((B[n:] == -7.25).all())


# ------------------------------------------------------------------------------------------------ bn_adam_multi and the state
class _Multi:
    """One flat buffer of a MULTI_LAYOUTS entry on the device with its step state, and the check of one launch."""

    def __init__(self, Fn, layout, rng_step0):
        self.Fn, self.layout, self.L = Fn, layout, SC.MULTI_LAYOUTS[layout]
        p, m, v, self.scale = SC.multi_state(layout)
        self.P, self.M, self.V = (torch.from_numpy(a).to(DEV) for a in (p, m, v))
        self.G = torch.zeros_like(self.P)
        self.state = _state(Fn, 5, rng_step0)
        Fn.state_views(self.state)[3].copy_(torch.from_numpy(SC.ring_sentinel()))
        self.counts = [0, 0, 0, 0]
        self.cur = rng_step0
        self.sums = {}                                    # rng_step -> (float64 sum, bound) of its partials

    def stage(self, launch):
        """Gradient, learning rate and loss partials of launch `launch` into the device buffers."""
        self.g = SC.adam_grad(self.scale, 400, launch)
        self.parts = SC.loss_partials(self.L["total"], launch)
        self.lr = SC.lr_of(launch)
        self.G.copy_(torch.from_numpy(self.g))
        self.Fn.state_views(self.state)[1].fill_(self.lr)
        self.Fn.state_loss_partials(self.state).copy_(torch.from_numpy(self.parts))

    def launch(self, act, wd, gs, zg):
        self.Fn.adam_multi(self.P, self.G, self.M, self.V, self.L["groups"], act, self.state, betas=BETAS, eps=SC.EPS, weight_decay=wd,
                           grad_scale=gs, zero_grad=zg)

    def step(self, tag, act, wd, gs, zg, run):
        """Copy the state out, `run()` the launch (eager, or a graph replay of one with the same arguments), compare."""
        p0, m0, v0, s0 = _np(self.P), _np(self.M), _np(self.V), _np(self.state)
        mask, ref, after = SC.multi_expect(self.layout, act, wd, gs, self.counts, p0, self.g, m0, v0, self.lr)
        run()
        p1, m1, v1, g1, s1 = _np(self.P), _np(self.M), _np(self.V), _np(self.G), _np(self.state)
        _assert_adam(tag, {k: a[mask] for k, a in (("p", p1), ("m", m1), ("v", v1))}, {k: a[mask] for k, a in ref.items()})
        # inactive groups, empty groups and the slack: bitwise untouched, the gradient included
        for a1, a0 in ((p1, p0), (m1, m0), (v1, v0), (g1, self.g)):
            assert np.array_equal(_bits(a1)[~mask], _bits(a0)[~mask]), tag
        # zero_grad: cleared exactly where read, left in place when off
        assert np.array_equal(_bits(g1)[mask], np.zeros(int(mask.sum()), np.int32) if zg else _bits(self.g)[mask]), tag
        self._check_state(tag, s0, s1, act, after)
        self.counts = after

    def _check_state(self, tag, s0, s1, act, after):
        i0, i1 = s0.view(np.int32), s1.view(np.int32)
        f1, d1 = s1.view(np.float32), s1.view(np.float64)
        cur = self.cur
        assert int(s1.view(np.uint64)[1]) == cur + 1, tag                          # rng_step, as the u64 it is
        assert i1[5] == 0, tag                                                     # done
        assert i1[6:10].tolist() == after, tag                                     # step counts: active groups only
        pw = d1[40:48]
        for gi in range(4):
            for k, b in enumerate(BETAS):
                want = SC.beta_pow(b, after[gi])
                assert abs(pw[4 * k + gi] / want - 1.0) <= SC.POW_RTOL, (tag, gi, k)
                if not act[gi]:
                    assert s1[40 + 4 * k + gi] == s0[40 + 4 * k + gi], tag        # bitwise
        assert not i1[128:192].any(), tag                                          # the 64 partials: exactly +0
        total, bound = float(self.parts.astype(np.float64).sum()), 64 * 2.0 ** -24 * float(np.abs(self.parts.astype(np.float64)).sum())
        slot = cur % SC.RING_SLOTS
        ring0, ring1 = i0[16:80], i1[16:80]
        assert abs(float(f1[16 + slot]) - total) <= bound, (tag, float(f1[16 + slot]), total, bound)
        others = np.arange(SC.RING_SLOTS) != slot
        assert np.array_equal(ring1[others], ring0[others]), tag
        # nothing else of the 1 KB moved: seed, lr, noise_std, the reserved words
        same = np.ones(256, dtype=bool)
        same[2:4] = same[5] = False
        same[6:10] = same[16:80] = same[80:96] = same[128:192] = False
        assert np.array_equal(i1[same], i0[same]), tag
        self.sums[cur] = (total, bound)
        self.cur = cur + 1


@pytest.mark.parametrize("layout,rng_step0,launches", SC.MULTI_RUNS)
def test_adam_multi_groups_ring_and_ticket(layout, rng_step0, launches):
    """Four groups of one flat buffer - "wrap": a group of 2^19 + 1028 elements that wraps the 512-workgroup grid, "small": one
    workgroup, with an empty active group - an inactive group between active ones, a group that joins at the third launch,
    weight decay / gradient scale / zero_grad changing per launch, the learning rate through the state.  After EVERY launch:
    p, m, v of the active groups within ADAM_TOL of the float64 update of the state before it; everything else of the four
    buffers bitwise as it was; the state's step counts, beta powers (float32(beta)^count to 1e-12), rng_step, ticket, the
    partial sums cleared, their float64 sum in ring slot rng_step % 64 within 64 x 2^-24 x sum |partial|, every other slot and
    every other word of the state bitwise unchanged.  rng_step starts at 0, at 60 (slot 63 -> 0) and at 2^32 - 3."""
    from brdf_nerf_amd import functions as Fn
    mu = _Multi(Fn, layout, rng_step0)
    for i in range(launches):
        act = SC.multi_active(layout, i)
        wd, gs, zg = SC.multi_args(i)
        mu.stage(i)
        mu.step(f"{layout} launch {i}", act, wd, gs, zg, lambda: mu.launch(act, wd, gs, zg))
    join = SC.MULTI_LAYOUTS[layout]["joins"]
    assert mu.counts[join] == launches - SC.JOIN_LAUNCH and mu.counts.count(0) == 1
    assert mu.cur == rng_step0 + launches


def test_adam_multi_graph_replay_reads_the_state():
    """One captured bn_adam_multi launch (a single kernel: no parallel branches), replayed 70 times with the gradient, the
    learning rate and the partial sums rewritten in place between replays: parameters and moments follow the float64 reference
    step by step - so bias corrections and learning rate come from the device state, not from the capture - and the ring ends
    up holding the last 64 sums."""
    from brdf_nerf_amd import functions as Fn
    mu = _Multi(Fn, "small", 0)
    wd, gs, zg = SC.GRAPH_ARGS
    mu.stage(0)
    mu.step("eager", SC.GRAPH_ACTIVE, wd, gs, zg, lambda: mu.launch(SC.GRAPH_ACTIVE, wd, gs, zg))
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        mu.launch(SC.GRAPH_ACTIVE, wd, gs, zg)
    assert mu.cur == 1 and int(Fn.state_views(mu.state)[0]) == 1                   # the capture itself launched nothing
    for i in range(1, SC.GRAPH_REPLAYS + 1):
        mu.stage(i)
        mu.step(f"replay {i}", SC.GRAPH_ACTIVE, wd, gs, zg, graph.replay)
    ring = _np(Fn.state_views(mu.state)[3]).astype(np.float64)
    last = range(mu.cur - SC.RING_SLOTS, mu.cur)
    assert mu.cur == SC.GRAPH_REPLAYS + 1 and len(last) == SC.RING_SLOTS
    for t in last:
        total, bound = mu.sums[t]
        assert abs(ring[t % SC.RING_SLOTS] - total) <= bound, t
    assert mu.counts == [SC.GRAPH_REPLAYS + 1, SC.GRAPH_REPLAYS + 1, 0, SC.GRAPH_REPLAYS + 1]


def _kernel_bias_corrections(state_np):
    """(bc1, bc2_sqrt) per group as bn_adam_multi forms them from the state's powers, in float32."""
    pw = state_np.view(np.float64)[40:48]
    b1, b2 = (np.float64(np.float32(b)) for b in BETAS)
    return np.float32(1.0 - pw[:4] * b1), np.sqrt(np.float32(1.0 - pw[4:] * b2))


def test_beta_powers_and_resume():
    """After s = 1, 10, 1000 launches the state's beta powers are float32(beta)^s (exact rational arithmetic, rounded once) to
    1e-12, and Fn.set_adam_steps writes the same values to the same bound.  A state set to step s, then one launch on the
    buffers of that moment, leaves what launch s + 1 of the uninterrupted run leaves: bit for bit where the float32 bias
    corrections formed from the two states' powers are equal (they are), and within ADAM_TOL of the float64 update in any
    case."""
    from brdf_nerf_amd import functions as Fn
    act, (wd, gs, zg) = SC.GRAPH_ACTIVE, SC.GRAPH_ARGS
    mu = _Multi(Fn, "small", 0)
    for i in range(max(SC.POW_STEPS) + 1):
        mu.stage(i)
        s = i
        if s in SC.POW_STEPS:
            assert mu.counts == [s, s, 0, s]
            run_pw = _np(mu.state).view(np.float64)[40:48]
            resumed = _state(Fn, 5, mu.cur, mu.lr)
            Fn.set_adam_steps(resumed, mu.counts, BETAS)
            set_pw = _np(resumed).view(np.float64)[40:48]
            for gi in range(4):
                for k, b in enumerate(BETAS):
                    want = SC.beta_pow(b, mu.counts[gi])
                    assert abs(run_pw[4 * k + gi] / want - 1.0) <= SC.POW_RTOL, (s, gi, k, "running product")
                    assert abs(set_pw[4 * k + gi] / want - 1.0) <= SC.POW_RTOL, (s, gi, k, "set_adam_steps")
            assert _np(resumed).view(np.int32)[6:10].tolist() == mu.counts
            same_bc = all(np.array_equal(a, b) for a, b in zip(_kernel_bias_corrections(_np(mu.state)), _kernel_bias_corrections(_np(resumed))))
            # one launch from the resumed state on copies of the buffers, with this launch's gradient
            p0, m0, v0 = _np(mu.P), _np(mu.M), _np(mu.V)
            P2, M2, V2, G2 = mu.P.clone(), mu.M.clone(), mu.V.clone(), mu.G.clone()
            Fn.adam_multi(P2, G2, M2, V2, mu.L["groups"], act, resumed, betas=BETAS, eps=SC.EPS, weight_decay=wd, grad_scale=gs, zero_grad=zg)
            mask, ref, after = SC.multi_expect("small", act, wd, gs, mu.counts, p0, mu.g, m0, v0, mu.lr)
            _assert_adam(f"resumed at {s}", {k: _np(a)[mask] for k, a in (("p", P2), ("m", M2), ("v", V2))}, {k: a[mask] for k, a in ref.items()})
            assert _np(resumed).view(np.int32)[6:10].tolist() == after
        mu.launch(act, wd, gs, zg)
        mu.counts = [c + a for c, a in zip(mu.counts, act)]
        mu.cur += 1
        if s in SC.POW_STEPS:
            assert same_bc, s
            for a, b in ((mu.P, P2), (mu.M, M2), (mu.V, V2), (mu.G, G2)):
                assert torch.equal(a, b), s
    assert int(_np(mu.state).view(np.uint64)[1]) == mu.cur


# ------------------------------------------------------------------------------------------------ bn_count_nonfinite
def test_count_nonfinite_across_its_grid_stride():
    """n = 2^20 + 3: 513 workgroups, every thread strides over 8 or 9 elements.  One NaN and one Inf in the first pass, in the
    second pass and on the last two elements; the counts are ADDED to what the counters held."""
    from brdf_nerf_amd import functions as Fn
    n, one = SC.NONFINITE_N, SC.NONFINITE_PASS
    x = torch.from_numpy(np.random.default_rng(3).standard_normal(n).astype(np.float32))
    nan_at, inf_at = (5, one + 77, n - 1), (one - 1, 2 * one - 3, n - 2)
    x[list(nan_at)] = float("nan")
    x[list(inf_at)] = torch.tensor([float("inf"), float("-inf"), float("inf")])
    counts = torch.tensor([1000, 7], dtype=torch.int64, device=DEV)
    out = Fn.count_nonfinite(x.to(DEV), counts)
    assert out.data_ptr() == counts.data_ptr() and counts.tolist() == [1003, 10]
    assert Fn.count_nonfinite(x[:one].to(DEV)).tolist() == [1, 1]
