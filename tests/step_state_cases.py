"""Shared by tests/test_step_state_cpu.py and tests/test_gpu_step_state.py: plain references of what the device step state
(bn_step_state, include/brdfnerf_hip.h) drives - the in-kernel draws, the two Adam entry points, the loss ring - and the fixed
inputs and tolerances of their comparison with the kernels.

Draws.  Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) in numpy uint64
integer arithmetic, written from the published algorithm: a round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to
(hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key is bumped by the Weyl constants between rounds.  The
step state's layout on top of it: counter = (index lo, index hi, stream, step lo), key = (seed lo, seed hi ^ step hi), where
`index` is the BLOCK index: uniform element i is word i & 3 of block i >> 2, normal element i is made of words 2 (i & 1) and
2 (i & 1) + 1 of block i >> 1.

Adam.  One update of (p, m, v) from float32 inputs as torch.optim.Adam states it, with the betas, eps, weight decay, gradient
scale and learning rate as the float32 values a C ABI with `float` arguments receives, promoted to double.

Every tolerance below is 4 x an error measured on the CPU from the references alone (test_step_state_cpu.py repeats each
measurement and asserts that it stays within a quarter of the constant), never from what a kernel gave.
"""
from fractions import Fraction

import numpy as np

import ray_kernel_cases as K

U64 = np.uint64
_MASK = U64(0xFFFFFFFF)
_32 = U64(32)
_M0, _M1 = U64(0xD2511F53), U64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85

# draw streams of one step (include/brdfnerf_hip.h)
RNG_COARSE, RNG_GUIDED, RNG_GUIDED_TARGET, RNG_NOISE_COARSE, RNG_NOISE_MERGED, RNG_SUN = 1, 2, 3, 4, 5, 6

# (counter; key -> output) of Philox4x32-10, the known-answer vectors of the Random123 distribution
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


# ------------------------------------------------------------------------------------------------ Philox4x32-10
def philox_scalar(counter, key):
    """One block in Python integers: counter (c0, c1, c2, c3), key (k0, k1) -> 4 words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox(c0, c1, c2, c3, k0, k1):
    """The same over arrays: uint64 arrays (or scalars) holding 32-bit words, broadcast against each other -> 4 uint64 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(a, dtype=U64) for a in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                                  # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + U64(_W0)) & _MASK, (k1 + U64(_W1)) & _MASK
    return c0, c1, c2, c3


def state_words(seed, step, stream, block):
    """The 4 words [4][n] of blocks `block` (uint64 array) of stream `stream` at (seed, step): the step state's counter / key
    layout.  seed, step, stream: Python integers or arrays that broadcast against `block`."""
    u = lambda a: np.asarray(a, dtype=U64)
    seed, step, block = u(seed), u(step), u(block)
    return np.stack(philox(block & _MASK, block >> _32, u(stream) & _MASK, step & _MASK,
                           seed & _MASK, (seed >> _32) ^ (step >> _32)))


def uniform_ref(seed, step, stream, index):
    """float32 uniforms in [0, 1) of elements `index`: exact, (w >> 8) 2^-24 has 24 bits."""
    index = np.asarray(index, dtype=U64)
    w = state_words(seed, step, stream, index >> U64(2))
    sel = np.take_along_axis(w, (index & U64(3)).astype(np.int64)[None], 0)[0]
    return ((sel >> U64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def normal_words(seed, step, stream, index):
    """(w0 >> 8, w1 >> 8) of normal elements `index`, as int64."""
    index = np.asarray(index, dtype=U64)
    w = state_words(seed, step, stream, index >> U64(1))
    q = ((index & U64(1)) * U64(2)).astype(np.int64)[None]
    return ((np.take_along_axis(w, q, 0)[0] >> U64(8)).astype(np.int64), (np.take_along_axis(w, q + 1, 0)[0] >> U64(8)).astype(np.int64))


def box_muller(a, b, dtype=np.float64):
    """x = sqrt(-2 ln u1) cos(2 pi u2), u1 = (a + 1) 2^-24 in (0, 1], u2 = b 2^-24 in [0, 1), every operation in `dtype`.
    -> (x, r = sqrt(-2 ln u1))."""
    t = dtype
    u1, u2 = (a + 1).astype(t) * t(2.0 ** -24), b.astype(t) * t(2.0 ** -24)
    r = np.sqrt(t(-2.0) * np.log(u1))
    return r * np.cos(t(2.0 * np.pi) * u2), r


def normal_ref(seed, step, stream, index):
    """float64 standard normals of elements `index`, and their radii (the scale of the comparison)."""
    return box_muller(*normal_words(seed, step, stream, index))


def normal_err(got, x, r):
    """max |got - x| / (|x| + r); a zero error counts as 0 on any scale (u1 = 1: x = r = 0)."""
    e = np.abs(np.asarray(got, dtype=np.float64) - x)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(e == 0, 0.0, e / (np.abs(x) + r))))


# |float32 evaluation - float64| / (|x| + r) of box_muller over every entry of DRAW_TABLE: measured 3.69e-07 (the float32
# product 2 pi u2 carries half an ulp of 6.28 into the cosine).  x 4: the device's logf and cospif are good to 1 ulp each.
NORMAL_TOL = 2e-6

# (seed, step, stream, n).  Steps and seeds are written to the state as they are (u64); n = 4099 is a multiple of neither 4 (the
# uniform block) nor 256 (the workgroup).
_SEED_HI = 0x9E3779B97F4A7C15                     # both halves non-zero, bit 63 set
_CANCEL = 0xABCD1234
N_DRAWS = 4099
DRAW_TABLE = {
    "known_answer": (0, 0, 0, 16),
    "seed_hi": (_SEED_HI, 7, RNG_COARSE, N_DRAWS),
    "seed_lo_only": (_SEED_HI & 0xFFFFFFFF, 7, RNG_COARSE, N_DRAWS),
    "step_2p32m1": (1234, 2 ** 32 - 1, RNG_GUIDED, N_DRAWS),
    "step_2p32": (1234, 2 ** 32, RNG_GUIDED, N_DRAWS),
    "step_2p32p1": (1234, 2 ** 32 + 1, RNG_GUIDED, N_DRAWS),
    "step_0": (1234, 0, RNG_GUIDED, N_DRAWS),       # = step 2^32 with its high word dropped
    "step_1": (1234, 1, RNG_GUIDED, N_DRAWS),
    **{f"stream_{s}": (99, 3, s, N_DRAWS) for s in range(1, 7)},
    "stream_max": (99, 3, 0xFFFFFFFF, N_DRAWS),
    "stream3_step5": (99, 5, 3, N_DRAWS),            # with stream_5 (stream 5, step 3): the two counter words swapped
    "hi_cancel": ((_CANCEL << 32) | 0x55, (_CANCEL << 32) | 9, RNG_SUN, N_DRAWS),          # key word 1 = 0
    "hi_cancel_next": ((_CANCEL << 32) | 0x55, ((_CANCEL + 1) << 32) | 9, RNG_SUN, N_DRAWS),
    "hi_cancel_off": (0x55, 9, RNG_SUN, N_DRAWS),    # the same key and counter as hi_cancel by construction: equal draws
}
# entries that must differ from each other pairwise although they share most of their words
DISTINCT = (("seed_hi", "seed_lo_only"), ("step_2p32", "step_0"), ("step_2p32p1", "step_1"), ("step_2p32m1", "step_2p32"),
            ("stream_5", "stream3_step5"), ("hi_cancel", "hi_cancel_next"), ("stream_1", "stream_2"))


def find_u1_edge(target, seed, stream, n, step0, budget):
    """The first (step, element) with step in [step0, step0 + budget), element < n, whose Box-Muller word w0 >> 8 equals
    `target` (0: u1 = 2^-24, the largest radius; 0xFFFFFF: u1 = 1, radius 0), or None.  budget x n / 2 blocks are generated."""
    idx = np.arange(n, dtype=U64)
    chunk = 512
    for s0 in range(step0, step0 + budget, chunk):
        steps = np.arange(s0, min(s0 + chunk, step0 + budget), dtype=U64)[:, None]
        a, _ = normal_words(seed, steps, stream, np.broadcast_to(idx, (steps.shape[0], n)))
        hit = np.argwhere(a == target)
        if hit.size:
            return int(steps[hit[0][0], 0]), int(hit[0][1])
    return None


# Found by find_u1_edge(target, 2024, RNG_NOISE_COARSE, 4096, 0, 16384) - a budget of 2^25 blocks per target, both hit inside
# it - as (seed, step, stream, n) with the element that holds the word:
U1_MIN = ((2024, 1919, RNG_NOISE_COARSE, 4096), 2778)          # w0 >> 8 = 0:        u1 = 2^-24, r = sqrt(48 ln 2) = 5.768
U1_ONE = ((2024, 666, RNG_NOISE_COARSE, 4096), 3952)           # w0 >> 8 = 0xFFFFFF: u1 = 1, x = r = 0
DRAW_TABLE["u1_min"], DRAW_TABLE["u1_one"] = U1_MIN[0], U1_ONE[0]

# bn_stratified_z_rng beyond the 32-bit draw index: element (ray_offset + r) S + s.  (R, S, ray_offset): the first starts at
# 2^32 + 2 (a block's third word), the second crosses 2^32 inside the call.
STRAT_HI = ((67, 6, 715827883), (67, 6, 715827882))
STRAT_SEED, STRAT_STEP = 0x1234567800000321, 2 ** 32 + 5

# bn_merged_composite_forward under in-kernel noise beyond the 32-bit index: ray 0 of the case crosses 2^32
# (66076419 x 65 = 2^32 - 61), every later ray lies above it.
NOISE_HI_OFFSET = 66076419
NOISE_HI_SEED, NOISE_HI_STEP = 77, 2 ** 32 + 1


def noise_hi_case():
    return K.build_case(65, "even", "5", 7, 7100, first_pattern=1)


def noise_hi_index(case):
    R, S2 = case["R"], case["S2"]
    return (np.arange(R, dtype=U64)[:, None] + U64(NOISE_HI_OFFSET)) * U64(S2) + np.arange(S2, dtype=U64)[None]


# ------------------------------------------------------------------------------------------------ Adam
B1, B2, EPS = 0.9, 0.999, 1e-8
WEIGHT_DECAYS = (0.0, 1e-2)
GRAD_SCALES = (1.0, 0.5, 2.0 ** -13)
COMBOS = tuple((wd, gs) for wd in WEIGHT_DECAYS for gs in GRAD_SCALES)
F32_MIN_NORMAL = float(np.finfo(np.float32).tiny)


def f32(x):
    """A Python float as the float32 a C `float` argument receives, back in double."""
    return float(np.float32(x))


def beta_pow(beta, t):
    """float32(beta)^t, exactly rational, rounded once to double."""
    return float(Fraction(f32(beta)) ** int(t))


def lr_of(launch):
    """The learning rate written to the state before launch `launch` (it changes every step)."""
    return f32(1e-3 * 0.7 ** launch)


def adam_update(p, g, m, v, lr, t, wd, gs, dtype=np.float64, b1=B1, b2=B2, eps=EPS, pow_of=beta_pow):
    """Step t (>= 1) of torch.optim.Adam on float32 arrays, evaluated in `dtype`:
        g' = g gs + wd p;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2
        p' = p - lr / (1 - b1^t) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
    The bias corrections are formed in double from the float32 betas (as the host, or the device from the state's powers, does)
    and rounded to `dtype`.  -> dict p, m, v, and in float64 the magnitudes that entered each: sp, sm, sv, and g' as gp."""
    t_ = dtype
    b1, b2, eps, wd, gs, lr = [t_(f32(x)) for x in (b1, b2, eps, wd, gs, lr)]
    bc1, bc2_sqrt = t_(1.0 - pow_of(b1, t)), np.sqrt(t_(1.0 - pow_of(b2, t)))
    p, g, m, v = [np.asarray(a, dtype=np.float32).astype(t_) for a in (p, g, m, v)]
    one = t_(1.0)
    gp = g * gs + wd * p
    m1 = b1 * m + (one - b1) * gp
    v1 = b2 * v + (one - b2) * gp * gp
    denom = np.sqrt(v1) / bc2_sqrt + eps
    upd = (lr / bc1) * (m1 / denom)
    o = {"p": p - upd, "m": m1, "v": v1}
    if t_ is np.float64:
        o.update(gp=gp, sm=np.abs(b1 * m) + np.abs((one - b1) * gp), sv=b2 * v + (one - b2) * gp * gp, sp=np.abs(p) + np.abs(upd))
    return o


def adam_errs(got, ref):
    """{q: max |got[q] - ref[q]| / ref[s<q>]} for q in p, m, v; a zero error counts as 0, a NaN as infinite."""
    out = {}
    for q in ("p", "m", "v"):
        e = np.abs(np.asarray(got[q], dtype=np.float64) - ref[q])
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(e == 0, 0.0, e / ref["s" + q])
        out[q] = float(np.max(np.where(np.isnan(r), np.inf, r))) if r.size else 0.0
    return out


# max over every launch of ADAM_STEP_CASES and MULTI_RUNS of |float32 update - float64 update| / magnitude, both from the same
# float32 state (measured in test_step_state_cpu.py), x 4 for FMA contraction and the kernel's association of
# lr / bc1 * (m / denom), rounded up to two significant digits:
ADAM_TOL = {
    "m": 7.8e-7,      # measured 1.93e-07
    "v": 1.5e-6,      # measured 3.61e-07
    "p": 1.1e-6,      # measured 2.65e-07
}


def adam_state(n, seed, lo_first=True):
    """p, m, v [n] float32, the per-element gradient magnitudes `scale` (log-uniform over 2e-12 .. 1e6, the extremes on the
    first two elements) and signs.  Moments are non-zero and of the size the gradients give them.

    The bounds on m and p are relative to the magnitudes that enter a SUM (|b1 m| + |(1 - b1) g'|; |p| + |update|), so they mean
    something only where the sums before them do not cancel: g gs against wd p in g', b1 m against (1 - b1) g' in m' (whose
    relative error is the update's).  Each element therefore keeps ONE sign for its parameter, moments and gradients - either
    sign, at random - and |p| >= 0.1, so that no launch of a walk takes a parameter through zero.  One element in 16 starts at
    p = 0 exactly, where the bound on p is a bound on the update alone; those have |g| >= 500, far above the wd p they meet
    on later launches.  test_step_state_cpu.py asserts on every launch that neither sum loses more than half."""
    r = np.random.default_rng(seed)
    scale = 10.0 ** r.uniform(np.log10(2e-12), 6.0, n)
    zero_p = r.random(n) < 1.0 / 16
    if lo_first and n:
        scale[0] = 1e6
        scale[1:2] = 2e-12
        zero_p[0:2] = (True, False)[:n]
    scale[zero_p] = np.maximum(scale[zero_p], 10.0 ** r.uniform(3.0, 6.0, n)[zero_p])
    sign = np.where(r.random(n) < 0.5, -1.0, 1.0)
    p = (sign * 10.0 ** r.uniform(-1.0, 0.0, n) * ~zero_p).astype(np.float32)
    m = (sign * scale * r.uniform(0.05, 0.5, n)).astype(np.float32)
    v = (scale ** 2 * r.uniform(0.25, 1.0, n)).astype(np.float32)
    return p, m, v, scale * sign


def adam_grad(scale, seed, launch):
    """Gradients of magnitude |scale| x [0.5, 1): 1e-12 .. 1e6, the sign of `scale`, every 16th element on average exactly 0
    (and one chosen by the launch always)."""
    n = scale.shape[0]
    r = np.random.default_rng([seed, launch])
    g = scale * r.uniform(0.5, 1.0, n)
    g[r.random(n) < 1.0 / 16] = 0.0
    if n > 2:
        g[2 + launch % (n - 2)] = 0.0
    return g.astype(np.float32)


# bn_adam_step: n -> the (step argument, (weight_decay, grad_scale)) launches, run one after the other on the same buffers.
# Grid: min(ceil(n / 1024), 2048) workgroups of 256 threads x 4 elements; n = 2^21 + 7 wraps it once, its second pass is one
# vector chunk (elements 2^21 .. 2^21 + 3) and the scalar tail (the last three).
ADAM_STEPS = (1, 2, 1000)
ADAM_SIZES = (1, 3, 4, 5, 1023, 1027, 2 ** 21 + 7)
_BIG_COMBOS = (5, 1, 3)          # one combination per step at the large size: (1e-2, 2^-13), (0, 0.5), (1e-2, 1)
ADAM_STEP_CASES = {n: tuple((t, COMBOS[i]) for j, t in enumerate(ADAM_STEPS) for i in (range(6) if n < 2048 else _BIG_COMBOS[j:j + 1]))
                   for n in ADAM_SIZES}


def adam_step_reference(n, on_launch=None):
    """Walk the launches of ADAM_STEP_CASES[n] on the CPU: the float32 evaluation carries the state, the float64 one restarts
    from it every launch.  -> the largest adam_errs entries.  on_launch(launch, args, state, grad, ref64) sees every launch."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    p, m, v, scale = adam_state(n, 100 + n)
    for i, (t, (wd, gs)) in enumerate(ADAM_STEP_CASES[n]):
        g = adam_grad(scale, 200 + n, i)
        ref = adam_update(p, g, m, v, lr_of(i), t, wd, gs)
        if on_launch is not None:
            on_launch(i, (t, wd, gs), (p, m, v), g, ref)
        got = adam_update(p, g, m, v, lr_of(i), t, wd, gs, np.float32)
        for q, e in adam_errs(got, ref).items():
            worst[q] = max(worst[q], e)
        p, m, v = got["p"], got["m"], got["v"]
    return worst


# bn_adam_multi: four groups of one flat buffer (BN_ADAM_MAX_GROUPS = 4), 4 .. 12 slack elements before, between and after.
# Grid: min(ceil(largest active group / 1024), 512) workgroups; 2^19 + 1024 + 4 elements wrap the 512 once, the second pass
# fills one workgroup and one thread of the next.  `joins`: the group that turns active at the third launch.
WRAP_N = 2 ** 19 + 1024 + 4
MULTI_LAYOUTS = {
    "wrap": dict(groups=((4, 8), (16, 276), (280, 280 + WRAP_N), (280 + WRAP_N + 12, 280 + WRAP_N + 272)),
                 active=(1, 0, 1, 0), joins=3, total=280 + WRAP_N + 276, workgroups=512),
    "small": dict(groups=((4, 264), (268, 268), (272, 276), (280, 284)),
                  active=(1, 1, 0, 0), joins=3, total=288, workgroups=1),
}
JOIN_LAUNCH = 2
# (layout, first rng_step, launches)
MULTI_RUNS = (("small", 0, 4), ("wrap", 0, 4), ("small", 60, 8), ("wrap", 60, 8), ("small", 2 ** 32 - 3, 8), ("wrap", 2 ** 32 - 3, 8))
RING_SLOTS = 64


def multi_active(layout, launch):
    L = MULTI_LAYOUTS[layout]
    return tuple(int(a or (gi == L["joins"] and launch >= JOIN_LAUNCH)) for gi, a in enumerate(L["active"]))


def multi_args(launch):
    """(weight_decay, grad_scale, zero_grad) of launch `launch`."""
    wd, gs = COMBOS[(launch * 5 + 1) % 6]
    return wd, gs, launch % 2 == 0


def multi_state(layout):
    L = MULTI_LAYOUTS[layout]
    return adam_state(L["total"], 300 + L["total"] % 97, lo_first=False)


def loss_partials(seed, launch):
    """64 partial sums of mixed sign and magnitude (1e-6 .. 1e3), float32."""
    r = np.random.default_rng([seed, launch, 17])
    return (np.where(r.random(RING_SLOTS) < 0.5, -1.0, 1.0) * 10.0 ** r.uniform(-6, 3, RING_SLOTS)).astype(np.float32)


def ring_sentinel():
    return (-1000.0 - np.arange(RING_SLOTS)).astype(np.float32)


def multi_expect(layout, act, wd, gs, counts, p, g, m, v, lr):
    """What one launch must leave, from the float32 buffers before it: float64 p, m, v (+ scales) on the elements of the
    active groups (`mask`), the step counts after it.  counts: the groups' step counts before it."""
    L = MULTI_LAYOUTS[layout]
    mask = np.zeros(L["total"], dtype=bool)
    ref = {k: np.zeros(L["total"]) for k in ("p", "m", "v", "sp", "sm", "sv", "gp")}
    for gi, (lo, hi) in enumerate(L["groups"]):
        if act[gi] and hi > lo:
            mask[lo:hi] = True
            o = adam_update(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], lr, counts[gi] + 1, wd, gs)
            for k in ref:
                ref[k][lo:hi] = o[k]
    return mask, ref, [c + int(bool(a)) for c, a in zip(counts, act)]


def multi_reference(layout, launches, on_launch=None):
    """The CPU walk of one MULTI_RUNS entry, as adam_step_reference."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    p, m, v, scale = multi_state(layout)
    counts = [0, 0, 0, 0]
    for i in range(launches):
        g = adam_grad(scale, 400, i)
        wd, gs, _ = multi_args(i)
        mask, ref, after = multi_expect(layout, multi_active(layout, i), wd, gs, counts, p, g, m, v, lr_of(i))
        if on_launch is not None:
            on_launch(i, mask, ref, p, g, m, v)
        for gi, (lo, hi) in enumerate(MULTI_LAYOUTS[layout]["groups"]):
            if after[gi] != counts[gi] and hi > lo:
                got = adam_update(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], lr_of(i), counts[gi] + 1, wd, gs, np.float32)
                for q, e in adam_errs(got, {k: a[lo:hi] for k, a in ref.items()}).items():
                    worst[q] = max(worst[q], e)
                p[lo:hi], m[lo:hi], v[lo:hi] = got["p"], got["m"], got["v"]
        counts = after
    return worst


POW_STEPS = (1, 10, 1000)
POW_RTOL = 1e-12          # a running product of 1000 doubles is off by at most 1000 x 2^-53 = 1.1e-13

# the captured launch of the replay test: one signature for every replay
GRAPH_ACTIVE, GRAPH_ARGS, GRAPH_REPLAYS = (1, 1, 0, 1), (1e-2, 0.5, True), 70

# bn_count_nonfinite: ceil(n / 2048) = 513 workgroups of 256 threads, each thread strides over 8 or 9 elements
NONFINITE_N = 2 ** 20 + 3
NONFINITE_PASS = 513 * 256
