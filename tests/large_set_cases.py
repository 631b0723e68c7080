"""A few live lattice points in a large set of silent ones: the point-split machinery of the weight-gradient phase at
the point counts it is tuned for, still held to the exact float64 reference of tests/lattice_cases.py.

Exactness on the dyadic lattice limits the number of points that CONTRIBUTE to a sum (lattice_cases.N_MAX = 1100), not
the number of rows of a call.  embed() places the first B lattice points of a case as LIVE rows (their d_out is
case.coef) in a set of N >> B rows; every other row is a FILLER, a copy of a lattice point of the same case with
d_out = 0 on every channel.  A filler's forward values are real (non-zero activations, masks and adjoint deltas in every
stash), every seed the backward forms for it is exactly zero (0 x act'; the normalisations' Jacobians are finite on
lattice points, the eps floor gives 0 / sqrt(eps)), so its products are exact zeros in every mode and the fp16 loss scales
see the live seeds alone.  The gradient of the N rows IS the gradient of the B live points, with the reference, the
bit-equality classes and the bounds of test_gpu_lattice._ref(name, B) - while the N rows are cut into as many splits,
slabs, rounds and reduce iterations as a real call (tests/test_gpu_large_sets.py; the premise is asserted in float64 by
tests/test_large_sets_cpu.py).

split_counts() RESTATES the split policy of the library (the source lines are named in its comments).  It chooses the
sizes and labels the tests; no comparison depends on it.  A change of the split policy must update the restatement (the
regime test of tests/test_large_sets_cpu.py then says which named regime a size no longer reaches); if it goes stale,
only the labels are lost.

Split counts by the restatement, per (case, dtype, size): Mpad, tiles of the job list, point splits of the tile launch
(16-bit: 256 x 256 tiles, fp32: 128 x 128), splits of the skinny launch, rounds of the 256 CUs (16-bit), and the
remainders the kernels branch on (n%8: wgrad_reduce_kernel's scalar tail; t*n%8: wgrad256_kernel's XCD remap rounds its
grid up; skinny 57 .. 63: some thread groups of skinny_reduce_kernel take the 64-stride loop, some only the tail).

  size  case                  dtype  Mpad    tiles  wgrad n_split (points each)  n%8  t*n%8  skinny n_split (points each)  rounds
  S1    lambert_F64_L8        fp32   15360   10       60 (  256)               4    0       120 (  128)                 1
  S1    lambert_F64_L8        16-bit 15360   10       24 (  640)               0    0        60 (  256)                 1
  S1    rpv_an_F128_L4        fp32   15360   12       60 (  256)               4    0       120 (  128)                 1
  S1    rpv_an_F128_L4        16-bit 15360   12       20 (  768)               4    0        60 (  256)                 1
  S1    rpv_anlr_F256_L8      fp32   15360   72       27 (  576)               3    0       120 (  128)                 1
  S1    rpv_anlr_F256_L8      16-bit 15360   22       11 ( 1408)               3    2        60 (  256)                 1
  S1    rpv_an_F512_L8        fp32   15360   272       7 ( 2208)               7    0       120 (  128)                 1
  S1    rpv_an_F512_L8        16-bit 15360   72        3 ( 5120)               3    0        60 (  256)                 1
  S1    viewdir_beta_F192_L8  fp32   15360   38       48 (  320)               0    0       120 (  128)                 1
  S1    viewdir_beta_F192_L8  16-bit 15360   13       19 (  832)               3    7        60 (  256)                 1
  S2    lambert_F64_L8        fp32   163840  10      197 (  832)               5    2       256 (  640)                 1
  S2    lambert_F64_L8        16-bit 163840  10       25 ( 6592)               1    2       256 (  640)                 1
  S2    rpv_an_F128_L4        fp32   163840  12      166 (  992)               6    0       256 (  640)                 1
  S2    rpv_an_F128_L4        16-bit 163840  12       21 ( 7808)               5    4       256 (  640)                 1
  S3    lambert_F64_L8        fp32   327744  10      201 ( 1632)               1    2       244 ( 1344)                 1
  S3    lambert_F64_L8        16-bit 327808  10       51 ( 6464)               3    6       233 ( 1408)                 2
  S3    rpv_an_F128_L4        fp32   327744  12      168 ( 1952)               0    0       244 ( 1344)                 1
  S3    rpv_an_F128_L4        16-bit 327808  12       42 ( 7808)               2    0       233 ( 1408)                 2
  S3    viewdir_beta_F192_L8  fp32   327744  38       53 ( 6208)               5    6       244 ( 1344)                 1
  S3    viewdir_beta_F192_L8  16-bit 327808  13       39 ( 8448)               7    3       233 ( 1408)                 2

What the sizes reach (asserted by test_large_sets_cpu.test_the_sizes_reach_every_named_regime):
  S1  15,300   Mpad = 15,360 in both tilings; skinny 60 splits in the 16-bit modes (thread groups 0 - 3 take the 64-stride
               loop, 4 - 7 only the tail), 120 in fp32; tile launch: n_split >= 8 on the narrow networks in both tilings,
               with a remainder (n%8 != 0) and with a grid that is rounded up (t*n%8 != 0).
  S2  163,803  Mpad = 163,840, past the skinny cap change at 131,072: exactly 256 skinny splits (bpart[256] full, the
               BN_REQUIRE bound); the tile launch at its full one-round split count, fp32 at its 2048-workgroup grid.
  S3  327,700  Mpad > 327,680: two rounds of the 256 CUs, twice the splits of S2.
The F = 256 / 512 cases stay at S1: their tile counts keep n_split small at any size; they are there for the many-tile
grid and the chained primal + adjoint jobs over 120 row tiles.

`spread` and the smallest split: the longest run of fillers is ceil(N / B) - 1 rows: 25 at S1, 148 at S2, 297 at S3.  At S1
and S2 that is below the floor of the tile launch (256 points in fp32, 512 in the 16-bit modes) and below every split of
the table (the smallest: the skinny launch's 128 points at S1 in fp32).  At S3 it is above fp32's 256-point floor, which
no launch is near at that size: the smallest split there has 1344 points.  Every split of every launch of the table
therefore holds a live row (asserted per (case, dtype, size) by tests/test_large_sets_cpu.py)."""
import torch

import lattice_cases as LC

PATTERNS = ("spread", "tail")
DTYPES = ("fp32", "bf16", "fp16")
MIN_SPLIT = {"fp32": 256, "bf16": 512, "fp16": 512}      # bn_wgrad_splits' min_mpb: the floor of the tile launch's point splits
W2_BLOCKS = 256                                          # BN_W2_BLOCKS (csrc/diag.h)
SKINNY_SPLITS = 256                                      # SKINNY_SPLITS (csrc/diag.h)

# size -> (N, live points B, cases)
SIZES = {
    "S1": (15300, 600, tuple(LC.CASES)),
    "S2": (163803, 1100, ("lambert_F64_L8", "rpv_an_F128_L4")),
    "S3": (327700, 1100, ("lambert_F64_L8", "rpv_an_F128_L4", "viewdir_beta_F192_L8")),
}


def case_sizes():
    return [(name, s) for s, (_, _, names) in SIZES.items() for name in names]


def embed(case, B, N, pattern):
    """-> (pts, coef, live, src): pts = (xyz, dirs, t) of N rows (float64; None where the case has none), coef the (N, C)
    float64 d_out (zero rows for fillers), live[i] the row of lattice point i < B, src[j] the lattice point row j copies.
      spread: live point i at row floor(i N / B) - no run of ceil(N / B) rows is without a live row
      tail:   the live points are the last B rows, ending at row N - 1
    Fillers cycle through all of the case's points (src[j] = j mod N_MAX)."""
    assert 1 <= B <= LC.N_MAX and B <= N and pattern in PATTERNS
    i = torch.arange(B, dtype=torch.int64)
    live = (i * N) // B if pattern == "spread" else N - B + i
    src = torch.arange(N, dtype=torch.int64) % LC.N_MAX
    src[live] = i
    pts = tuple(None if a is None else a[src].contiguous() for a in case.pts)
    coef = torch.zeros(N, case.coef.shape[1], dtype=torch.float64)
    coef[live] = case.coef[:B]
    return pts, coef, live, src


def longest_filler_run(live, N):
    """Longest run of consecutive rows without a live row."""
    edges = torch.cat([torch.tensor([-1]), live, torch.tensor([N])])
    return int((edges[1:] - edges[:-1]).max()) - 1


# ------------------------------------------------------------------------------------------------ the split policy, restated
def _cdiv(a, b):
    return -(-a // b)


def wgrad_jobs(case):
    """(N, K) of every job of the tile launch, in the order bn_field_backward_parts adds them (csrc/field_bwd.hip, the
    `add(...)` calls under "---- weight gradients"; the feats layer is folded into the heads: no job of its own)."""
    cfg = case.cfg
    F, L, skip, P, H2 = cfg.feat, cfg.layers, case.skip, 3, cfg.feat // 2          # P = FieldGeom.P without mapping
    trunk = []
    for l in range(L):
        if l == 0:
            trunk.append((F, P))
        elif l == skip:
            trunk += [(F, P), (F, F)]
        else:
            trunk.append((F, F))
    jobs = list(trunk)
    if case.flags.get("nr_an_on"):                      # `if (a.an)`: delta_l^T [gbar_PE ; abar_l], the same shapes again
        jobs += trunk
    jobs += [(H2, F)] * len(case.heads)                 # the folded first layers
    if cfg.dir_dim:
        jobs.append((H2, cfg.dir_dim))                  # `if (g.DD > 0 && G->head0_wdir)`
    if cfg.beta:
        jobs.append((H2, cfg.t_dim))                    # `if (g.TD > 0 && G->head1_wt)`
    return jobs


def split_counts(case, dtype, N):
    """-> (n_split of the tile launch, n_split of the skinny launch, rounds of the 256 CUs: 1 or 2; fp32: 1, its grid
    bound does not depend on the point count).  regime() gives the quantities they are made from."""
    r = regime(case, dtype, N)
    return r["wgrad"], r["skinny"], r["rounds"]


def regime(case, dtype, N):
    half = dtype != "fp32"
    BM = 128 if half else 64                            # bn_tile_config (csrc/field.h)
    Mpad = _cdiv(N, BM) * BM                            # bn_make_stash_layout (csrc/field.h)
    T = 256 if half else 128                            # bn_launch_wgrad (csrc/field_wgrad.hip): wv.tile0[j + 1] = ...
    tiles = sum(_cdiv(n, T) * _cdiv(k, T) for n, k in wgrad_jobs(case))
    # bn_wgrad_splits (csrc/field.h)
    stage, min_mpb = (64, 512) if half else (32, 256)
    bound = ((W2_BLOCKS if Mpad <= 327680 else 2 * W2_BLOCKS) if half else 2048)
    n_split = max(bound // tiles, 1)
    mpb = max(_cdiv(_cdiv(Mpad, n_split), stage) * stage, min_mpb)
    assert mpb >= MIN_SPLIT[dtype]
    wgrad = _cdiv(Mpad, mpb)
    # the `skinny_splits` block of bn_field_backward_parts (csrc/field_bwd.hip) and bn_launch_skinny (csrc/field_wgrad.hip)
    most = max(Mpad // (2 * BM), 1)
    if Mpad <= 131072 and most > 128:
        most = 128
    smpb = _cdiv(_cdiv(Mpad, min(SKINNY_SPLITS, most)), BM) * BM
    skinny = _cdiv(Mpad, smpb)
    return dict(Mpad=Mpad, tiles=tiles, bound=bound, wgrad=wgrad, mpb=mpb, skinny=skinny, smpb=smpb,
                rounds=2 if half and Mpad > 327680 else 1)


def table():
    """The docstring's table, from the restatement (test_large_sets_cpu asserts that the two agree)."""
    rows = ["  size  case                  dtype  Mpad    tiles  wgrad n_split (points each)  n%8  t*n%8  skinny n_split (points each)  rounds"]
    for name, s in case_sizes():
        N = SIZES[s][0]
        for dtype in ("fp32", "bf16"):                  # (fp16 = bf16: the policy knows the two tilings only)
            r = regime(LC.get_case(name), dtype, N)
            assert r == regime(LC.get_case(name), "fp16" if dtype == "bf16" else dtype, N)
            rows.append(f"  {s}    {name:<21} {'16-bit' if dtype == 'bf16' else dtype:<6} {r['Mpad']:<7} {r['tiles']:<6} "
                        f"{r['wgrad']:>4} ({r['mpb']:>5})               {r['wgrad'] % 8:<4} {r['tiles'] * r['wgrad'] % 8:<6} "
                        f"{r['skinny']:>4} ({r['smpb']:>5})                 {r['rounds']}")
    return "\n".join(rows)
