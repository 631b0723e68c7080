"""Premises of the large-set tests (tests/large_set_cases.py, tests/test_gpu_large_sets.py), asserted without a GPU: that
fillers are silent in the float64 reference, that embed() places the rows it says it places, and that the committed sizes
reach the split regimes they are named for (by the restated split policy)."""
import pytest
import torch

import lattice_cases as LC
import large_set_cases as LS


def _oracle(case, pts, coef):
    """oracle/field.py in float64 over the rows of `pts`: the output and autograd's gradient of sum(out * coef) with respect to
    every parameter (and the embedding rows with --beta), as lattice_cases.oracle_grads forms it for the first B points."""
    p = {k: v.clone().requires_grad_(True) for k, v in case.params.items()}
    xyz, dirs, t = pts
    t_in = None if t is None else t.clone().requires_grad_(True)
    out = LC.OF.field_forward(p, case.cfg, xyz, dirs=dirs, t_embed=t_in, **case.flags)
    leaves = list(p.values()) + ([t_in] if t_in is not None else [])
    gr = torch.autograd.grad((out * coef).sum(), leaves, allow_unused=True)
    G = {k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(p.items(), gr)}
    if t_in is not None:
        G["d_t_embed"] = gr[-1]
    return out.detach(), G


@pytest.mark.parametrize("pattern", LS.PATTERNS)
@pytest.mark.parametrize("name", ["rpv_an_F128_L4", "viewdir_beta_F192_L8"])
def test_fillers_are_silent_in_the_reference(name, pattern):
    """N = 300 rows, B = 65 live ones: autograd through oracle/field.py over ALL rows gives the gradient of the live points -
    the restated chains on the B lattice points, to the 1e-10 relative that test_lattice_cpu.py uses for the same tie; the
    filler rows of d_t_embed are exactly 0; forward row j is reference row src[j] (lattice_cases.reference_out, the GPU
    tests' reference).  Not bit for bit, because the reference itself is not: the pre-activations are exact, but torch
    evaluates exp / log1p of a float64 array with vector code in its body and scalar code in its last few elements, and the
    two differ in the last bit - reference_out(case, 300) and reference_out(case, 1100)[:300] differ by 1.1e-16 in rows 293 .. 299.
    So every head and sigma channel is held to 2^-51 max(|value|, 1) (the GPU tests' tolerance for them starts at
    4 x 2^-24 |value|), and at least 95 % of them must agree exactly.  The analytic normal the oracle takes from autograd,
    whose float64 sum over the paths rounds in an order that depends on the batch; it is held to the restated chain's exact
    value within the 1e-12 of test_lattice_cpu.py."""
    case = LC.get_case(name)
    N, B = 300, 65
    pts, coef, live, src = LS.embed(case, B, N, pattern)
    out, G64 = _oracle(case, pts, coef)
    G, _ = LC.backward_chains(case, LC.forward_book(case, B), LC.seeds_of(case, B))
    assert set(G) == set(G64), sorted(set(G) ^ set(G64))
    filler = torch.ones(N, dtype=torch.bool)
    filler[live] = False
    for k in G64:
        got = G64[k]
        if k == "d_t_embed":
            assert got.shape[0] == N and float(got[filler].abs().max()) == 0.0, f"{name} {pattern}: a filler row of d_t_embed is not exactly 0"
            got = got[live]
        assert float(G[k].abs().max()) > 0
        assert float((G[k] - got).abs().max()) <= 1e-10 * max(float(got.abs().max()), 1.0), f"{name} {pattern} {k}"
    want = LC.reference_out(case, LC.N_MAX)[src]
    assert out.shape == want.shape
    an = torch.zeros(out.shape[1], dtype=torch.bool)
    for kind, _, c0, w in LC.channels(case)[0]:
        an[c0:c0 + w] = kind == "normal_an"
    err, ulp = (out - want).abs(), 2.0 ** -52 * want.abs().clamp_min(1.0)     # (the RPV channels 2 y - 1, 2 y cross zero: ulps of 1)
    assert bool((err[:, ~an] <= 2 * ulp[:, ~an]).all()), f"{name} {pattern}: {int((err > 2 * ulp)[:, ~an].any(1).sum())} forward rows are not their source's row"
    assert int((err[:, ~an] == 0).sum()) >= 0.95 * err[:, ~an].numel()
    if bool(an.any()):
        assert float(err[:, an].max()) < 1e-12


def _smallest_split(case, dtype, N):
    r = LS.regime(case, dtype, N)
    return min(r["mpb"], r["smpb"])


@pytest.mark.parametrize("pattern", LS.PATTERNS)
@pytest.mark.parametrize("name,size", LS.case_sizes())
def test_embed_places_what_it_says(name, size, pattern):
    case = LC.get_case(name)
    N, B, _ = LS.SIZES[size]
    pts, coef, live, src = LS.embed(case, B, N, pattern)
    assert live.shape == (B,) and int(live[0]) >= 0 and int(live[-1]) < N and bool((live[1:] > live[:-1]).all())
    assert torch.equal(src[live], torch.arange(B)) and int(src.min()) >= 0 and int(src.max()) < LC.N_MAX
    assert len(torch.unique(src)) == LC.N_MAX, "the fillers do not cycle through all of the case's points"
    for a, b in zip(pts, case.pts):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.shape[0] == N and torch.equal(a, b[src])
    filler = torch.ones(N, dtype=torch.bool)
    filler[live] = False
    assert int(filler.sum()) == N - B and float(coef[filler].abs().max()) == 0.0
    assert torch.equal(coef[live], case.coef[:B]) and bool((coef[live] != 0).any(1).all())
    run = LS.longest_filler_run(live, N)
    if pattern == "spread":
        assert int(live[0]) == 0 and run == -(-N // B) - 1
        for dtype in LS.DTYPES:
            assert run < _smallest_split(case, dtype, N), f"{name} {size} {dtype}: a split of {_smallest_split(case, dtype, N)} points can be all fillers"
            if size != "S3":      # (S3: see the module docstring of large_set_cases)
                assert run < LS.MIN_SPLIT[dtype]
    else:
        assert int(live[-1]) == N - 1 and int(live[0]) == N - B and run == N - B
        for dtype in LS.DTYPES:
            BM = 128 if dtype != "fp32" else 64
            assert N % BM != 0, "the set is not ragged: no pad rows behind the live ones"


def test_the_sizes_reach_every_named_regime():
    """By the restatement (large_set_cases.regime): every regime the sizes are named for is reached at least once, and the
    table of the module docstring is the restatement's."""
    assert LS.table() in LS.__doc__, "the table in large_set_cases' docstring is not what the restatement gives:\n" + LS.table()
    R = {(n, s, d): LS.regime(LC.get_case(n), d, LS.SIZES[s][0]) for n, s in LS.case_sizes() for d in LS.DTYPES}
    for (n, s, d), r in R.items():
        assert LS.split_counts(LC.get_case(n), d, LS.SIZES[s][0]) == (r["wgrad"], r["skinny"], r["rounds"])
        assert r["skinny"] <= 256 and r["tiles"] * r["wgrad"] <= max(r["tiles"], r["bound"])
    half = lambda d: d != "fp32"  # noqa: E731
    narrow = ("lambert_F64_L8", "rpv_an_F128_L4")
    # S1
    for (n, s, d), r in R.items():
        if s == "S1":
            assert r["Mpad"] == 15360 and r["skinny"] == (60 if half(d) else 120)
            if n in narrow:
                assert r["wgrad"] >= 8, f"{n} {d}: wgrad_reduce_kernel's 8-wide loop is not reached"
    assert any(s == "S1" and half(d) and r["wgrad"] >= 8 and r["wgrad"] % 8 for (n, s, d), r in R.items())
    assert any(s == "S1" and not half(d) and r["wgrad"] >= 8 and r["wgrad"] % 8 for (n, s, d), r in R.items())
    assert any(s == "S1" and half(d) and r["tiles"] * r["wgrad"] % 8 for (n, s, d), r in R.items()), "no 16-bit grid is rounded up to a multiple of 8"
    assert any(57 <= r["skinny"] <= 63 for r in R.values()), "no skinny launch with thread groups on both sides of the 64-stride loop"
    assert any(r["skinny"] >= 64 and r["skinny"] % 64 for r in R.values())
    # S2
    for (n, s, d), r in R.items():
        if s == "S2":
            assert r["Mpad"] == 163840 and r["skinny"] == 256 and r["rounds"] == 1
            if half(d):
                assert r["wgrad"] == LS.W2_BLOCKS // r["tiles"], f"{n} {d}: not the full one-round split count"
            else:
                assert 2048 - r["tiles"] * 16 <= r["tiles"] * r["wgrad"] <= 2048, f"{n} {d}: the fp32 grid is not near its 2048 workgroups"
    # both sides of 131,072 and of 327,680
    assert any(r["Mpad"] <= 131072 for r in R.values()) and any(131072 < r["Mpad"] <= 327680 for r in R.values())
    for (n, s, d), r in R.items():
        if s == "S3":
            assert r["Mpad"] > 327680 and r["rounds"] == (2 if half(d) else 1)
            if half(d):
                assert r["wgrad"] == 2 * LS.W2_BLOCKS // r["tiles"]
                if (n, "S2", d) in R:
                    assert r["wgrad"] in (2 * R[(n, "S2", d)]["wgrad"], 2 * R[(n, "S2", d)]["wgrad"] + 1)
