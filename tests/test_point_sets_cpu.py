"""Premises of tests/test_gpu_point_sets.py, asserted on the CPU (tests/point_set_cases.py).  They are conditions, not
measurements: if one fails, the GPU tests' bit-equality argument does not hold and the cases have to change."""
import pytest
import torch

import lattice_cases as LC
import point_set_cases as PS


def _cases():
    return [(n, 11) for n in PS.SETS] + [("A", 6)]


def _fp32_exact(t):
    return torch.equal(t.float().double(), t)


@pytest.mark.parametrize("name,stride", _cases())
def test_the_points_of_a_ray_set_are_exact(name, stride):
    """o, d, z on their grids and inside their ranges; d z and o + d z survive float(): the fp32 evaluation (a multiply and an
    add, each rounded) equals the float64 one bit for bit, and so does an fma, whose single rounding acts on an exactly
    representable value; |x| <= 1; no two points of the set coincide; S != G where the case says so; R S is a tile
    multiple in every mode exactly for the sets that are run merged."""
    R, S, G = PS.SETS[name]
    rs = PS.ray_set(name, stride)
    rays, z, z2 = rs["rays"], rs["z"], rs["z2"]
    assert rays.shape == (R, stride) and z.shape == (R, S) and z2.shape == (R, G)
    o, d = rays[:, 0:3], rays[:, 3:6]
    for t, q, lo, hi in ((o, PS.QO, -0.5, 0.5), (d, PS.QD, -1.0, 1.0), (z, PS.QZ, 0.0, 0.5 - PS.QZ), (z2, PS.QZ, 0.0, 0.5 - PS.QZ)):
        assert torch.equal(torch.round(t / q) * q, t) and float(t.min()) >= lo and float(t.max()) <= hi
    assert bool(d.ne(0).any(1).all())
    for zz in (z, z2):
        assert bool((zz[:, 1:] > zz[:, :-1]).all()), "depths ascend strictly within a block"
        prod = d[:, None, :] * zz[:, :, None]
        assert _fp32_exact(prod)
        x64, _ = PS.block_points(rays, zz)
        x32, _ = PS.block_points(rays.float(), zz.float())
        assert _fp32_exact(x64) and torch.equal(x32.double(), x64)
    X, dirs = PS.set_points(rs)
    n_all = R * (S + G)
    assert X.shape == (n_all, 3) and dirs.shape == (n_all, 3)
    assert float(X.abs().max()) <= 1.0
    assert torch.unique(X, dim=0).shape[0] == n_all, "two points of the set coincide"
    assert torch.equal(dirs[:R * S].view(R, S, 3)[:, 0], d) and torch.equal(dirs[R * S:].view(R, G, 3)[:, -1], d)
    if name in PS.S_NE_G:
        assert S != G
    for dtype, tile in PS.TILE.items():
        assert ((R * S) % tile == 0) == (name in PS.MERGEABLE), (name, dtype)


def test_the_sets_reach_what_they_claim():
    """A: the second block starts at tile 1 of the 16-bit modes and the last tile is ragged; B / C: two / three point splits of
    the 16-bit weight gradient (512 points per split at these sizes, bn_wgrad_splits in csrc/field.h: min_mpb); D: R S is no
    multiple of a tile, G of C is a power of two while S is not."""
    n = {k: R * (S + G) for k, (R, S, G) in PS.SETS.items()}
    assert n == {"A": 208, "B": 608, "C": 1152, "D": 104}
    assert PS.SETS["A"][0] * PS.SETS["A"][1] == 128 and n["A"] % 128 != 0 and n["A"] % 64 != 0
    pad = lambda m: -(-m // 128) * 128  # noqa: E731
    assert -(-pad(n["A"]) // 512) == 1 and -(-pad(n["B"]) // 512) == 2 and -(-pad(n["C"]) // 512) == 3
    _, S, G = PS.SETS["C"]
    assert G & (G - 1) == 0 and S & (S - 1) != 0


@pytest.mark.parametrize("name,B", PS.LATTICE)
def test_the_lattice_cases_in_set_form(name, B):
    """The lattice cases are ones case_sizes() offers with B in (600, 1100); the split is a tile multiple of every mode
    inside the set; as one-sample rays (z = 1, z2 = 2) the fp32 evaluation of o + d z gives the case's points bit for bit,
    with an fma or without (d z and the sum are exact)."""
    assert (name, B) in LC.case_sizes() and B in (600, 1100)
    assert {bool(LC.CASES[n][1].get("nr_an_on")) for n, _ in PS.LATTICE} == {False, True}
    h = PS.split_point(B)
    assert 0 < h < B and all(h % t == 0 for t in PS.TILE.values()) and abs(h - B / 2) <= 64
    case = LC.get_case(name)
    rb = PS.lattice_ray_blocks(name, B)
    R = rb["n"] // 2
    assert R == h and rb["rays"].shape == (R, 11) and rb["z"].shape == (R, 1) and rb["z2"].shape == (R, 1)
    for zz, want in ((rb["z"], case.pts[0][:R]), (rb["z2"], case.pts[0][R:2 * R])):
        assert _fp32_exact(rb["rays"]) and _fp32_exact(rb["rays"][:, None, 3:6] * zz[:, :, None])
        x64, _ = PS.block_points(rb["rays"], zz)
        x32, _ = PS.block_points(rb["rays"].float(), zz.float())
        assert torch.equal(x64, want) and torch.equal(x32.double(), want)


@pytest.mark.parametrize("name,B", PS.LATTICE)
def test_a_preloaded_accumulator_stays_exact(name, B):
    """The accumulation test preloads gradient accumulators with a constant c and expects c + gradient back, bit for bit in
    the 16-bit modes: c + (the first half's gradient) and c + (the whole gradient) must be fp32 values, and so must the
    gradients (asserted by test_gpu_lattice._check_gradients as well)."""
    case = LC.get_case(name)
    h = PS.split_point(B)
    G_half, _ = LC.backward_chains(case, LC.forward_book(case, h), LC.seeds_of(case, h))
    G_all, _ = LC.backward_chains(case, LC.forward_book(case, B), LC.seeds_of(case, B))
    for k, c in PS.PRELOAD.items():
        assert k in G_all
        assert float(G_all[k].abs().max()) > 0, f"{k}: the case gives it no gradient"
        for g in (G_half[k], G_all[k]):
            assert _fp32_exact(g) and _fp32_exact(g + c), k
