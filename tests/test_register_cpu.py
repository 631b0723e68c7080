"""CPU tests of the xy registration (brdf_nerf_amd/register.py): the statements of tests/register_cases.py against what the
reference's dsmr.py recorded (tests/golden/dsmr_*.npz, written by tests/golden/make_dsmr_goldens.py), the host logic - the choice
of (pivot, k), the scan order on a tie, a level where no shift can win - the refusals and the ABI."""
import math
import os
import re

import numpy as np
import pytest
import torch

import register_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.int64(0x7FF8000000000000), a.view(np.int64))


def bits32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.int32(0x7FC00000), a.view(np.int32))


@pytest.mark.parametrize("name", R.GOLDENS)
def test_goldens_meet_their_condition(name):
    """The inputs' condition, recorded by the generator: the reference's best correlation leads the second by 1e-3 or more at
    every level, so a restatement that moves a correlation by 1e-7 must find the same shift."""
    g = R.golden(name)
    assert g["u"].dtype == np.float32 and g["v"].dtype == np.float32 and g["rdsm"].dtype == np.float32
    assert len(g["gaps"]) == len(g["levels"]) == {"no_pyramid": 1, "one_level": 2, "two_levels": 3}[name]
    assert float(g["gaps"].min()) >= 1e-3
    assert min(g["u"].shape) <= 100 if name == "no_pyramid" else min(g["u"].shape) > 100


@pytest.mark.parametrize("name", R.GOLDENS)
def test_halve_statement_is_the_reference_pyramid(name):
    """Every level of the pyramid recursive_ncc formed, bit for bit, NaN cells included."""
    g = R.golden(name)
    pyr = R.golden_registration(name)["pyramid"]
    assert len(pyr) == len(g["levels"])
    for l in range(1, len(pyr)):
        for got, key in zip(pyr[l], (f"u{l}", f"v{l}")):
            assert got.shape == g[key].shape and got.dtype == np.float64
            assert np.array_equal(bits64(got), bits64(g[key])), (name, key)


@pytest.mark.parametrize("name", R.GOLDENS)
def test_integer_search_finds_the_reference_shifts(name):
    """(dx, dy) of every level equals compute_ncc's; the integer correlations are printed against the reference's float64 ones;
    |b - b_ref| <= 2^-k + 1e-9 (each mean is within half a quantum of the float64 one; 1e-9 covers the float64 sums' own error)."""
    g = R.golden(name)
    s = R.golden_registration(name)
    assert [tuple(int(x) for x in row) for row in g["levels"]] == s["levels"]
    worst = 0.0
    for ms, ref in zip(s["moments"], g["corr"]):
        for m, c in zip(ms, ref):
            mine = R.corr(m)
            assert (mine is None) == (not np.isfinite(c))
            if mine is not None:
                worst = max(worst, abs(mine - float(c)))
    err_b = abs(s["b"] - float(g["b"]))
    print(f"{name}: k {s['k']} pivot {s['pivot']}, max |corr_int - corr_ref| {worst:.3e}, |b - b_ref| {err_b:.3e}, gaps {g['gaps']}")
    assert err_b <= 2.0 ** -s["k"] + 1e-9


@pytest.mark.parametrize("name", R.GOLDENS)
def test_shift_statement_is_the_reference_apply_shift(name):
    """Fed the reference's own b, rdsm equals apply_shift_'s float32 output bit for bit."""
    g = R.golden(name)
    H, W, dx, dy = (int(x) for x in g["levels"][-1])
    rdsm, diff, sums = R.shift_diff(g["v"], g["u"], dx, dy, float(g["b"]))
    assert np.array_equal(bits32(rdsm), bits32(g["rdsm"]))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(bits32(diff), bits32(g["rdsm"] - g["u"]))          # the float32 subtraction of sat_utils.py:246
    assert 0 < sums[1] < H * W and sums[0] / (sums[1] * 2.0 ** 20) == pytest.approx(float(np.nanmean(np.abs(diff))), rel=1e-6)
    assert sums[0] / (sums[1] * 2.0 ** 20) < 0.2                                  # registered: noise alone is left


def test_pivot_and_scale_choice():
    """span 1 -> k = 16 (the cap), 63 and 64 -> 14, 65 -> 13, 2^20 -> 0, above: refused.  The package's rule is the statement's."""
    from brdf_nerf_amd.register import quantisation
    for lo, hi, want in ((5.0, 5.0, (5, 16)), (5.25, 5.75, (5, 16)), (-3.5, 59.2, (-4, 14)), (0.0, 63.0, (0, 14)), (0.0, 64.0, (0, 14)), (10.0, 74.5, (10, 13)),
                         (-7.0, 2.0 ** 20 - 7.0, (-7, 0)), (0.5, 16.5, (0, 15)), (0.0, 16.0, (0, 16))):
        assert quantisation(lo, hi) == want == R.choose_scale(lo, hi), (lo, hi)
    assert R.choose_scale(0.0, 2.0 ** 20 + 0.5) is None
    with pytest.raises(ValueError, match="2\\^20"):
        quantisation(0.0, 2.0 ** 20 + 0.5)
    with pytest.raises(ValueError, match="finite"):
        quantisation(float("nan"), 1.0)
    # the ends of the span are the ends of the quanta
    q, skipped = R.quanta(np.array([[100.0, 164.0, 132.0, np.nan, np.inf]]), 100, 14)
    assert q.tolist() == [[0, 1 << 20, 1 << 19, -1, -1]] and skipped == 0
    assert R.quanta(np.array([[99.0, 165.0, 100.0]]), 100, 14)[1] == 2


def test_tie_order():
    """Two shifts with equal integer moments: the scan is dy outer, dx inner with strict >, so (1, 0) wins over (0, 1); the
    same integers scanned dx outer would return (0, 1), so this case tells the orders apart."""
    from brdf_nerf_amd.register import best_shift, correlation
    u, v = R.tie_case()
    pivot, k = R.choose_scale(0.0, 8.0)
    ms, _ = R.moments(u, v, pivot, k, 0, 0, 2)
    side = 5
    at = lambda dx, dy: (dy + 2) * side + (dx + 2)
    assert ms[at(1, 0)] == ms[at(0, 1)] and correlation(ms[at(1, 0)]) == max(c for c in map(correlation, ms) if c is not None)
    assert best_shift(ms, 0, 0, 2) == (1, 0, at(1, 0)) == R.search(ms, 0, 0, 2)
    swapped = [ms[at(dx, dy)] for dx in range(-2, 3) for dy in range(-2, 3)]      # dx outer
    s = best_shift(swapped, 0, 0, 2)[2]
    assert (s // side - 2, s % side - 2) == (0, 1)


def test_a_level_where_no_shift_can_win_returns_its_start():
    from brdf_nerf_amd.register import best_shift, correlation
    u, v = np.full((6, 7), 3.0), R.moment_case("33x31_r5")["v"][:6, :7]
    ms, _ = R.moments(u, v, 0, 10, 4, -2, 1)                                      # a constant u: B = 0 at every shift
    assert all(correlation(m) is None for m in ms) and any(m[0] > 0 for m in ms)
    assert best_shift(ms, 4, -2, 1) == (4, -2, None) == R.search(ms, 4, -2, 1)
    empty = [(0,) * 6] * 9
    assert best_shift(empty, -3, 5, 1) == (-3, 5, None)


def test_moment_statement_against_plain_pearson():
    """The integer correlation against numpy's float64 Pearson coefficient of the same pairs, and row bands that add up."""
    c = R.moment_case("33x31_r5")
    ms, skipped = R.moments_expected("33x31_r5")
    assert skipped == 0 and len(ms) == 121
    u, v = c["u"], c["v"]
    for (dx, dy) in ((0, 0), (3, -2), (-5, 5)):
        m = ms[(dy + 5) * 11 + (dx + 5)]
        a, b = [], []
        for j in range(33):
            for i in range(31):
                if 0 <= j + dy < 33 and 0 <= i + dx < 31 and np.isfinite(u[j, i]) and np.isfinite(v[j + dy, i + dx]):
                    a.append(u[j, i])
                    b.append(v[j + dy, i + dx])
        assert m[0] == len(a) > 100
        assert R.corr(m) == pytest.approx(float(np.corrcoef(a, b)[0, 1]), abs=1e-6)
        assert (m[1] - m[2]) / (m[0] * 2 ** c["k"]) == pytest.approx(float(np.mean(a) - np.mean(b)), abs=2.0 ** -c["k"])
    parts = [R.moments_expected("33x31_r5", rows)[0] for rows in ((0, 7), (7, 32), (32, 33))]
    assert [tuple(sum(x) for x in zip(*ps)) for ps in zip(*parts)] == ms
    few = R.moments_expected("3x5_r5")[0]
    assert sum(1 for m in few if m[0] == 0) > 60
    ends = R.moments_expected("32x64_ends")[0]
    assert max(m[3] for m in ends) >= 1000 * (1 << 40)                            # sums of q^2 that need 64 bits
    assert R.moments_expected("33x40_wrong_pivot")[1] > 0 and all(m[0] == 0 for m in R.moments_expected("20x34_vnan")[0])


def test_header_and_binding_carry_the_three_entries():
    from brdf_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    declared = set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", header))
    for name in ("bn_grid_halve", "bn_ncc_moments", "bn_dsm_shift_diff"):
        assert name in declared and name in _lib._SIGS, name
        assert hasattr(_lib.lib(), name), name
    assert int(re.search(r"#define BN_NCC_MAX_RANGE (\d+)", header).group(1)) == _lib.BN_NCC_MAX_RANGE == 8
    assert int(re.search(r"#define BN_NCC_MAX_SCALE (\d+)", header).group(1)) == _lib.BN_NCC_MAX_SCALE == 16
    assert _lib.BN_NCC_MAX_SHIFT == 1 << 20 and _lib.BN_NCC_MAX_CELLS == 1 << 22
    assert _lib.BN_ABI_VERSION == 7 and _lib.lib().bn_abi_version() == 7
    assert [len(_lib._SIGS[n][1]) for n in ("bn_grid_halve", "bn_ncc_moments", "bn_dsm_shift_diff")] == [5, 14, 12]
    import brdf_nerf_amd
    for name in ("register_xy", "apply_registration", "altitude_mae_xy"):
        assert name in brdf_nerf_amd.__all__ and callable(getattr(brdf_nerf_amd, name))
    from brdf_nerf_amd.build import FILE_FLAGS
    assert "-ffp-contract=off" in FILE_FLAGS["register.hip"]
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "brdf_nerf_amd", "csrc", "register.hip")).read()


def test_refusals_raise_before_any_library_call(monkeypatch):
    """ValueError by name, from host tensors, with the three bindings replaced by a trap."""
    from brdf_nerf_amd import functions as Fn
    from brdf_nerf_amd import altitude_mae_xy, apply_registration, register_xy, score_view

    def trap(*a, **k):
        raise AssertionError("the library was called")

    for name in ("grid_halve", "ncc_moments", "dsm_shift_diff"):
        monkeypatch.setattr(Fn, name, trap)
    z = torch.zeros(4, 5)
    for fn in (register_xy, altitude_mae_xy):
        with pytest.raises(ValueError, match="one"):
            fn(z, torch.zeros(5, 4))
        with pytest.raises(ValueError, match="2\\^22"):
            fn(torch.zeros(2049, 2048), torch.zeros(2049, 2048))
    with pytest.raises(ValueError, match="one"):
        apply_registration(z, torch.zeros(4, 5, 1), 0, 0, 0.0)
    for bad in (-1, 9, 2.0):
        with pytest.raises(ValueError, match="irange"):
            register_xy(z, z, irange=bad)
    with pytest.raises(ValueError, match="device"):
        register_xy(z, z)
    with pytest.raises(ValueError, match="device"):
        apply_registration(z, z, 0, 0, 0.0)
    with pytest.raises(ValueError, match="mask"):
        altitude_mae_xy(z, z, mask=torch.ones(5, 5))
    with pytest.raises(ValueError, match="register"):
        score_view(None, None, torch.zeros(12, 11), torch.zeros(12, 3), 3, 4, register="bogus")
    assert math.isnan(R.register(np.full((3, 3), np.nan), np.ones((3, 3)))["b"])
