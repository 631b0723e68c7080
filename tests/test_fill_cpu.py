"""CPU tests of the hole filling (brdf_nerf_amd/fill.py): the statement of tests/fill_cases.py against what the reference's
quickly_interpolate_nans_from_singlechannel_img recorded (tests/golden/fill_*.npz, written by tests/golden/make_fill_goldens.py),
the proof that the two-pass decomposition is the brute force, the ABI's two entries and the refusals the host can check."""
import os
import re

import numpy as np
import pytest
import torch

import fill_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", F.GOLDENS)
def test_statement_against_the_reference(name):
    """Known cells unchanged on both sides; the statement's value equals the reference's bit for bit on every hole with a unique
    nearest known cell; on every other hole the reference's value is found among the known cells at the statement's d2.  The
    generator's two conditions on the inputs hold on the committed files."""
    g = F.golden(name)
    assert g["u"].dtype == np.float32 and g["ref"].dtype == np.float32
    assert g["u"].shape == {"holes5": (60, 72), "holes30": (104, 112), "sparse90": (96, 130)}[name]
    filled, source, dist2 = F.statement(g["u"])
    unique, ties = F.against_reference(g["u"], filled, dist2, g["ref"])
    print(f"{name}: {unique + ties} holes, {unique} with a unique nearest cell, {ties} ties, largest d2 {int(dist2.max())}")
    assert unique >= 400 and ties >= 200
    assert unique + ties == int(np.isnan(g["u"]).sum())
    size = os.path.getsize(os.path.join(F.GOLDEN_DIR, f"fill_{name}.npz"))
    assert size <= max(os.path.getsize(os.path.join(F.GOLDEN_DIR, f)) for f in os.listdir(F.GOLDEN_DIR) if f.startswith("dsmr_"))


def same(a, b):
    return all(np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(F.CASES))
def test_two_pass_is_the_brute_force(name):
    """The decomposition of include/brdfnerf_hip.h: the column pass, then the row pass over every column, gives the brute
    force's filled bits, source and d2 in every cell."""
    u = F.CASES[name]
    assert same(F.two_pass(u), F.statement(u)), name


def test_two_pass_is_the_brute_force_on_the_small_patterns_and_goldens():
    for u in F.patterns_3x3() + F.patterns_4x5() + [F.golden(n)["u"] for n in F.GOLDENS]:
        assert same(F.two_pass(u), F.statement(u)), u
    assert len(F.patterns_3x3()) == 511 and len(F.patterns_4x5()) == 200
    assert same(F.two_pass(F.ALL_NAN), F.statement(F.ALL_NAN)) and (F.statement(F.ALL_NAN)[1] == -1).all()


def test_the_statement_on_cases_with_a_known_answer():
    """The tie pair's answer is (1, 2); an all-known grid is the identity; values keep their bits, NaN payloads do not leak."""
    filled, source, dist2 = F.statement(F.tie_pair())
    assert source[1, 1] == 1 * 3 + 2 and filled[1, 1] == 12.0 and dist2[1, 1] == 1
    u = F.CASES["5x6_all_known"]
    filled, source, dist2 = F.statement(u)
    assert np.array_equal(F.bits(filled), F.bits(u)) and np.array_equal(source, np.arange(30).reshape(5, 6)) and not dist2.any()
    u = F.CASES["7x9_special_values"]
    filled, source, _ = F.statement(u)
    known = ~np.isnan(u)
    assert not np.isnan(filled).any() and set(F.bits(filled).ravel()) <= set(F.bits(u)[known])
    for v in (np.float32(-0.0), np.float32(1e-42), np.float32(np.inf), np.float32(-np.inf), np.float32(-1e-45)):
        assert v.view(np.int32) in F.bits(u)[known]
    assert len({int(b) for b in F.bits(u)[~known]}) >= 3                       # several NaN payloads among the holes
    u = F.CASES["40x600_last_two_columns"]
    assert not (~np.isnan(u))[:, :598].any() and F.counts(u)[1] >= 598 ** 2
    assert F.near_rows(np.array([[1.0], [np.nan], [2.0]], np.float32))[:, 0].tolist() == [0, 0, 2]   # the tie goes to the smaller row


def test_header_and_binding_carry_the_two_entries():
    from brdf_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    declared = set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", header))
    for name in ("bn_grid_nearest_col", "bn_grid_fill"):
        assert name in declared and name in _lib._SIGS and name in _lib.exported_symbols(), name
        assert hasattr(_lib.lib(), name), name
    assert int(re.search(r"#define BN_FILL_MAX_SIDE (\d+)", header).group(1)) == _lib.BN_FILL_MAX_SIDE == 8192
    assert [len(_lib._SIGS[n][1]) for n in ("bn_grid_nearest_col", "bn_grid_fill")] == [5, 11]
    assert _lib.BN_ABI_VERSION == 7 and _lib.lib().bn_abi_version() == 7
    import brdf_nerf_amd
    for name in ("fill_holes", "apply_fill"):
        assert name in brdf_nerf_amd.__all__ and callable(getattr(brdf_nerf_amd, name))


def test_refusals_raise_before_any_library_call(monkeypatch):
    """ValueError by name from host tensors, with the library's loader replaced by a trap: host tensors, a dtype other than
    float32, a grid that is not 2-D or not contiguous, too large a side, rows out of range."""
    from brdf_nerf_amd import _lib
    from brdf_nerf_amd import functions as Fn
    from brdf_nerf_amd import apply_fill, fill_holes

    def trap(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "lib", trap)
    z = torch.zeros(4, 5)
    near = torch.zeros(4, 5, dtype=torch.int32)
    for call in (lambda: fill_holes(z), lambda: Fn.grid_nearest_col(z), lambda: Fn.grid_fill(z, near)):
        with pytest.raises(ValueError, match="device"):
            call()
    with pytest.raises(ValueError, match="device"):
        fill_holes(z.numpy())
    for call in (lambda: fill_holes(z.double()), lambda: Fn.grid_nearest_col(z.half()), lambda: Fn.grid_fill(z.double(), near),
                 lambda: Fn.grid_fill(z, near.long())):
        with pytest.raises(ValueError, match="float32|int32"):
            call()
    for bad in (torch.zeros(20), torch.zeros(2, 2, 5), torch.zeros(5, 4).t(), torch.zeros(4, 10)[:, ::2]):
        with pytest.raises(ValueError, match="contiguous 2-D"):
            fill_holes(bad)
        with pytest.raises(ValueError, match="contiguous 2-D"):
            Fn.grid_nearest_col(bad)
    with pytest.raises(ValueError, match="8192"):
        fill_holes(torch.zeros(1, 8193))
    with pytest.raises(ValueError, match="8192"):
        Fn.grid_nearest_col(torch.zeros(0, 5))
    with pytest.raises(ValueError, match="not on the grid"):
        Fn.grid_fill(z, torch.zeros(5, 4, dtype=torch.int32))
    for rows in ((-1, 3), (0, 5), (3, 2)):
        with pytest.raises(ValueError, match="rows"):
            fill_holes(z, rows=rows)
        with pytest.raises(ValueError, match="rows"):
            Fn.grid_fill(z, near, rows=rows)
    with pytest.raises(ValueError, match="one"):
        apply_fill(z, torch.zeros(5, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        apply_fill(z, torch.zeros(4, 5))
    # apply_fill is one take on whatever device the layer lies on
    src = torch.tensor([[1, 1, 2], [5, 4, 5]], dtype=torch.int32)
    assert apply_fill(torch.arange(6.0).reshape(2, 3), src).tolist() == [[1.0, 1.0, 2.0], [5.0, 4.0, 5.0]]
