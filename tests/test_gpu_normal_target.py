"""bn_normal_target_loss (csrc/normal_target.hip: NormalLoss against the rays' target normals, --nr_spv_type 2 / 3) against its
statement in numpy float32 (tests/normal_spv_cases.py) BIT FOR BIT: the three d_acc columns it adds into, ray_loss and the count;
every other column of d_acc and every unselected row bitwise untouched.  The statement is held to the reference by
tests/test_normal_spv_cpu.py.  A NaN is compared as a NaN (its payload is not part of the rule)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normal_spv_cases as NS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
LAM = 0.37


def same_bits(got, want):
    got, want = np.asarray(got, F), np.asarray(want, F)
    nan = np.isnan(want)
    return got.shape == want.shape and (np.isnan(got) == nan).all() and (NS.bits(got)[~nan] == NS.bits(want)[~nan]).all()


def run(c, ch, lam=LAM, nonfinite=False, strided=False, slots=0):
    """One call on the case dict `c` (numpy) -> (d_acc, ray_loss, n_sel, dropped (nan, inf) or None, loss_acc or None)."""
    from brdf_nerf_amd import functions as Fn
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    acc, d_acc, ray_loss = t(c["acc"]), t(c["d_acc"]), t(c["ray_loss"])
    R = acc.shape[0]
    if strided:      # valid_depth as a column of depths-like storage, the normals as three columns of wider rows, valid_normal every 3rd element
        store = torch.full((R, 2), 7.0, device=DEV)
        store[:, 1] = t(c["valid_depth"])
        vd = store[:, 1]
        wide = torch.full((R, 5), -3.0, device=DEV)
        wide[:, 1:4] = t(c["normals"])
        normals = wide[:, 1:4]
        vn3 = torch.full((R, 3), 9.0, device=DEV)
        vn3[:, 2] = t(c["valid_normal"])
        vn = vn3[:, 2]
    else:
        vd, normals, vn = t(c["valid_depth"]), t(c["normals"]), t(c["valid_normal"])
    nf = torch.zeros(2, dtype=torch.int64, device=DEV) if nonfinite else None
    la = torch.zeros(slots, device=DEV) if slots else None
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    Fn.normal_target_loss(acc, ch, normals, vn, vd, lam, d_acc, ray_loss=ray_loss, loss_acc=la, nonfinite=nf, count=count)
    torch.cuda.synchronize()
    return (d_acc.cpu().numpy(), ray_loss.cpu().numpy(), int(count.item()), None if nf is None else tuple(nf.tolist()),
            None if la is None else la.cpu().numpy())


def check(c, ch, **kw):
    st = NS.statement(c["acc"], ch, c["normals"], c["valid_normal"], c["valid_depth"], kw.get("lam", LAM), kw.get("nonfinite", False))
    want_d, want_l = NS.apply(c["d_acc"], c["ray_loss"], ch, st)
    d, rl, n, dropped, la = run(c, ch, **kw)
    assert n == st["n_sel"]
    assert same_bits(d, want_d), np.argwhere(NS.bits(d) != NS.bits(want_d))[:5]
    assert same_bits(rl, want_l)
    # (implied by the above, stated for the reader: what the entry must not touch)
    other = np.ones(c["acc"].shape[1], bool)
    other[ch:ch + 3] = False
    assert (NS.bits(d[:, other]) == NS.bits(c["d_acc"][:, other])).all()
    assert (NS.bits(d[~st["touched"]]) == NS.bits(c["d_acc"][~st["touched"]])).all()
    if dropped is not None:
        assert dropped == st["dropped"]
    return st, d, rl, la


@pytest.mark.parametrize("R", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_kernel_equals_statement_bit_for_bit(R):
    """Sizes around the wave (64), the block (256) and the count's stride (1000 < 1024 lanes, one ray each); C in {7, 16, 28} with
    the normal at the first, the last and a middle channel; contiguous and strided inputs; two calls give the same bits."""
    for C_, chs in ((7, (0, 4, 2)), (16, (0, 13, 5)), (28, (0, 25, 11))):
        for i, ch in enumerate(chs):
            c = NS.make_inputs(R, C_, ch, seed=1000 * R + 10 * C_ + ch)
            if R == 1:
                c["valid_depth"][:] = 1.0
            st, d, rl, _ = check(c, ch, strided=(i == 1), nonfinite=(i == 2))
            if i == 0:
                d2, rl2, n2, _, _ = run(c, ch)
                assert (NS.bits(d2) == NS.bits(d)).all() and (NS.bits(rl2) == NS.bits(rl)).all() and n2 == st["n_sel"]
    assert st["n_sel"] >= 1


def test_count_needs_more_than_one_pass_of_the_workgroup():
    """R over 1024: every lane of the count takes several rays, the per-ray grid has a partial last block."""
    c = NS.make_inputs(2500, 7, 4, seed=5)
    st, *_ = check(c, 4, strided=True)
    assert 1000 < st["n_sel"] < 2000


@pytest.mark.parametrize("R", [65, 257])
def test_selection_all_none_one(R):
    c = NS.make_inputs(R, 16, 7, seed=R)
    c["valid_depth"][:] = 1.0
    assert check(c, 7)[0]["n_sel"] == R
    c["valid_depth"][:] = 0.0
    st, d, rl, la = check(c, 7, slots=64)
    assert st["n_sel"] == 0 and (NS.bits(d) == NS.bits(c["d_acc"])).all() and (NS.bits(rl) == NS.bits(c["ray_loss"])).all()
    assert not la.any()
    c["valid_depth"][R - 2] = 1.0
    c["valid_normal"][R - 2] = 1.0
    st, d, _, _ = check(c, 7)
    assert st["n_sel"] == 1 and st["touched"].sum() == 1 and (d[R - 2, 7:10] != c["d_acc"][R - 2, 7:10]).any()


def test_valid_depth_values_and_valid_normal_all_zero():
    """valid_depth 0.5 and 2 select; -1, -0.0 and NaN do not.  valid_normal plays no part in the count: all 0 still counts every
    selected ray (their terms and gradients are zeros)."""
    R = 130
    c = NS.make_inputs(R, 7, 4, seed=77)
    c["valid_depth"] = np.resize(np.array([0.5, 2.0, -1.0, -0.0, np.nan, 0.0, 1.0], F), R)
    st, *_ = check(c, 4)
    assert st["n_sel"] == int(np.isin(np.arange(R) % 7, (0, 1, 6)).sum())
    c["valid_normal"][:] = 0.0
    st0, d, rl, _ = check(c, 4, strided=True)
    assert st0["n_sel"] == st["n_sel"] and not st0["term"].any()
    assert (d == c["d_acc"]).all() and (rl == c["ray_loss"]).all()        # (numerically; a -0.0 + 0.0 may change a sign bit)


def test_planted_zeros_and_negative_zero():
    """e_c == 0 exactly (acc equal to the target) gives s = 0; acc == -0.0 against a target of 0 likewise; the additions of a zero
    follow float32 (-0.0 + 0.0 = +0.0), as the statement's do."""
    R = 70
    c = NS.make_inputs(R, 16, 5, seed=9)
    c["valid_depth"][:8] = 1.0
    c["valid_normal"][:8] = 1.0
    c["acc"][0, 5:8] = c["normals"][0]
    c["acc"][1, 6] = c["normals"][1, 1]
    c["normals"][2, 0] = 0.0
    c["acc"][2, 5] = -0.0
    c["normals"][3] = [0.0, -0.0, 1.0]
    c["acc"][3, 5:8] = [-0.0, 0.0, 1.0]
    c["d_acc"][0, 5:8] = [-0.0, 0.0, 1.5]
    c["d_acc"][3, 5:8] = -0.0
    st, d, _, _ = check(c, 5)
    assert not st["grad"][0].any() and st["grad"][1, 1] == 0 and st["grad"][2, 0] == 0 and not st["grad"][3].any()
    assert st["term"][0] == 0 and st["grad"][1, 0] != 0
    assert d[0, 7] == F(1.5)


@pytest.mark.parametrize("nonfinite", [False, True])
def test_nan_and_inf_composited_normal(nonfinite):
    R = 66
    c = NS.make_inputs(R, 7, 4, seed=3)
    c["valid_depth"][[4, 9, 65]] = 1.0
    c["valid_normal"][[4, 9, 65]] = 1.0
    c["acc"][4, 5] = np.nan
    c["acc"][9, 4] = np.inf
    c["acc"][65, 6] = -np.inf
    st, d, rl, _ = check(c, 4, nonfinite=nonfinite)
    if nonfinite:      # counted, and nothing added: the rows keep the bits they had
        assert st["dropped"] == (1, 2) and not st["touched"][[4, 9, 65]].any()
        assert np.isfinite(rl).all()
    else:              # the term reaches the loss; the gradient follows the comparisons (0 at the NaN component, finite at the inf ones)
        assert np.isnan(rl[4]) and np.isinf(rl[9]) and np.isinf(rl[65])
        assert st["grad"][4, 1] == 0 and st["grad"][4, 0] != 0 and np.isfinite(st["grad"][[4, 9, 65]]).all()
        assert st["grad"][9, 0] > 0 and st["grad"][65, 2] < 0
        assert np.isfinite(d).all()


@pytest.mark.parametrize("slots", [1, 64])
def test_loss_acc_sums_to_the_ray_loss_total(slots):
    """The atomics' total against the float64 sum of the per-ray terms: n_sel non-negative float32 terms added in any order, each
    addition rounding once -> (n_sel + 1) 2^-24 relative."""
    R = 1000
    c = NS.make_inputs(R, 7, 4, seed=21)
    c["ray_loss"][:] = 0.0
    st, _, rl, la = check(c, 4, slots=slots)
    total = float(st["term"].astype(np.float64).sum())
    assert total > 0 and abs(float(la.astype(np.float64).sum()) - total) <= (st["n_sel"] + 1) * 2.0 ** -24 * total
    assert abs(float(rl.astype(np.float64).sum()) - total) == 0.0


def test_refusals_return_einval_and_launch_nothing():
    from brdf_nerf_amd import _lib as L
    from brdf_nerf_amd import functions as Fn
    R, C_, ch = 40, 7, 4
    c = NS.make_inputs(R, C_, ch, seed=1)
    c["valid_depth"][:] = 1.0
    t = {k: torch.from_numpy(v).to(DEV) for k, v in c.items()}
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())
    good = dict(acc=p(t["acc"]), C=C_, ch=ch, normals=p(t["normals"]), ns=3, vn=p(t["valid_normal"]), vns=1, vd=p(t["valid_depth"]),
                vds=1, lam=0.3, R=R, d_acc=p(t["d_acc"]), ray_loss=p(t["ray_loss"]), loss_acc=None, slots=0, nonfinite=None,
                count=p(count))
    bad = [dict(acc=None), dict(normals=None), dict(vn=None), dict(vd=None), dict(d_acc=None), dict(count=None), dict(R=0), dict(R=-1),
           dict(R=(1 << 30) + 1), dict(C=3), dict(C=33), dict(ch=-1), dict(ch=C_ - 2), dict(lam=float("nan")), dict(lam=float("inf")),
           dict(ns=-3), dict(vns=-1), dict(vds=-1)]
    for over in bad:
        a = dict(good, **over)
        status = L.lib().bn_normal_target_loss(a["acc"], a["C"], a["ch"], a["normals"], a["ns"], a["vn"], a["vns"], a["vd"], a["vds"],
                                               a["lam"], a["R"], a["d_acc"], a["ray_loss"], a["loss_acc"], a["slots"], a["nonfinite"],
                                               a["count"], Fn._stream())
        assert status == -1, over                          # BN_EINVAL
        assert b"normal_target_loss" in L.lib().bn_last_error()
    torch.cuda.synchronize()
    assert int(count.item()) == -7
    assert (NS.bits(t["d_acc"].cpu().numpy()) == NS.bits(c["d_acc"])).all()
    assert (NS.bits(t["ray_loss"].cpu().numpy()) == NS.bits(c["ray_loss"])).all()
    # and the same arguments unchanged are served
    a = good
    assert L.lib().bn_normal_target_loss(a["acc"], a["C"], a["ch"], a["normals"], a["ns"], a["vn"], a["vns"], a["vd"], a["vds"],
                                         a["lam"], a["R"], a["d_acc"], a["ray_loss"], a["loss_acc"], a["slots"], a["nonfinite"],
                                         a["count"], Fn._stream()) == 0
    torch.cuda.synchronize()
    assert int(count.item()) == R
