#!/usr/bin/env python3
"""Golden vectors of NormalLoss(keyword='an') (metrics.py:218-261, --nr_spv_type 3), made by running the REFERENCE on the CPU.

    python tests/golden/make_normal_spv_goldens.py        (build container only: it imports the reference as make_goldens.py does)

Writes normal_spv.npz beside this file: inputs, loss and the gradients w.r.t. normal_pred and weights of
  ps_*     a per-sample input of 96 rays x 12 samples;
  r<R>_*   the one-sample form weights = 1, normal_pred = acc[:, None] - what the fused step's kernel sees - at
           R in {1, 63, 64, 65, 257, 1000}.
The inputs are asserted to exercise the rule: enough selected rays, selected rays with valid_normal == 0 (they count in the mean and
contribute 0), unselected rays with valid_normal == 1 (they must not count), planted exact zeros of e_c, and no other |e_c| near 0
(there the sign of a one-ulp difference would decide the gradient).  Nothing of the reference is copied: it is fed and recorded."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import import_reference, quiet, save  # noqa: E402

LAMBDA = 0.1
ONE_SAMPLE_R = (1, 63, 64, 65, 257, 1000)


def make_case(R, S, seed):
    g = torch.Generator().manual_seed(seed)
    if S == 1:
        w = torch.ones(R, 1)
    else:
        w = torch.rand(R, S, generator=g)
        w = w / w.sum(-1, keepdim=True) * torch.rand(R, 1, generator=g)
    pred = torch.randn(R, S, 3, generator=g)
    gt = torch.randn(R, 3, generator=g)
    gt = gt / gt.norm(dim=-1, keepdim=True)
    valid = (torch.rand(R, generator=g) < 0.6).float()
    vn = (torch.rand(R, generator=g) < 0.6).float()
    planted = np.zeros((R, 3), bool)
    if R == 1:
        valid[:] = 1.0
        vn[:] = 1.0
    else:
        # make sure of the four kinds of ray, whatever the draw
        valid[:20] = torch.tensor([1.0] * 14 + [0.0] * 6)
        vn[:20] = torch.tensor([1.0] * 7 + [0.0] * 7 + [1.0] * 6)
        if S == 1:
            # planted exact zeros: e_c = vn n - vn n on a selected ray with valid_normal == 1, one and all three components
            pred[0, 0, 1] = gt[0, 1]
            pred[1, 0, :] = gt[1]
            planted[0, 1] = True
            planted[1, :] = True
    return w, pred, gt, vn, valid, planted


def check_inputs(R, w, pred, gt, vn, valid, planted):
    sel = valid > 0
    n_sel = int(sel.sum())
    if R >= 63:
        assert n_sel >= 10, n_sel
        assert int((sel & (vn == 0)).sum()) >= 5 and int((~sel & (vn == 1)).sum()) >= 5
    pred_s = (w.unsqueeze(-1) * pred).sum(-2)
    e = (vn[:, None] * gt - vn[:, None] * pred_s).numpy()
    live = (sel & (vn > 0)).numpy()[:, None] & ~planted
    assert (np.abs(e[live]) >= 1e-5).all(), np.abs(e[live]).min()
    assert (e[planted] == 0).all()
    return n_sel


def run(ref, w, pred, gt, vn, valid):
    w = w.clone().requires_grad_(True)
    pred = pred.clone().requires_grad_(True)
    loss, _ = quiet(ref["metrics"].NormalLoss(lambda_nr_spv=LAMBDA), w, gt, pred, target_weight=vn, target_valid_depth=valid,
                    keyword="an")
    loss.backward()
    return loss.detach(), pred.grad, w.grad


if __name__ == "__main__":
    torch.set_num_threads(1)
    ref = import_reference()
    out = {"lambda": torch.tensor(LAMBDA, dtype=torch.float64), "one_sample_R": torch.tensor(ONE_SAMPLE_R)}
    cases = [("ps", 96, 12, 301)] + [(f"r{R}", R, 1, 400 + R) for R in ONE_SAMPLE_R]
    for name, R, S, seed in cases:
        w, pred, gt, vn, valid, planted = make_case(R, S, seed)
        n_sel = check_inputs(R, w, pred, gt, vn, valid, planted)
        loss, d_pred, d_w = run(ref, w, pred, gt, vn, valid)
        assert torch.isfinite(loss) and torch.isfinite(d_pred).all() and torch.isfinite(d_w).all()
        out.update({f"{name}_weights": w, f"{name}_normal_pred": pred, f"{name}_normal_gt": gt, f"{name}_valid_normal": vn,
                    f"{name}_valid_depth": valid, f"{name}_planted": torch.from_numpy(planted), f"{name}_loss": loss,
                    f"{name}_d_normal_pred": d_pred, f"{name}_d_weights": d_w, f"{name}_n_sel": torch.tensor(n_sel)})
    save("normal_spv", **out)
