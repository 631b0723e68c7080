"""The compositing entry points share ONE recurrence (csrc/composite_ray.h): on the same depths and rows, without noise,
bn_composite_forward, bn_merged_composite_forward on a single block (no sort index, S1 == S2) and the pass-1 compositing of
bn_composite_guided give the same alphas, transparencies, weights and depth BIT FOR BIT - at one lane, a partly filled last lane,
cpl 1 -> 2, an odd cpl with a ragged tail and the largest S, on R = 5 rays (not a multiple of the four waves of a block), with the
C = 4 row kept in registers and with C = 13 strided rows.

Not compared: acc (the flat channel path of bn_composite_forward adds up in another order) and the sun kernel (a serial product).
bn_composite_guided merges S + G <= 512 positions with G >= 3, so it does not take S = 512: there the test holds the first two to
each other and checks that the third refuses the shape."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_kernel_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R, G = 5, 3
S_LIST = (1, 63, 64, 65, 449, 512)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(tag, a, b):
    n = int((_bits(a) != _bits(b)).sum())
    assert n == 0, f"{tag}: {n} of {a.numel()} values differ, largest difference {float((a.double() - b.double()).abs().max()):.3e}"


@pytest.mark.parametrize("pattern", ("moderate", "negative", "opaque_last"))
@pytest.mark.parametrize("C", (4, 13))
@pytest.mark.parametrize("S", S_LIST)
def test_entry_points_composite_alike(S, C, pattern):
    from brdf_nerf_amd import functions as Fn
    g = torch.Generator().manual_seed(7000 + 64 * S + C)
    z = torch.sort(torch.rand(R, S, generator=g) * K.FAR, -1)[0]
    rows = torch.rand(R, S, C, generator=g)
    for r in range(R):
        rows[r, :, 3] = K._sigma_pattern(pattern, z[r], g)
    z, rows = z.to(DEV).contiguous(), rows.to(DEV).contiguous()
    alphas, trans, weights, depth, _ = Fn.composite_forward_raw(z, rows)
    assert float(weights.sum()) > 0 and bool(torch.isfinite(weights).all())
    m = Fn.merged_composite_forward(z, None, rows, None, want=("alphas", "trans", "weights", "depth"))
    tag = f"S={S} C={C} {pattern}"
    for k, v in (("alphas", alphas), ("trans", trans), ("weights", weights), ("depth", depth)):
        _same(f"{tag}: {k}, composite_forward against merged_composite_forward", v, m[k])
    nf = torch.tensor([0.0, K.FAR], device=DEV)
    u = torch.rand(R, G, generator=g).to(DEV)
    if S + G > 512:
        with pytest.raises(RuntimeError, match="composite_guided"):
            Fn.composite_guided(z, rows, G, nf, 3.0, u=u, want_pass1=True)
        return
    w1, d1 = Fn.composite_guided(z, rows, G, nf, 3.0, u=u, want_pass1=True)[3:]
    _same(f"{tag}: weights, composite_forward against composite_guided", weights, w1)
    _same(f"{tag}: depth, composite_forward against composite_guided", depth, d1)
