"""Point sets in RAY form (rays + depths) whose points o + d z are exact fp32 values, for the tests that hold the raw field
entry points on the forms the training step uses (tests/test_gpu_point_sets.py) to the xyz form the exact tests pin.

A set is R rays with two sample blocks: z (R, S), then z2 (R, G).  Its points in row order are block 1 ray-major, then
block 2 ray-major - the order in which two forward launches at point_offset 0 and R S fill one output array, and in which
the two-block backward walks them (bn_points.seg1_points).  Everything sits on a dyadic grid:
    o in multiples of 2^-6 within [-0.5, 0.5],  d in multiples of 2^-4 within [-1, 1] (not normalised),
    z in multiples of 2^-6 within [0, 0.5),
so d z is an integer multiple of 2^-10 below 2^9 quanta and o + d z one below 2^10: exact in fp32 whether a kernel forms it
with an fma or with a multiply and an add, and the xyz-form reference receives the very same bits.  The premises are
asserted by tests/test_point_sets_cpu.py; nothing here needs a GPU."""
import numpy as np
import torch

import lattice_cases as LC

TILE = {"fp32": 64, "bf16": 128, "fp16": 128}
# name -> (R, S, G): what each shape reaches is tabulated in tests/test_gpu_point_sets.py
SETS = {"A": (16, 8, 5), "B": (32, 12, 7), "C": (64, 10, 8), "D": (13, 5, 3)}
S_NE_G = ("A", "B", "C", "D")        # sets that claim S != G
MERGEABLE = ("A", "B", "C")          # R S is a multiple of every mode's tile: the second launch may start there
QO, QD, QZ = 2.0 ** -6, 2.0 ** -4, 2.0 ** -6


def ray_set(name, stride=11):
    """-> dict(rays (R, stride), z (R, S), z2 (R, G)) in float64, every entry on its grid.  Columns 6.. of the rays (near, far,
    sun direction in the satellite layout) are filled with dyadic values the field never reads."""
    R, S, G = SETS[name]
    rng = np.random.default_rng(4000 + sum(map(ord, name)) + stride)
    o = rng.integers(-32, 33, size=(R, 3)) * QO
    d = rng.integers(-16, 17, size=(R, 3)) * QD
    for r in range(R):                       # a zero direction would put all of a ray's samples on one point
        while not d[r].any():
            d[r] = rng.integers(-16, 17, size=3) * QD
    zi = np.stack([rng.permutation(32)[:S + G] for _ in range(R)])           # no depth twice on a ray, over both blocks
    z, z2 = np.sort(zi[:, :S], 1) * QZ, np.sort(zi[:, S:], 1) * QZ
    rest = rng.integers(-16, 17, size=(R, stride - 6)) * QD
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    return dict(rays=tt(np.concatenate([o, d, rest], 1)), z=tt(z), z2=tt(z2))


def block_points(rays, z):
    """(R S, 3) points o + d z of one block, ray-major, and each point's direction, in the dtype of the inputs."""
    o, d = rays[:, None, 0:3], rays[:, None, 3:6]
    x = o + d * z[:, :, None]
    return x.reshape(-1, 3).contiguous(), d.expand(-1, z.shape[1], -1).reshape(-1, 3).contiguous()


def set_points(rs):
    """X (n_all, 3) and dirs (n_all, 3) of a set in row order: block 1, then block 2."""
    x1, d1 = block_points(rs["rays"], rs["z"])
    x2, d2 = block_points(rs["rays"], rs["z2"])
    return torch.cat([x1, x2]).contiguous(), torch.cat([d1, d2]).contiguous()


def ray_embedding(name, t_dim):
    """A per-ray image embedding (R, t_dim), float32 values."""
    g = torch.Generator().manual_seed(77 + sum(map(ord, name)))
    return torch.randn(SETS[name][0], t_dim, generator=g)


# ------------------------------------------------------------------------------------------------ lattice cases in set form
# (case of tests/lattice_cases.py, B): B in (600, 1100) as case_sizes() offers them, one without and one with analytic normals
LATTICE = [("lambert_F64_L8", 600), ("rpv_an_F128_L4", 1100)]


def split_point(B):
    """The multiple of 128 (a tile multiple in every mode) nearest to B / 2."""
    return int(round(B / 2 / 128)) * 128


def lattice_ray_blocks(name, B):
    """The lattice points of a case as ONE-sample rays in two blocks over the same rays (property 9).  Two blocks share their
    rays, and the second launch starts at a tile multiple, so the set has 2 R points with R = split_point(B): the first 2 R
    points of the case.  Ray r carries point r at depth z = 1 and point R + r at depth z2 = 2:
        d_r = x_{R+r} - x_r,  o_r = x_r - d_r      (multiples of Q0 = 1/8 with |d| <= 2, |o| <= 3: every operation exact)
    -> dict(rays (R, 11), z (R, 1), z2 (R, 1), n (= 2 R)) in float64."""
    case = LC.get_case(name)
    assert case.pts[1] is None, "a case with view directions fixes d: not served here"
    R = split_point(B)
    assert 2 * R <= LC.N_MAX
    x = case.pts[0]
    d = x[R:2 * R] - x[:R]
    o = x[:R] - d
    rays = torch.cat([o, d, torch.zeros(R, 5, dtype=torch.float64)], 1).contiguous()
    return dict(rays=rays, z=torch.ones(R, 1, dtype=torch.float64), z2=torch.full((R, 1), 2.0, dtype=torch.float64), n=2 * R)


# the `+=` contract of bn_field_grads: accumulators preloaded with a lattice-valued constant before the first call of the
# accumulation test, one per kernel that adds into a gradient (wgrad_reduce_kernel, skinny_reduce_kernel, bn_unfold_heads)
PRELOAD = {"fc_net.2.weight": 4.0, "sigma_from_xyz.0.weight": 8.0, "rgb_from_xyzdir.0.bias": 2.0}
