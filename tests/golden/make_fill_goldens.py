#!/usr/bin/env python
"""Generate the hole-filling goldens (tests/golden/fill_*.npz) by running the REFERENCE's eval.py on synthetic grids.

Run only where the reference tree is present (BRDFNERF_REFERENCE, default /root/reference, read-only) and scipy is installed:

    python tests/golden/make_fill_goldens.py

eval.py is imported with empty stub modules for the imports that drag in the model or that the machine may lack (train_utils,
models, rendering, metrics, sat_utils, opt; yaml when it is missing), as make_dsmr_goldens.py stubs numba and rasterio: they are
used only inside other functions.  Its quickly_interpolate_nans_from_singlechannel_img - scipy's griddata(method='nearest') -
then runs on float32 grids as save_dsm_grid runs it on a float32 raster.

Recorded per fixture: `u` the input (NaN = hole) and `ref` the reference's output, both float32.  The surfaces are those of
make_dsmr_goldens.surface (smooth + steps + noise) in multiples of 2^-6 m, so that the files compress.

CONDITIONS ON THE INPUTS (not a tolerance on any code), so that the comparison of tests/fill_cases.against_reference cannot go
vacuous: every fixture has at least 400 holes whose nearest known cell is unique (compared bit for bit) and at least 200 holes
with several known cells at the minimal distance (where upstream's k-d tree picks one by its traversal order and only
membership can be compared).
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fill_cases as F  # noqa: E402

REF = os.environ.get("BRDFNERF_REFERENCE", "/root/reference")
MIN_UNIQUE, MIN_TIES = 400, 200

# name: (H, W, fraction of random NaN cells, NaN patch (rows, columns) or None, seed)
FIXTURES = {
    "holes5": (60, 72, 0.05, (17, 29), 31),
    "holes30": (104, 112, 0.30, (17, 29), 32),
    "sparse90": (96, 130, 0.90, None, 33),
}


def load_eval():
    stubs = {"train_utils": {}, "models": {"load_model": None}, "rendering": {"render_rays": None}, "metrics": {}, "sat_utils": {},
             "opt": {"Test_parser": None, "printArgs": None}}
    try:
        import yaml  # noqa: F401
    except ImportError:
        stubs["yaml"] = {}
    for name, attrs in stubs.items():
        mod = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(mod, k, v)
        sys.modules[name] = mod
    sys.path.insert(0, REF)
    return importlib.import_module("eval")


def grid(H, W, frac, patch, seed):
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    f = 40.0 + 4.0 * np.sin(jj / 17.0) * np.cos(ii / 23.0) + 0.02 * ii
    for _ in range(12):
        r0, c0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
        f[r0:r0 + rng.integers(6, 24), c0:c0 + rng.integers(6, 24)] += rng.uniform(3.0, 15.0)
    f = f + 0.05 * rng.standard_normal((H, W))
    u = (np.round(f * 64.0) / 64.0).astype(np.float32)
    u[rng.random((H, W)) < frac] = np.nan
    if patch is not None:
        u[H // 3:H // 3 + patch[0], W // 4:W // 4 + patch[1]] = np.nan
    return u


def run(mod, name):
    u = grid(*FIXTURES[name])
    ref = mod.quickly_interpolate_nans_from_singlechannel_img(u.copy())
    assert ref.dtype == np.float32 and ref.shape == u.shape
    _, _, mult = F.unique_and_ties(u)
    unique, ties = int((mult == 1).sum()), int((mult > 1).sum())
    assert unique >= MIN_UNIQUE and ties >= MIN_TIES, f"{name}: {unique} unique-nearest holes, {ties} tie holes: choose other inputs"
    filled, _, dist2 = F.statement(u)
    assert F.against_reference(u, filled, dist2, ref) == (unique, ties)
    path = os.path.join(HERE, f"fill_{name}.npz")
    np.savez_compressed(path, u=u, ref=ref)
    print(f"{name}: {u.shape[0]} x {u.shape[1]}, {mult.size} holes, {unique} with a unique nearest cell, {ties} ties, "
          f"largest d2 {int(dist2.max())}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    module = load_eval()
    for fixture in (sys.argv[1:] or FIXTURES):
        run(module, fixture)
