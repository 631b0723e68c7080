"""The oracle against the REFERENCE ITSELF on random configurations.

The golden fixtures pin the oracle on the reference's own shapes; tests/test_gpu_fuzz.py then uses the oracle as the checker on
RANDOM shapes and flag sets.  This closes the loop: on the same family of random configurations the oracle must reproduce the
reference - field forward and every parameter gradient, and the full render_rays dictionary with the reference's own random
draws recorded and replayed.  The configurations, their inputs and the reference's outputs are stored in
tests/golden/random_{field,render}_*.npz (tests/golden/make_goldens.py --only-random-configs runs the reference to write them)."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden, tparams, replay_list
from oracle.config import FieldConfig
from oracle import field as OF
from oracle import render as ORD


def load_case(kind, seed, seeds_per_file=4):
    lo = seed // seeds_per_file * seeds_per_file
    gold = load_golden(f"random_{kind}_{lo:02d}_{lo + seeds_per_file - 1:02d}")
    pre = f"s{seed}/"
    case = {k[len(pre):]: v for k, v in gold.items() if k.startswith(pre)}
    assert case, f"no case {seed} in the {kind} fixtures"
    kw = json.loads(str(case["cfg"]))
    kw["skips"] = tuple(kw["skips"])
    cfg = FieldConfig(**kw)
    p = tparams(cfg, int(case["param_seed"]))
    csum = float(sum(v.double().sum() for v in p.values()))
    assert abs(csum - float(case["param_checksum"])) <= 1e-9 * max(1.0, abs(csum)), "make_params drifted from the fixture's"
    return case, cfg, p


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("seed", list(range(16)))
def test_oracle_field_matches_reference_on_random_configurations(seed):
    case, cfg, p = load_case("field", seed)
    flags = json.loads(str(case["flags"]))
    xyz, dirs, t_in, coef, out_ref = (t(case[k]) for k in ("xyz", "dirs", "t_in", "coef", "out"))
    for v in p.values():
        v.requires_grad_(True)
    t_or = t_in.clone().requires_grad_(True)
    out = OF.field_forward(p, cfg, xyz, dirs=dirs if cfg.dir_dim else None, t_embed=t_or if cfg.beta else None, **flags)
    tag = f"seed {seed}: {cfg}"
    assert out.shape == out_ref.shape, tag
    assert float((out - out_ref).detach().abs().max()) <= 2e-5 * float(out_ref.abs().max()) + 2e-6, tag
    (out * coef).sum().backward()
    if cfg.beta:
        t_grad = t(case["t_grad"])
        assert float((t_or.grad - t_grad).abs().max()) <= 1e-4 * float(t_grad.abs().max()) + 1e-9, tag
    for k, v in p.items():
        if "grad/" + k not in case:
            assert v.grad is None or float(v.grad.abs().max()) == 0.0, f"{tag}: {k}"
            continue
        gr = t(case["grad/" + k])
        scale = float(gr.abs().max())
        assert float((v.grad - gr).abs().max()) <= 2e-4 * scale + 1e-9, f"{tag}: {k}"


@pytest.mark.parametrize("seed", list(range(12)))
def test_oracle_render_rays_matches_reference_on_random_configurations(seed):
    case, cfg, p = load_case("render", seed)
    flags = json.loads(str(case["flags"]))
    mode = str(case["mode"])
    rays = t(case["rays"])
    dk = {k[3:]: t(v) for k, v in case.items() if k.startswith("dk/")}
    rays_t = t(case["emb"])[t(case["ts"])] if cfg.beta else None
    res = {k: t(case["res/" + k]) for k in str(case["res_keys"]).split("\n")}
    bt = json.loads(str(case["brdf_type"]))
    with torch.no_grad():
        got, bt2 = ORD.render_rays(p, cfg, rays, ORD.Randoms(replay=replay_list(case)), mode=mode, rays_t=rays_t, **flags, **dk)
    tag = f"seed {seed}: {cfg} {mode} {flags} prior={bool(dk)}"
    assert bt == bt2, tag
    assert set(res) == {k for k in got if not k.startswith("_")}, (tag, sorted(set(res) ^ {k for k in got if not k.startswith('_')}))
    for k, v in res.items():
        a = got[k]
        if k == "sort_idx_coarse":
            assert torch.equal(a, v), f"{tag}: {k}"
            continue
        fin = torch.isfinite(v)
        assert torch.equal(fin, torch.isfinite(a)), f"{tag}: {k} finiteness"
        if k == "hpk_scl_coarse":
            a, v = 1.0 / a, 1.0 / v
        e = float((a[fin] - v[fin]).abs().max()) if bool(fin.any()) else 0.0
        assert e <= 1e-4 * float(v[fin].abs().max() if bool(fin.any()) else 0.0) + 2e-5, f"{tag}: {k} err {e:.2e}"
