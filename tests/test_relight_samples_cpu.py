"""CPU side of per-sample relighting (brdf_nerf_amd/relight.py per_sample=True, bn_sample_shade_dirs): the float64 statement of
the per-sample shading pinned to the oracle's own --MultiBRDF render, the fixed inputs of the GPU tests checked against the
oracle's own precision, and the opt-in's argument checks, which run before any device work."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relight_cases as RC  # noqa: E402
import relight_sample_cases as SC  # noqa: E402
from test_host_cpu import make_args  # noqa: E402

# shapes of the GPU oracle test (tests/test_gpu_relight_samples.py)
R_SYN, S_SYN, SEED_SYN = 130, 21, 5


@pytest.mark.parametrize("name", list(SC.CASES))
def test_helper_matches_the_oracles_own_multibrdf_render(name):
    """oracle/render.py's render_rays of a --MultiBRDF model (pinned by the goldens) with sun k written into the rays, against
    oracle_sample_shade on that render's per-sample outputs and weights: float64, 1e-10."""
    from brdf_nerf_amd.raytable import synthetic_table
    from oracle import render as ORD
    cfg = SC.config(name)
    fl = SC.flags(name)
    p = {k: torch.from_numpy(v).double() for k, v in RC.level_normals(cfg.make_params(RC.MODEL_SEED)).items()}
    rays = synthetic_table(24, device="cpu", seed=RC.RAYS_SEED).data["rays"].double()
    suns = RC.sun_directions().double()
    for k in range(suns.shape[0]):
        r = rays.clone()
        r[:, 8:11] = suns[k]
        g = torch.Generator().manual_seed(3)
        res, _ = ORD.render_rays(p, cfg, r, ORD.Randoms(generator=g), mode="test", **fl)
        rows, w = SC.oracle_rows(cfg, res, fl["apply_brdf"], fl["apply_theta"])
        rgb, _ = SC.oracle_sample_shade(cfg, rows, w, r[:, 3:6], suns[k:k + 1], None, fl)
        want = res["rgb_coarse"].detach()
        assert bool(torch.isfinite(want).all())
        err = float((rgb[0] - want).abs().max())
        print(f"{name} sun {k}: max |helper - oracle render| = {err:.3e}")
        assert err <= 1e-10, (name, k, err)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_fixed_inputs_are_within_the_oracles_own_precision(name):
    """The synthetic rows and direction lists of the GPU oracle test: oracle_sample_shade is finite at every entry, and evaluated
    in float32 it agrees with itself in float64 within HALF the tolerance the GPU test uses - rgb and brdf, every entry."""
    cfg = SC.config(name)
    fl = SC.flags(name)
    rtol, atol = SC.tolerance(name)
    rows, w, rays_d = SC.synthetic_rows(name, R_SYN, S_SYN, SEED_SYN)
    assert SC.sun_directions_many().shape == (SC.N_SUN, 3) and SC.N_SUN > 64
    for mode, sun, view in (("sun", SC.sun_directions_many(), None), ("lobe",) + SC.lobe_pairs()):
        got64 = SC.oracle_sample_shade(cfg, rows, w, rays_d, sun, view, fl)
        got32 = SC.oracle_sample_shade(cfg, rows, w, rays_d, sun, view, fl, dtype=torch.float32)
        for what, a64, a32 in zip(("rgb", "brdf"), got64, got32):
            assert tuple(a64.shape) == (sun.shape[0], R_SYN, 3)
            assert bool(torch.isfinite(a64).all()), f"{name} {mode} {what}: oracle not finite"
            ratio = float(((a32.double() - a64).abs() / (atol + rtol * a64.abs())).max())
            print(f"{name} {mode} {what}: float32 against float64, max err / tol = {ratio:.3f}")
            assert ratio <= 0.5, (name, mode, what, ratio)


def _models(cfg_kw, **over):
    from brdf_nerf_amd import load_model
    from oracle.config import FieldConfig
    cfg = FieldConfig(feat=64, n_samples=16, guided_samples=16, **cfg_kw)
    args = make_args(cfg, **over)
    return {"coarse": load_model(args)}, args


@pytest.mark.parametrize("over,kw,flag", [(dict(MultiBRDF=1, sun_v="analystic"), {}, "sun_v analystic"),
                                          (dict(MultiBRDF=1), dict(gsam_only=True), "gsam_only")])
def test_per_sample_still_refuses_by_name(over, kw, flag):
    """NotImplementedError naming the flag from relight_image and render_surface alike: model and rays are on the CPU."""
    from brdf_nerf_amd import relight_image, render_surface
    models, args = _models(dict(funcM=1, funcF=1, funcH=1, normal="learned"), **over)
    rays = torch.zeros(8, 11)
    with pytest.raises(NotImplementedError, match=flag):
        relight_image(models, args, rays, RC.sun_directions(), per_sample=True, **kw)
    with pytest.raises(NotImplementedError, match=flag):
        render_surface(models, args, rays, per_sample=True, **kw)


def test_per_sample_needs_a_multibrdf_model():
    """ValueError on a model with one BRDF per ray: a sum of per-sample BRDF values would not be render_rays' result."""
    from brdf_nerf_amd import relight_image, render_surface
    models, args = _models(dict(funcM=1, funcF=1, funcH=1, normal="learned"))
    rays = torch.zeros(8, 11)
    with pytest.raises(ValueError, match="MultiBRDF"):
        relight_image(models, args, rays, RC.sun_directions(), per_sample=True)
    with pytest.raises(ValueError, match="MultiBRDF"):
        render_surface(models, args, rays, per_sample=True)


def test_the_refusal_without_the_opt_in_points_at_it():
    from brdf_nerf_amd import render_surface
    models, args = _models(dict(funcM=1, funcF=1, funcH=1, normal="learned"), MultiBRDF=1)
    with pytest.raises(NotImplementedError, match="per_sample=True"):
        render_surface(models, args, torch.zeros(8, 11))
