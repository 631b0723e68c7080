"""CPU side of relighting with cast shadows (brdf_nerf_amd/shadows.py, bn_sun_ray_table / bn_sun_shade_dirs): the argument
checks, which run before any device work; the refusals of the unshadowed calls, which stay; and the float64 statement of
transmittance + shading (tests/relight_shadow_cases.py) pinned to the oracle's own --sun_v analystic render and checked against
the oracle's own precision on exactly the inputs of the GPU comparison."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relight_cases as RC  # noqa: E402
import relight_shadow_cases as HC  # noqa: E402
from test_host_cpu import make_args  # noqa: E402

R_CPU, SEED = 24, 3
_RENDERS = {}


def _models(cfg_kw, **over):
    from brdf_nerf_amd import load_model
    from oracle.config import FieldConfig
    cfg = FieldConfig(feat=64, n_samples=16, guided_samples=16, **cfg_kw)
    args = make_args(cfg, **over)
    return {"coarse": load_model(args)}, args


def test_a_model_without_the_sun_pass_is_pointed_at_relight_image():
    """ValueError naming sun_v and relight_image from every entry that renders: model and rays are on the CPU."""
    from brdf_nerf_amd import relight_image_shadowed, render_shadow_surface
    models, args = _models(dict(funcM=1, funcF=1, funcH=1, normal="analystic"))
    rays = torch.zeros(8, 11)
    for call in (lambda: relight_image_shadowed(models, args, rays, RC.sun_directions()), lambda: render_shadow_surface(models, args, rays)):
        with pytest.raises(ValueError, match="sun_v") as e:
            call()
        assert "relight_image" in str(e.value)


def test_without_a_brdf_there_is_no_sun_pass():
    """apply_brdf=False: ValueError - the reference runs no sun pass then (rendering.py:244)."""
    from brdf_nerf_amd import relight_image_shadowed, render_shadow_surface
    models, args = _models(dict(funcM=1, funcF=1, funcH=1, normal="analystic"), sun_v="analystic")
    rays = torch.zeros(8, 11)
    with pytest.raises(ValueError, match="apply_brdf"):
        relight_image_shadowed(models, args, rays, RC.sun_directions(), apply_brdf=False)
    with pytest.raises(ValueError, match="apply_brdf"):
        render_shadow_surface(models, args, rays, apply_brdf=False)


@pytest.mark.parametrize("over,kw,flag", [(dict(sun_v="analystic"), {}, "sun_v analystic"), (dict(), dict(gsam_only=True), "gsam_only")])
def test_the_unshadowed_calls_still_refuse_by_name(over, kw, flag):
    from brdf_nerf_amd import relight_image, render_surface
    models, args = _models(dict(funcM=1, funcF=1, funcH=1, normal="learned"), **over)
    rays = torch.zeros(8, 11)
    with pytest.raises(NotImplementedError, match=flag):
        relight_image(models, args, rays, RC.sun_directions(), **kw)
    with pytest.raises(NotImplementedError, match=flag):
        render_surface(models, args, rays, **kw)


def _render(name):
    """The oracle's render of a case under the six suns (shared by the tests below, unchanged by them)."""
    if name not in _RENDERS:
        from brdf_nerf_amd.raytable import synthetic_table
        rays = synthetic_table(R_CPU, device="cpu", seed=RC.RAYS_SEED).data["rays"]
        _RENDERS[name] = HC.oracle_render(name, rays, RC.sun_directions(), SEED)
    return _RENDERS[name]


def _statement(name, o, dtype):
    cfg = HC.config(name)
    src = dict(rows=o["rows"], weights=o["weights"]) if HC.per_sample(name) else dict(acc=o["acc"], wsum=o["wsum"])
    return HC.oracle_sun_shade(cfg, o["sigma_sun"], o["z_sun"], RC.sun_directions(), o["rays_d"], dtype=dtype, **src)


@pytest.mark.parametrize("name", [n for n in HC.CASES if not HC.cos_on(n)])
def test_statement_matches_the_oracles_own_shadowed_render(name):
    """oracle/render.py's render_rays(gsam_only=True) of a --sun_v analystic model with sun k written into the rays, against the
    shared statement on the sun pass rebuilt from that render's pass-1 depth and uniforms: rgb_coarse and sun_coarse[:, -1, 0],
    float64, 1e-10."""
    o = _render(name)
    rgb, vis = _statement(name, o, torch.float64)
    assert bool(torch.isfinite(o["rgb"]).all()) and bool(torch.isfinite(rgb).all())
    err_rgb, err_vis = float((rgb - o["rgb"]).abs().max()), float((vis - o["vis"]).abs().max())
    print(f"{name}: max |statement - oracle render| rgb {err_rgb:.3e}, visibility {err_vis:.3e}; visibility in "
          f"[{float(vis.min()):.3f}, {float(vis.max()):.3f}]")
    assert err_rgb <= 1e-10 and err_vis <= 1e-10, (name, err_rgb, err_vis)
    assert float(vis.max()) - float(vis.min()) > 0.05, "the suns cast no shadow on these rays: the comparison would show nothing"


@pytest.mark.parametrize("name", [n for n in HC.CASES if not HC.cos_on(n)])
def test_float32_evaluation_stays_within_half_the_tolerance(name):
    """On the oracle's own render of each case: the statement evaluated in float32 agrees with itself in float64 within HALF of
    ORACLE_TOL, rgb and visibility, every (ray, direction) - the tolerance of the GPU comparison is reachable by a correct
    float32 kernel on these inputs."""
    o = _render(name)
    rtol, atol = HC.tolerance(name)
    got64, got32 = _statement(name, o, torch.float64), _statement(name, o, torch.float32)
    for what, a64, a32 in zip(("rgb", "vis"), got64, got32):
        assert bool(torch.isfinite(a64).all()), f"{name} {what}: oracle not finite"
        ratio = float(((a32.double() - a64).abs() / (atol + rtol * a64.abs())).max())
        print(f"{name} {what}: float32 against float64, max err / tol = {ratio:.3f}")
        assert ratio <= 0.5, (name, what, ratio)
