"""CPU side of relighting (brdf_nerf_amd/relight.py): the angle convention, the refusals (argument checks that run before any
device work), and the fixed direction lists of the GPU tests checked against the oracle alone."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relight_cases as RC  # noqa: E402
from test_host_cpu import make_args  # noqa: E402


@pytest.mark.parametrize("el,az", [(0.0, 0.0), (0.0, 90.0), (30.0, 0.0), (45.0, 135.0), (62.5, 250.0), (90.0, 0.0), (90.0, 77.0)])
def test_directions_closed_form(el, az):
    from brdf_nerf_amd import directions
    d = directions(el, az)
    e, a = math.radians(el), math.radians(az)
    want = [math.sin(a) * math.cos(e), math.cos(a) * math.cos(e), math.sin(e)]
    assert d.dtype == torch.float32 and tuple(d.shape) == (3,)
    np.testing.assert_allclose(d.double().numpy(), want, rtol=0, atol=1e-7)
    assert abs(float(d.double().norm()) - 1.0) < 1e-6
    if el == 90.0:
        np.testing.assert_allclose(d.double().numpy(), [0.0, 0.0, 1.0], rtol=0, atol=1e-7)


def test_directions_broadcast_and_known_axes():
    from brdf_nerf_amd import directions
    d = directions(torch.tensor([[0.0], [30.0]]), torch.tensor([0.0, 90.0, 180.0]))
    assert tuple(d.shape) == (2, 3, 3)
    np.testing.assert_allclose(d[0].numpy(), [[0, 1, 0], [1, 0, 0], [0, -1, 0]], atol=1e-7)       # azimuth from +y towards +x
    np.testing.assert_allclose(d[1, :, 2].numpy(), [0.5, 0.5, 0.5], atol=1e-7)
    np.testing.assert_allclose(directions(25.0, 10.0).numpy(), np.float32(RC.unit(25, 10)), atol=1e-7)


@pytest.mark.parametrize("cfg_kw,over,kw,flag", [(dict(funcM=1, funcF=1, funcH=1, normal="learned"), dict(MultiBRDF=1), {}, "MultiBRDF"),
                                                 (dict(normal="learned"), dict(sun_v="analystic"), {}, "sun_v analystic"),
                                                 (dict(), dict(), dict(gsam_only=True), "gsam_only")])
def test_relighting_refuses_what_the_shortcut_does_not_cover(cfg_kw, over, kw, flag):
    """NotImplementedError naming the flag, from relight_image and render_surface alike, before any device work: the model and
    the rays are on the CPU here."""
    from brdf_nerf_amd import load_model, relight_image, render_surface
    from oracle.config import FieldConfig
    cfg = FieldConfig(feat=64, n_samples=16, guided_samples=16, **cfg_kw)
    args = make_args(cfg, **over)
    models = {"coarse": load_model(args)}
    rays = torch.zeros(8, 11)
    with pytest.raises(NotImplementedError, match=flag):
        relight_image(models, args, rays, RC.sun_directions(), **kw)
    with pytest.raises(NotImplementedError, match=flag):
        render_surface(models, args, rays, **kw)


@pytest.mark.parametrize("name", list(RC.CASES))
def test_oracle_is_finite_on_the_fixed_directions(name):
    """The direction lists of tests/test_gpu_relight.py, on the oracle's own render of the same rays and parameters (CPU,
    float64): finite for every (ray, direction), in sun mode and in lobe mode."""
    from brdf_nerf_amd.raytable import synthetic_table
    _, fl, _ = RC.CASES[name]
    cfg = RC.config(name)
    orig = cfg.make_params
    cfg.make_params = lambda seed=0: RC.level_normals(orig(seed))
    ab, at, ci = fl.get("apply_brdf", False), fl.get("apply_theta", False), fl.get("cos_irra_on", False)
    rays = synthetic_table(96, device="cpu", seed=RC.RAYS_SEED).data["rays"]
    acc, wsum, rays_d = RC.oracle_surface(cfg, rays, 3, ab, at)
    lobe = RC.lobe_directions()
    assert RC.sun_directions().shape[0] >= 5 and lobe.shape[0] == 32
    for sun, view in ((RC.sun_directions(), None), (torch.tensor([RC.unit(*RC.LOBE_SUN)]).expand(lobe.shape[0], 3), lobe)):
        rgb, brdf = RC.oracle_shade(cfg, acc, wsum, rays_d, sun, view, ab, at, ci)
        assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(brdf).all())


def _f32_against_f64(name, level, sun, view, n_rays=96):
    """max over (ray, direction, channel) of |oracle in float32 - oracle in float64| / (atol + rtol |float64|) for the case's
    tolerance, on the oracle's own surface: what ANY float32 implementation of these formulas can be expected to reach."""
    from brdf_nerf_amd.raytable import synthetic_table
    _, fl, kind = RC.CASES[name]
    cfg = RC.config(name)
    if level:
        orig = cfg.make_params
        cfg.make_params = lambda seed=0: RC.level_normals(orig(seed))
    ab, at, ci = fl.get("apply_brdf", False), fl.get("apply_theta", False), fl.get("cos_irra_on", False)
    rays = synthetic_table(n_rays, device="cpu", seed=RC.RAYS_SEED).data["rays"]
    acc, wsum, rays_d = RC.oracle_surface(cfg, rays, 3, ab, at)
    _, b64 = RC.oracle_shade(cfg, acc, wsum, rays_d, sun, view, ab, at, ci)
    _, b32 = RC.oracle_shade(cfg, acc.float(), wsum.float(), rays_d.float(), sun, view, ab, at, ci, dtype=torch.float32)
    rtol, atol = RC.ORACLE_TOL[kind]
    return float(((b32.double() - b64).abs() / (atol + rtol * b64.abs())).max())


def test_why_the_oracle_comparison_levels_the_normals_and_leaves_the_principal_plane_out():
    """The two narrowings of the GPU oracle test (relight_cases.level_normals, lobe_directions), shown with the oracle alone:
    oracle/brdf.py evaluated in float32 against itself in float64.
    - Freshly initialised learned normals face away from some sun for a fifth of the rays; cos(incidence) then sits on its 1e-5
      clamp and Hapke's 1 / cos(acos(1e-5)) loses the tolerance in float32 (measured 15 x).  With level normals it holds with
      a wide margin.  (rpv111 has analytic normals - no head to level - and RPV has no such term: it holds as it is.)
    - With Hapke's theta, a view in the principal plane opposite the sun has phi = pi, where exp(-2 tan((phi + 1e-5) / 2))
      jumps from 0 to inf (asserted on the function itself).  phi = pi is reached when the azimuth cosine rounds onto its -1 clamp,
      which the last bit of a ray's normal decides: float32 and float64 then land on different sides and differ by the whole
      value, for a handful of unpredictable rays."""
    suns = RC.sun_directions()
    lobe = RC.lobe_directions()
    lobe_sun = torch.tensor([RC.unit(*RC.LOBE_SUN)])
    assert _f32_against_f64("hapke_bc", False, suns, None) > 1.0
    assert _f32_against_f64("rpv111", False, suns, None) < 0.5
    for name in ("hapke_bc", "hapke_bct", "hapke_shell3", "microfacet"):
        assert _f32_against_f64(name, True, suns, None) < 0.5, name
        assert _f32_against_f64(name, True, lobe_sun.expand(lobe.shape[0], 3), lobe) < 0.5, name
    from oracle import brdf as OB
    at_pi = OB._f(torch.tensor([math.pi], dtype=torch.float64))
    below = OB._f(torch.tensor([math.pi - 1e-4], dtype=torch.float64))
    assert bool(torch.isinf(at_pi).all()) and float(below) == 0.0
