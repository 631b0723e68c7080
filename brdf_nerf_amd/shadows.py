"""Relighting WITH cast shadows: a view of a --sun_v analystic model under K sun directions from ONE geometry pass.

In such a model the irradiance of a sample is the transparency of the field along the sun direction, taken from the ray's
pass-1 surface point (rendering.py:244-259, models/spsbrdfnerf.py:259-273, 354): a moved sun moves the shadows.  The reference
runs that model with gsam_only=True only, and relights by rendering again per direction.  Per ray only the sun
pass depends on the sun: G sigma-only points along the sun ray, a transmittance scan over them, and the shading.  So:

  render_shadow_surface    the geometry of render_rays(gsam_only=True): pass 1 (sigma only), the guided samples, pass 2 on them
                           and its compositing - kept with the pass-1 depth and the sun pass's own draws
  relight_shadowed         K directions from a ShadowSurface: per direction tile and chunk bn_sun_ray_table, ONE bn_field_sigma
                           over the tile's kt R G points, bn_sun_shade_dirs (transmittance + shading fused)
  sun_visibility           the shadow map alone: T_{G-1} of every (direction, ray)
  relight_image_shadowed   the two in one call, streamed chunk by chunk

K suns cost one geometry pass + K R G sigma-only points instead of K (R S + R G sigma-only + R G full) points.
relight.relight_image serves every model WITHOUT the sun pass and keeps refusing this one by name.
"""
import torch

from . import functions as Fn
from .relight import _TILE_BYTES, _dirs       # (the package binds the name `relight` to the function: import by module path)
from .rendering import _field_spec, _sample_passes, shade_desc
from .viewwalk import ViewWalk, check_out


def _check_shadowed(model, args, apply_brdf):
    """The argument checks, before any device work."""
    if not (getattr(args, "sun_v", "none") == "analystic" or getattr(model, "sun_v", "none") == "analystic"):
        raise ValueError("relighting with cast shadows needs a model trained with --sun_v analystic (this one has sun_v="
                         f"{getattr(model, 'sun_v', 'none')!r}): without the sun-visibility pass use relight_image")
    if not apply_brdf:
        raise ValueError("apply_brdf=False: the reference runs no sun-visibility pass then (rendering.py:244), so nothing casts a "
                         "shadow - use relight_image's path on a model without --sun_v analystic")


class ShadowSurface:
    """What K shadowed shadings of R rays read: the composited sums acc (R, C), wsum (R,), depth (R,) of the guided samples, the
    rays (R, W) themselves, the pass-1 depth d1 (R,) the sun rays start from, and the sun pass's own draws u_sun, noise_sun (R, G)
    - one draw shared by every direction, as K reseeded render_rays calls would draw it.  rows (R, G, C) and weights (R, G) are
    kept only when the shading is per sample (a Lambertian kind or --MultiBRDF 1).  bounds: the (i, j) ray ranges that were
    rendered by one call each - the far bound of a sun ray is scaled with the directions of ROW 0 of its call (rendering.sun_far,
    the reference's quirk), so the ranges are shaded one by one."""

    def __init__(self, acc, wsum, depth, rays, d1, u_sun, noise_sun, model, args, spec, packed, apply_theta, rows=None, weights=None,
                 bounds=None):
        self.acc, self.wsum, self.depth, self.rays, self.d1, self.u_sun, self.noise_sun = acc, wsum, depth, rays, d1, u_sun, noise_sun
        self.model, self.args, self.spec, self.packed, self.apply_theta = model, args, spec, packed, apply_theta
        assert (rows is None) == (weights is None)
        self.rows, self.weights = rows, weights
        self.bounds = [(0, acc.shape[0])] if bounds is None else list(bounds)

    @property
    def per_sample(self):
        return self.rows is not None

    @property
    def n_rays(self):
        return self.acc.shape[0]

    @property
    def rays_d(self):
        return self.rays[:, 3:6]

    @staticmethod
    def row_table(spec, args, per_sample, W):
        """(attribute, trailing shape) of the per-ray tensors that ViewWalk.join_attrs joins; W: the columns of the ray table."""
        C, G = spec.out_channels, args.guided_samples
        return ([("acc", (C,)), ("wsum", ()), ("depth", ()), ("rays", (W,)), ("d1", ()), ("u_sun", (G,))]
                + ([("noise_sun", (G,))] if args.noise_std != 0 else []) + ([("rows", (G, C)), ("weights", (G,))] if per_sample else []))

    def desc(self, cos_irra_on=False):
        """bn_shade_desc of this surface (the selection rules of rendering.shade(), apply_brdf=True)."""
        return shade_desc(self.model, self.args, self.spec, True, cos_irra_on)


def _per_sample(model, args, spec):
    """Per-sample irradiance reaches the colour sample by sample for a Lambertian kind (models/spsbrdfnerf.py:265-273) and for one
    BRDF per sample (:350-352); one BRDF per ray reads the last sample's alone (:354)."""
    from . import _lib as L
    return shade_desc(model, args, spec, True, False).kind == L.BN_SHADE_LAMBERT or bool(model.MultiBRDF)


def _shadow_chunks(walk, models, args, rays, ts, apply_theta, bTestNormal):
    """The geometry of this rank's share of the rays, chunk by chunk: yields (i, j, ShadowSurface of rays[i:j])."""
    noise_on = args.noise_std != 0
    for i, j in walk.chunks():
        # rand (R, S), randn (R, S), the sun pass's rand (R, G) and randn (R, G), rand (R, G): render_rays' order
        p = _sample_passes(models, args, rays[i:j], None if ts is None else ts[i:j], "test", None, None, None, True, bTestNormal,
                           False, True, apply_theta, defer_sun=True)
        R, G = p.z2.shape
        C = p.spec.out_channels
        noise2 = torch.randn(R, G, device=p.rays.device)        # inference() draws it before the field pass
        out = p.model.evaluate(p.spec, p.packed, rays=p.rays, z=p.z2, t_embed=p.rays_t).view(R, G, C)
        _, _, weights, depth, acc = Fn.composite(p.z2.contiguous(), out, noise2 if noise_on else None, args.noise_std)
        keep = _per_sample(p.model, args, p.spec)
        u_sun, noise_sun = p.sun_draws
        yield i, j, ShadowSurface(acc, weights.sum(-1), depth, p.rays, p.d1.contiguous(), u_sun, noise_sun if noise_on else None,
                                  p.model, args, p.spec, p.packed, bool(apply_theta), out.contiguous() if keep else None,
                                  weights.contiguous() if keep else None)


@torch.no_grad()
def render_shadow_surface(models, args, rays, ts=None, chunk=None, apply_brdf=True, apply_theta=False, group=None, bTestNormal=False):
    """The geometry of render_rays(gsam_only=True) for a --sun_v analystic model, per chunk: pass 1 (sigma only), the guided
    samples, pass 2 on the G guided samples and its compositing - WITHOUT the sun pass and the shading.  Every random draw is taken
    in render_rays' order (the sun pass's two included), so after the same torch.manual_seed `depth` is its depth_coarse bit for
    bit.  Under data parallelism every rank renders its contiguous share and the rows are all-gathered.  -> ShadowSurface."""
    model = models["coarse"]
    _check_shadowed(model, args, apply_brdf)
    walk = ViewWalk(rays.shape[0], chunk or args.chunk, group)
    parts = [c for _, _, c in _shadow_chunks(walk, models, args, rays, ts, apply_theta, bTestNormal)]
    spec = parts[0].spec if parts else _field_spec(model, True, apply_theta, bTestNormal)
    packed = parts[0].packed if parts else model.repack(spec)
    res = walk.join_attrs(parts, ShadowSurface.row_table(spec, args, _per_sample(model, args, spec), rays.shape[1]), rays.device)
    return ShadowSurface(res["acc"], res["wsum"], res["depth"], res["rays"], res["d1"], res["u_sun"], res.get("noise_sun"), model, args,
                         spec, packed, bool(apply_theta), res.get("rows"), res.get("weights"), walk.all_chunks())


def _sun_pass(surface, sun, desc, rgb, vis, dir_tile):
    """bn_sun_ray_table, bn_field_sigma and bn_sun_shade_dirs per direction tile and per rendered range of the surface; rgb
    (K, R, 3) / vis (K, R) or None are device tensors written through their plane strides."""
    from . import _lib as L
    model, args = surface.model, surface.args
    K, G = sun.shape[0], surface.u_sun.shape[1]
    sigma_spec = model.spec(False, False, False, False)       # the sigma-only pass of rendering.inference(): no head, no normal
    named = model.named()
    samples = desc.kind == L.BN_SHADE_LAMBERT or bool(model.MultiBRDF)
    if samples and not surface.per_sample:
        raise ValueError("this surface holds no per-sample rows, which a Lambertian kind or --MultiBRDF 1 is shaded from")
    longest = max([j - i for i, j in surface.bounds] + [1])
    if dir_tile is None:
        dir_tile = max(1, _TILE_BYTES // (8 * longest * G))   # sigma_sun + z_sun of a tile: 8 bytes per point
    dir_tile = max(1, min(int(dir_tile), K))
    for i, j in surface.bounds:
        if j <= i:
            continue
        rays, d1, u = surface.rays[i:j], surface.d1[i:j], surface.u_sun[i:j]
        noise = None if surface.noise_sun is None else surface.noise_sun[i:j]
        src = dict(X=surface.rows[i:j], w=surface.weights[i:j]) if samples else dict(acc=surface.acc[i:j], wsum=surface.wsum[i:j])
        for k0 in range(0, K, dir_tile):
            k1 = min(K, k0 + dir_tile)
            table, z_sun = Fn.sun_ray_table(rays, d1, sun[k0:k1], u)
            sigma = Fn.field_sigma(sigma_spec, named, surface.packed, rays=table, z=z_sun)
            Fn.sun_shade_dirs(desc, sigma, z_sun, rays[:, 3:6], sun[k0:k1], noise=noise, noise_std=args.noise_std,
                              rgb=None if rgb is None else rgb[k0:k1, i:j], vis=None if vis is None else vis[k0:k1, i:j], **src)


@torch.no_grad()
def sun_visibility(surface, sun_dirs, dir_tile=None):
    """The shadow map alone: -> (K, R), the sun visibility T_{G-1} of every ray's surface point under every direction - what
    render_rays returns as sun_coarse[:, -1, 0] with rays[:, 8:11] = sun_dirs[k] (same draws)."""
    sun = _dirs(sun_dirs, surface.acc.device)
    vis = torch.empty((sun.shape[0], surface.n_rays), dtype=torch.float32, device=surface.acc.device)
    if surface.n_rays:
        _sun_pass(surface, sun, surface.desc(False), None, vis, dir_tile)
    return vis


@torch.no_grad()
def relight_shadowed(surface, sun_dirs, cos_irra_on=False, out=None, dir_tile=None, want_visibility=False):
    """Shade a ShadowSurface under K sun directions: -> rgb (K, R, 3), rgb[k] = what render_rays(gsam_only=True) gives as
    rgb_coarse with rays[:, 8:11] = sun_dirs[k] (same draws); with want_visibility -> (rgb, visibility (K, R)).
      cos_irra_on  with a normal field the reference drops the visibility (shade(): the cosine branch wins): no sun point is
                   evaluated then, bn_ray_shade_dirs / bn_sample_shade_dirs shade the sums / rows (want_visibility still runs
                   the sun pass, for the map)
      out          (K, R, 3) float32 to write into, on the device (rows contiguous, e.g. a [:, i:j] slice) or on the host
      dir_tile     directions per field pass (None: sigma_sun + z_sun of a tile stay under relight._TILE_BYTES); every
                   (direction, ray) is computed on its own and bn_field_sigma is batch invariant: the split changes no bit."""
    from . import _lib as L
    dev = surface.acc.device
    sun = _dirs(sun_dirs, dev)
    K, R = sun.shape[0], surface.n_rays
    check_out(out, (K, R, 3))
    desc = surface.desc(cos_irra_on)
    direct = out is None or (out.is_cuda and Fn.plane_rows(out))
    rgb = out if (direct and out is not None) else torch.empty((K, R, 3), dtype=torch.float32, device=dev)
    vis = torch.empty((K, R), dtype=torch.float32, device=dev) if want_visibility else None
    if R > 0:
        if cos_irra_on and desc.ch_normal >= 0:
            samples = surface.per_sample and desc.kind != L.BN_SHADE_LAMBERT
            for k0 in range(0, K, max(1, min(int(dir_tile or K), K))):
                k1 = min(K, k0 + max(1, min(int(dir_tile or K), K)))
                if samples:
                    Fn.sample_shade_dirs(desc, surface.rows, surface.weights, surface.rays_d, sun[k0:k1], rgb=rgb[k0:k1])
                else:
                    rgb[k0:k1].copy_(Fn.ray_shade_dirs(desc, surface.acc, surface.wsum, surface.rays_d, sun[k0:k1])[0])
            if vis is not None:
                _sun_pass(surface, sun, surface.desc(False), None, vis, dir_tile)
        else:
            _sun_pass(surface, sun, desc, rgb, vis, dir_tile)
    if out is None:
        out = rgb
    elif not direct:
        out.copy_(rgb)
    return (out, vis) if want_visibility else out


@torch.no_grad()
def relight_image_shadowed(models, args, rays, sun_dirs, ts=None, chunk=None, apply_brdf=True, apply_theta=False, cos_irra_on=False,
                           group=None, out=None, bTestNormal=False, dir_tile=None, want_visibility=None):
    """render_shadow_surface + relight_shadowed, streamed: each chunk's geometry is rendered once, shaded under all K directions
    straight into rgb[:, i:j] and dropped.  -> dict rgb (K, R, 3), depth (R,), visibility (K, R).  Replaces K calls of
    render_image(gsam_only=True) with the sun replaced; the far bound's row-0 quirk is per chunk, exactly as there.  With
    cos_irra_on and a normal field the sun pass is unused upstream and is not run: visibility is None unless
    want_visibility=True asks for the map (want_visibility=False: never computed).  Under data parallelism each rank takes its
    contiguous share and the results are all-gathered."""
    model = models["coarse"]
    _check_shadowed(model, args, apply_brdf)
    dev = rays.device
    sun = _dirs(sun_dirs, dev)
    K = sun.shape[0]
    walk = ViewWalk(rays.shape[0], chunk or args.chunk, group)
    rgb, vis, depth = walk.planes(K, (3,), out, dev), None, []
    for i, j, part in _shadow_chunks(walk, models, args, rays, ts, apply_theta, bTestNormal):
        if want_visibility is None:
            want_visibility = not (cos_irra_on and part.desc(False).ch_normal >= 0)
        if want_visibility and vis is None:
            vis = walk.planes(K, (), None, dev)
        got = relight_shadowed(part, sun, cos_irra_on=cos_irra_on, out=rgb.chunk(i, j), dir_tile=dir_tile,
                               want_visibility=bool(want_visibility))
        if want_visibility:
            vis.chunk(i, j).copy_(got[1])
        depth.append(part.depth)
    if want_visibility is None and walk.world > 1:           # a rank without rays: as the ranks with rays decide
        nr = model.normal in ("analystic_learned", "analystic", "learned") or bTestNormal
        want_visibility = not (cos_irra_on and nr)
    if want_visibility and vis is None:                      # a rank without rays takes part in the gather with zero rays
        vis = walk.planes(K, (), None, dev)
    rgb, vis = rgb.result(), None if vis is None else vis.result()
    return {"rgb": rgb, "depth": walk.join(depth, (), device=dev), "visibility": vis}


__all__ = ["ShadowSurface", "render_shadow_surface", "sun_visibility", "relight_shadowed", "relight_image_shadowed"]
