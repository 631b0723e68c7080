"""Relighting a rendered view and the BRDF lobe of a pixel from ONE geometry pass.

The reference relights by writing a sun direction into the ray table and rendering again, once per direction
(create_dsm.py:44-77: rays[:, 8:11] = sun; eval.py's eval_pixel_variedvw / get_view_dirs for the view hemisphere): every call
evaluates the field again, which is all of the cost.  With one BRDF per ray (MultiBRDF == 0) and no sun-visibility pass the
colour is a function of the composited sums, the view direction and the sun direction (rendering.shade_ray), and the sums do
not depend on the sun.  So:

  render_surface   the geometry half of evaluate.render_image: acc, wsum, depth of every ray of the view, kept
  relight          K sun directions (or K (view, sun) pairs) shaded from a surface in one launch (bn_ray_shade_dirs)
  relight_image    the two in one call
  brdf_lobe        BRDF value and colour of chosen pixels over a grid of view directions
  directions       the reference's (elevation, azimuth) -> unit vector convention (eval.py:300-314, create_dsm.py:48-50)

With one BRDF per SAMPLE (--MultiBRDF 1) the same holds one level down: rgb = clamp(sum_s w_s (brdf(row_s, sun, view) (1 + 2 pad)
- pad) irr), and neither the depth-sorted rows nor their weights depend on the sun.  per_sample=True keeps (or, in relight_image,
streams) the rows and weights and shades them with bn_sample_shade_dirs: one geometry pass + R S K pointwise BRDF evaluations.  It
is an explicit opt-in because a per-sample surface is S C times larger than the composited one.

Not covered, and refused by name: --MultiBRDF without per_sample=True (shading is per sample), --sun_v analystic (the irradiance
itself depends on the sun through a field pass: shadows.py serves that model), gsam_only.
"""
import torch

from . import functions as Fn
from .rendering import _field_spec, _merged_geometry, shade_desc
from .viewwalk import ViewWalk, check_out

# directions of one bn_ray_shade_dirs launch at most: bounds the (K, R, 3) result a launch writes when `out` lives on the host
_TILE_BYTES = 1 << 30


def directions(elevation_deg, azimuth_deg):
    """Unit vectors of (elevation, azimuth) in degrees, the reference's convention (eval.py:300-314, create_dsm.py:48-50):
    (sin az cos el, cos az cos el, sin el) - azimuth from the +y axis towards +x, elevation above the x-y plane.  The two
    arguments broadcast; -> float32 (..., 3)."""
    el = torch.deg2rad(torch.as_tensor(elevation_deg, dtype=torch.float64))
    az = torch.deg2rad(torch.as_tensor(azimuth_deg, dtype=torch.float64))
    el, az = torch.broadcast_tensors(el, az)
    return torch.stack([torch.sin(az) * torch.cos(el), torch.cos(az) * torch.cos(el), torch.sin(el)], -1).float()


def _check_relightable(model, args, gsam_only=False, per_sample=False):
    """The argument checks of the shortcut, before any device work."""
    multi = bool(int(getattr(args, "MultiBRDF", 0)) or getattr(model, "MultiBRDF", False))
    if multi and not per_sample:
        raise NotImplementedError("relighting from composited sums does not cover --MultiBRDF 1: every sample is shaded by its own "
                                  "BRDF, so each direction needs the per-sample outputs (render_rays per direction), or "
                                  "per_sample=True, which keeps them")
    if getattr(args, "sun_v", "none") == "analystic" or getattr(model, "sun_v", "none") == "analystic":
        raise NotImplementedError("relighting from composited sums does not cover --sun_v analystic: the irradiance is the sun "
                                  "visibility of a field pass along each sun direction (shadows.relight_image_shadowed runs that "
                                  "pass per direction on one geometry pass)")
    if gsam_only:
        raise NotImplementedError("relighting does not cover gsam_only=True: the surface is composited from the merged S + G "
                                  "sample set of the default evaluation path")
    if per_sample and not multi:
        raise ValueError("per_sample=True needs a --MultiBRDF 1 model: with one BRDF per ray render_rays shades the composited "
                         "sums, which a sum of per-sample BRDF values does not reproduce (leave per_sample off)")


class Surface:
    """What the ray-level shading reads, for all R rays of a view: the composited sums acc (R, C) and wsum (R,), depth (R,),
    the ray directions rays_d (R, 3), and the model / args / spec that name the BRDF (rendering.shade_desc).  16 MB for a
    512 x 512 view at C = 16.
    A per-sample surface (render_surface(per_sample=True), --MultiBRDF 1) also holds the depth-sorted field-output rows
    (R, S + G, C) and their compositing weights (R, S + G): S C times the size - about 2.3 GB for a 512 x 512 view at
    S + G = 128 and C = 16 (262,144 x 128 x (16 + 1) x 4 bytes)."""

    def __init__(self, acc, wsum, depth, rays_d, model, args, spec, apply_brdf, apply_theta, rows=None, weights=None):
        self.acc, self.wsum, self.depth, self.rays_d = acc, wsum, depth, rays_d
        self.model, self.args, self.spec, self.apply_brdf, self.apply_theta = model, args, spec, apply_brdf, apply_theta
        assert (rows is None) == (weights is None)
        self.rows, self.weights = rows, weights

    @property
    def per_sample(self):
        return self.rows is not None

    @property
    def n_rays(self):
        return self.acc.shape[0]

    @staticmethod
    def row_table(spec, args, per_sample):
        """(attribute, trailing shape) of the per-ray tensors that ViewWalk.join_attrs joins."""
        C, SG = spec.out_channels, args.n_samples + args.guided_samples
        return [("acc", (C,)), ("wsum", ()), ("depth", ())] + ([("rows", (SG, C)), ("weights", (SG,))] if per_sample else [])

    def select(self, rows):
        """The surface of the chosen rays (rows: indices, a slice or a mask)."""
        if not isinstance(rows, slice):
            rows = torch.as_tensor(rows, device=self.acc.device)
        pick = lambda t: t[rows].contiguous()
        return Surface(pick(self.acc), pick(self.wsum), pick(self.depth), pick(self.rays_d), self.model, self.args, self.spec,
                       self.apply_brdf, self.apply_theta, None if self.rows is None else pick(self.rows),
                       None if self.weights is None else pick(self.weights))

    def desc(self, apply_brdf=None, cos_irra_on=False):
        """bn_shade_desc of this surface (the selection rules of rendering.shade())."""
        apply_brdf = self.apply_brdf if apply_brdf is None else apply_brdf
        if apply_brdf and not self.apply_brdf:
            raise ValueError("this surface was rendered with apply_brdf=False: the BRDF heads were not composited")
        return shade_desc(self.model, self.args, self.spec, apply_brdf, cos_irra_on)


@torch.no_grad()
def render_surface(models, args, rays, ts=None, chunk=None, apply_brdf=False, apply_theta=False, group=None, gsam_only=False,
                   bTestNormal=False, per_sample=False):
    """The geometry half of evaluate.render_image: pass 1, the guided samples and the compositing of the merged sample set of
    every ray, in chunks, WITHOUT the shading - the random stream is consumed exactly as render_rays consumes it, so after the
    same torch.manual_seed the sums are the ones render_rays composited (and `depth` is its depth_coarse bit for bit).  Under
    data parallelism every rank renders its contiguous share of the rays and the rows are all-gathered, as in render_image.
    per_sample=True (a --MultiBRDF 1 model only): the surface also keeps the depth-sorted field-output rows (R, S + G, C) and
    their weights (R, S + G), which relight / brdf_lobe then shade sample by sample.  That is S C times the composited
    surface - about 2.3 GB for a 512 x 512 view at S + G = 128 and C = 16; relight_image(per_sample=True) streams the rows
    chunk by chunk instead of holding them.
    -> Surface."""
    _check_relightable(models["coarse"], args, gsam_only, per_sample)
    walk = ViewWalk(rays.shape[0], chunk or args.chunk, group)
    parts = [c for _, _, c in _surface_chunks(walk, models, args, rays, ts, apply_brdf, apply_theta, bTestNormal, per_sample)]
    return _join_surfaces(walk, parts, models, args, rays, apply_brdf, apply_theta, bTestNormal, per_sample)


def _surface_chunks(walk, models, args, rays, ts, apply_brdf, apply_theta, bTestNormal, per_sample):
    """The geometry of this rank's share of the rays, chunk by chunk: yields (i, j, Surface of rays[i:j])."""
    for i, j in walk.chunks():
        p, (out, _, _, weights, depth, acc) = _merged_geometry(models, args, rays[i:j], None if ts is None else ts[i:j],
                                                               apply_brdf=apply_brdf, bTestNormal=bTestNormal, apply_theta=apply_theta)
        yield i, j, Surface(acc, weights.sum(-1), depth, rays[i:j, 3:6].float().contiguous(), p.model, args, p.spec, bool(apply_brdf),
                            bool(apply_theta), out.contiguous() if per_sample else None, weights.contiguous() if per_sample else None)


def _join_surfaces(walk, parts, models, args, rays, apply_brdf, apply_theta, bTestNormal, per_sample):
    """One Surface of all rays from this rank's chunk surfaces (all-gathered along the ray axis under data parallelism)."""
    model = models["coarse"]
    # a rank without rays (more ranks than rays): the spec is still the model's
    spec = parts[0].spec if parts else _field_spec(model, apply_brdf, apply_theta, bTestNormal)
    res = walk.join_attrs(parts, Surface.row_table(spec, args, per_sample), rays.device)
    return Surface(res["acc"], res["wsum"], res["depth"], rays[:, 3:6].float().contiguous(), model, args, spec, bool(apply_brdf),
                   bool(apply_theta), res.get("rows"), res.get("weights"))


def _dirs(d, device, K=None):
    d = torch.as_tensor(d, dtype=torch.float32).to(device).reshape(-1, 3)
    if K is not None and d.shape[0] == 1 and K != 1:
        d = d.expand(K, 3)
    return d.contiguous()


@torch.no_grad()
def relight(surface, sun_dirs, apply_brdf=None, cos_irra_on=False, out=None, view_dirs=None, want_brdf=False, dir_tile=None):
    """Shade a Surface under K sun directions: -> rgb (K, R, 3), rgb[k] = what render_rays gives as rgb_coarse with
    rays[:, 8:11] = sun_dirs[k] (same draws).  No field evaluation.  A per-sample surface (--MultiBRDF 1) whose shading is a
    BRDF goes through bn_sample_shade_dirs on its rows and weights; without a BRDF (apply_brdf=False) the reference shades such a
    model per ray too, and the composited sums go through bn_ray_shade_dirs like any other surface.
      sun_dirs   (K, 3)
      view_dirs  None: every ray is seen along its own -rays_d.  (K, 3) (or (1, 3)): lobe mode - direction k REPLACES the view
                 of every ray, paired with sun_dirs[k] (sun_dirs (1, 3): one fixed sun).
      apply_brdf / cos_irra_on  as in render_rays (apply_brdf None: as the surface was rendered)
      out        (K, R, 3) float32 to write into, on the device or on the host
      want_brdf  also return the BRDF value before irradiance and clamp: -> (rgb, brdf); per sample: sum_s w_s brdf_s
      dir_tile   directions per launch (None: all at once on the device, 1 GiB of results at a time into a host `out`);
                 every (direction, ray) is computed on its own, so the split changes no bit."""
    dev = surface.acc.device
    K = None if view_dirs is None else torch.as_tensor(view_dirs).reshape(-1, 3).shape[0]
    sun = _dirs(sun_dirs, dev, K)
    K = sun.shape[0]
    view = None if view_dirs is None else _dirs(view_dirs, dev, K)
    if view is not None and view.shape[0] != K:
        raise ValueError(f"view_dirs ({view.shape[0]}) and sun_dirs ({K}) must pair up (or one of them be a single direction)")
    R = surface.n_rays
    desc = surface.desc(apply_brdf, cos_irra_on)
    check_out(out, (K, R, 3))
    from . import _lib as L
    samples = surface.per_sample and desc.kind != L.BN_SHADE_LAMBERT
    # the per-sample kernel writes through a plane stride: the (K, i:j, 3) slice of a whole view is written in place
    direct = out is None or (out.is_cuda and (Fn.plane_rows(out) if samples else out.is_contiguous()))
    if dir_tile is None:
        dir_tile = K if direct else max(1, _TILE_BYTES // max(1, 12 * R))
    dir_tile = max(1, min(int(dir_tile), K))
    if out is None:
        out = torch.empty((K, R, 3), dtype=torch.float32, device=dev)
    brdf = torch.empty((K, R, 3), dtype=torch.float32, device=dev) if want_brdf else None
    if R > 0:
        for k0 in range(0, K, dir_tile):
            k1 = min(K, k0 + dir_tile)
            tile = dict(view=None if view is None else view[k0:k1], rgb=out[k0:k1] if direct else None,
                        brdf=None if brdf is None else brdf[k0:k1])
            if samples:
                rgb_t, _ = Fn.sample_shade_dirs(desc, surface.rows, surface.weights, surface.rays_d, sun[k0:k1], **tile)
            else:
                rgb_t, _ = Fn.ray_shade_dirs(desc, surface.acc, surface.wsum, surface.rays_d, sun[k0:k1], **tile)
            if not direct:
                out[k0:k1].copy_(rgb_t)
    return (out, brdf) if want_brdf else out


@torch.no_grad()
def relight_image(models, args, rays, sun_dirs, ts=None, chunk=None, apply_brdf=False, apply_theta=False, cos_irra_on=False,
                  group=None, out=None, return_surface=False, per_sample=False, **kw):
    """render_surface + relight: one geometry pass over the rays of a view, then K ray-level shadings.
    -> dict rgb (K, R, 3), depth (R,) (+ surface with return_surface).  Replaces K calls of render_image with the sun replaced.
    per_sample=True (a --MultiBRDF 1 model): the view's rows are never held - each chunk's geometry is rendered, shaded under all
    K directions straight into rgb[:, i:j, :] and dropped (a chunk of 16,384 rays at S + G = 128, C = 16 is 143 MB; the whole
    512 x 512 view would be 2.3 GB).  Only return_surface=True keeps them.  The draws are consumed as render_rays consumes them."""
    if not per_sample:
        surface = render_surface(models, args, rays, ts=ts, chunk=chunk, apply_brdf=apply_brdf, apply_theta=apply_theta, group=group,
                                 **kw)
        res = {"rgb": relight(surface, sun_dirs, apply_brdf=apply_brdf, cos_irra_on=cos_irra_on, out=out), "depth": surface.depth}
        if return_surface:
            res["surface"] = surface
        return res
    gsam_only, bTestNormal = kw.pop("gsam_only", False), kw.pop("bTestNormal", False)
    if kw:
        raise TypeError(f"relight_image: unexpected arguments {sorted(kw)}")
    _check_relightable(models["coarse"], args, gsam_only, True)
    sun = _dirs(sun_dirs, rays.device)
    walk = ViewWalk(rays.shape[0], chunk or args.chunk, group)
    rgb = walk.planes(sun.shape[0], (3,), out, rays.device)        # this rank's rays are shaded straight into it
    kept, depth = [], []
    for i, j, part in _surface_chunks(walk, models, args, rays, ts, apply_brdf, apply_theta, bTestNormal, True):
        relight(part, sun, apply_brdf=apply_brdf, cos_irra_on=cos_irra_on, out=rgb.chunk(i, j))
        depth.append(part.depth)
        if return_surface:
            kept.append(part)
    res = {"rgb": rgb.result(), "depth": walk.join(depth, (), device=rays.device)}
    if return_surface:
        res["surface"] = _join_surfaces(walk, kept, models, args, rays, apply_brdf, apply_theta, bTestNormal, True)
    return res


@torch.no_grad()
def brdf_lobe(surface, rows, view_dirs, sun_dirs, apply_brdf=None, cos_irra_on=False):
    """The BRDF of the chosen pixels over a grid of view directions (eval.py's eval_pixel_variedvw): -> (brdf, rgb), each
    (len(rows), V, 3); brdf is the value before irradiance and clamp, which is what a lobe plot shows.  sun_dirs: one fixed sun
    (3,) / (1, 3), or (V, 3) paired with view_dirs.  No field evaluation: the pixel's composited normal, albedo and BRDF
    parameters stay as rendered (a per-sample surface: its samples' own, brdf = sum_s w_s brdf_s).  With --input_viewdir the field's own view input stays the camera's (the albedo head was
    evaluated for the rendered ray); only the BRDF's view direction varies."""
    sub = surface.select(rows)
    rgb, brdf = relight(sub, sun_dirs, apply_brdf=apply_brdf, cos_irra_on=cos_irra_on, view_dirs=view_dirs, want_brdf=True)
    return brdf.permute(1, 0, 2).contiguous(), rgb.permute(1, 0, 2).contiguous()


__all__ = ["Surface", "render_surface", "relight", "relight_image", "brdf_lobe", "directions"]
