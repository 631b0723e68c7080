"""The validation maps of a rendered view on the device, streamed chunk by chunk.

After every validation render the reference builds a stack of per-view maps from the per-sample dict of the WHOLE view
(eval.py:403-456, main.py:451-555): it takes the sample nearest the composited depth with a host np.argmin, picks that sample's
values with a Python double loop over all rays (train_utils.get_surface_feature, run four times), sums weights x feature for
the accumulated maps, and logs val/depth_std, val/bad_nr_an% and val/nr_an0%.  Here every chunk is reduced while it is on the
device and only ray-level results are kept:

  ray_maps       bn_ray_maps: np.argmin(|z - depth|), the surface sample's values as bits, calc_depth_std(_2), sum_s w X and the
                 integer counts of NormalRegLoss's perc_ng_nr and check_vec0
  point_normals  bn_point_normals: sat_utils.calc_normal_from_pts3d (:16-50) on an (H, W, 3) image of points
  depth_normals  calc_normal_from_depth_v2 (datasets/satellite_rgb_dep.py:578-584): point_cloud + point_normals
  view_maps      render_image's walk (viewwalk.py) with the reductions in it: the maps, the logged scalars and (cross_rows=) the per-sample
                 values of one image row, the dump of main.py:567-595

precision: 'reference' rounds the UTM points to float32 before differencing them, as upstream's `.type(torch.FloatTensor)`
does (a float32 ulp is 0.25 m at a northing of 3.3e6 m: on points 0.4 m apart that alone turns normals by tens of degrees);
'exact' differences the float64 points.  Both then run the same float64 chain.

The maps are float32 in physical units, before any colour encoding.  Not covered: ToImage's 8-bit normalisation and colour
maps (cv2 / PIL), TensorBoard, GeoTIFF I/O, the `sun` map, visu_scale != 1.
"""
import torch

from . import functions as Fn
from .functions import RAY_MAP_COUNTERS, fixed_mean

_PRECISIONS = {"reference": True, "exact": False}
STD_FIX = 2.0 ** 20
# field heads -> the keys of the reference's result dict (models/spsbrdfnerf.py) and of its maps
_HEAD_KEYS = {"k_from_xyz": "rpv_k", "theta_rpv_from_xyz": "rpv_theta", "rhoc_from_xyz": "rpv_rhoc", "b_from_xyz": "hpk_b",
              "c_from_xyz": "hpk_c", "theta_from_xyz": "hpk_theta", "roughness_from_xyz": "roughness"}
# BRDF auxiliaries of shade(): (R, 1, D) with one BRDF per ray, (R, S, D) with --MultiBRDF 1
_AUX_KEYS = ("brdf", "glossy", "f", "g", "d", "l_dot_n", "v_dot_n", "halfvec", "n_h", "hpk_P", "hpk_Hi", "hpk_Hv", "hpk_ci", "hpk_cv",
             "hpk_ShadFunc")
_RAY_KEYS = ("nr_vw", "nr_sun")
CROSS_KEYS = ("z_vals", "sigmas", "alphas", "transparency", "sort_idx", "depth", "std")


def _precision(precision):
    if precision not in _PRECISIONS:
        raise ValueError(f"precision {precision!r} ('reference' or 'exact')")
    return _PRECISIONS[precision]


@torch.no_grad()
def ray_maps(z_vals, weights, depth, X=None, accumulate=False, normal_col=None, view=None):
    """bn_ray_maps on one chunk of rays.  z_vals, weights (R, S), depth (R,): float32 on the device, contiguous; X (R, S, E)
    float32 or None, any strides (a column slice is read in place); normal_col with view (R, 3) = -rays_d: count the samples
    whose normal X[..., normal_col:normal_col + 3] faces away from the camera or is not of unit length.
    -> surf_idx (R,) int32 - np.argmin(|z - depth|, axis=1), the first NaN else the first minimum; surf (R, E) - the bits of
    X[r, surf_idx[r]] (None without X); var, std (R,) - sum_s (z - depth)^2 w in float64 in ascending s, and its root;
    accum (R, E) - sum_s w X in float64 in ascending s (None unless accumulate); counters (6,) int64 on the device, in the
    order of RAY_MAP_COUNTERS.  ValueError on host tensors, other dtypes, S outside [1, 4096], more than 64 channels, a normal
    column outside [0, E - 3]."""
    return Fn.ray_maps(z_vals, weights, depth, X, accumulate, normal_col, view)


@torch.no_grad()
def point_normals(points, valid=None, precision="reference"):
    """sat_utils.calc_normal_from_pts3d: points (H, W, 3) float64 on the device -> normals (H, W, 3) float32, zero on the
    border, NaN where a NaN is read; with valid (H, W) float32 also valid_normal (H, W) by the rule of :19-24, else None.
    The cross product is over the coordinate axis always (upstream's torch.cross without dim goes wrong when H - 2 or W - 2
    is 3; not reproduced).  -> (normals, valid_normal)."""
    return Fn.point_normals(points, valid, _precision(precision))


@torch.no_grad()
def depth_normals(rays, depth, frame, H, W, precision="reference"):
    """calc_normal_from_depth_v2: the normals of the surface points of a view, (H W, 3) float32.  rays (H W, >= 6), depth (H W,)."""
    from .dsm import point_cloud
    round_f32 = _precision(precision)
    if rays.shape[0] != H * W or depth.numel() != H * W:
        raise ValueError(f"depth_normals: {rays.shape[0]} rays and {depth.numel()} depths for a view of {H} x {W}")
    pts = point_cloud(rays, depth, frame)
    return Fn.point_normals(pts.reshape(H, W, 3), None, round_f32)[0].reshape(H * W, 3)


def _check(model, args, rays, H, W, precision, cross_rows):
    if getattr(args, "sun_v", "none") == "analystic" or getattr(model, "sun_v", "none") == "analystic":
        raise NotImplementedError("view_maps does not cover --sun_v analystic: it needs gsam_only=True and the `sun` map of the "
                                  "sun-visibility pass, which are not served here")
    if abs(float(getattr(args, "visu_scale", 1.0)) - 1.0) > 1e-5:
        raise NotImplementedError("view_maps does not cover visu_scale != 1: upstream clamps albedo x visu_scale per SAMPLE before "
                                  "the sum, which the composited sums do not reproduce")
    if rays.shape[0] != H * W:
        raise ValueError(f"view_maps: {rays.shape[0]} rays for a view of {H} x {W}")
    if cross_rows is not None and not (isinstance(cross_rows, int) and 0 <= cross_rows < H):
        raise ValueError(f"view_maps: cross_rows {cross_rows!r} is not an image row in [0, {H})")
    return _precision(precision)


def _blocks(tensors):
    """Per-sample (R, S, d) float32 views -> [(X, {key: (column, d)})]: views of one storage with the same ray and sample strides
    and unit channel stride that fit in 64 columns are read as ONE strided X (the BRDF auxiliaries are columns of one buffer)."""
    groups = {}
    for key, t in tensors.items():
        sc = t.stride(2) if t.shape[2] > 1 else 1
        groups.setdefault((t.untyped_storage().data_ptr(), t.stride(0), t.stride(1), sc), []).append((key, t))
    out = []
    for (_, sr, ss, sc), members in groups.items():
        lo = min(t.storage_offset() for _, t in members)
        hi = max(t.storage_offset() + t.shape[2] for _, t in members)
        if sc == 1 and len(members) > 1 and hi - lo <= min(ss, 64):
            R, S = members[0][1].shape[:2]
            X = members[0][1].as_strided((R, S, hi - lo), (sr, ss, 1), lo)
            out.append((X, {k: (t.storage_offset() - lo, t.shape[2]) for k, t in members}))
        else:
            out.extend((t, {k: (0, t.shape[2])}) for k, t in members)
    return out


@torch.no_grad()
def view_maps(models, args, rays, H, W, frame=None, chunk=None, apply_brdf=False, apply_theta=False, cos_irra_on=False, group=None,
              cross_rows=None, precision="reference", gsam_only=False):
    """The validation maps of one view (eval.py:403-456, main.py:451-595).  It renders as evaluate.render_image does - the same
    shard bounds, chunks and draws, so after the same torch.manual_seed `rgb` and `depth` are bitwise render_image's - and
    reduces every chunk's per-sample tensors with bn_ray_maps before dropping them.
    -> {"maps", "stats", "counters", "brdf_type"} (+ "cross" with cross_rows=).

    maps: float32 on the device, rgb (H W, 3), depth, depth_std (H W,), surf_idx (H W,) int32, every other one (H W, D):
      sigma_s, alpha_s, transparency_s, weight_s   the sample nearest the composited depth (idx= upstream), bit copies
      albedo, normal_an, normal_lr, rpv_k / rpv_theta / rpv_rhoc, hpk_b / hpk_c / hpk_theta, roughness (those the model has)
                         sum_s w x: the columns of the `acc` the compositing kernel returned, bitwise what the shading read
      nr_vw, nr_sun, and with one BRDF per ray brdf, glossy, f, ... : the (R, 1, D) entries of shade() as they are.  Upstream asks
                         for Accum=True on them and does not accumulate a (R, 1, D) tensor (quirk, kept); where it asks for
                         Accum=False on a per-sample tensor it takes the LAST sample (quirk: only `sun`, which is not covered)
      with --MultiBRDF 1 the per-sample auxiliaries K (brdf, glossy, f, ...): K = sum_s w K_s (bn_ray_maps' accum) and K_s, the
                         surface sample; also <map>_s for the field heads above (roughness_s, ...)
      with a frame       altitude (H W,) and nr_from_depth (H W, 3), calc_normal_from_depth_v2 of the gathered depth
    stats: depth_std (val/depth_std, the mean of the map from the integer sum), bad_nr_an%, bad_nr_lr%, nr_an0% (None without
      that normal), depth_std_skipped.  counters: {"an": (6,), "lr": (6,)} int64 on the host (functions.RAY_MAP_COUNTERS).
    cross_rows=h: cross = the per-sample z_vals, sigmas, alphas, transparency, sort_idx (W, S + G) and depth, std (W,) of image
      row h only, sliced out of the chunks that hold it; writing the text file is the caller's business.
    Under a `group` every rank reduces its share, the rows are gathered and the counters merge by one SUM all-reduce.
    Refused: gsam_only=True and --sun_v analystic (NotImplementedError), visu_scale != 1, H W != rays.shape[0]."""
    from .distributed import allreduce_
    from .dsm import altitude_image
    from .rendering import _merged_geometry, shade
    from .viewwalk import ViewWalk
    model = models["coarse"]
    if gsam_only:
        raise NotImplementedError("view_maps does not cover gsam_only=True: the maps are reduced from the merged S + G sample set of "
                                  "the default evaluation path")
    round_f32 = _check(model, args, rays, H, W, precision, cross_rows)
    walk = ViewWalk(rays.shape[0], chunk or args.chunk, group)
    dev = rays.device
    counters = torch.zeros((2, len(RAY_MAP_COUNTERS)), dtype=torch.int64, device=dev)       # rows: normal_an | normal_lr
    parts, cross, brdf_type, main_row = {}, {k: [] for k in CROSS_KEYS}, "Lambertian", 0
    c_lo, c_hi = (cross_rows * W, (cross_rows + 1) * W) if cross_rows is not None else (0, 0)

    def keep(key, t):
        parts.setdefault(key, []).append(t)

    for i, j in walk.chunks():
        p, (out, alphas, transparency, weights, depth, acc) = _merged_geometry(models, args, rays[i:j], apply_brdf=apply_brdf,
                                                                               apply_theta=apply_theta)
        res, brdf_type = shade(model, args, p.spec, out, p.z_all, alphas, transparency, weights, depth, acc, p.rays_d, p.sun_d,
                               apply_brdf, cos_irra_on, p.idx, None)
        spec, R = p.spec, j - i
        view = -p.rays_d
        an = spec.ch_normal_an if spec.normal_an else None
        lr = spec.ch_normal_lr if spec.normal_lr else None
        main_row = 1 if (an is None and lr is not None) else 0
        z_all, weights, depth = p.z_all.contiguous(), weights.contiguous(), depth.contiguous()
        # one launch over the field rows: surface index and sample, std, and the counts of the first normal column
        idx, surf, _, std, _, _ = Fn.ray_maps(z_all, weights, depth, out, False, an if an is not None else lr, view, counters[main_row])
        if an is not None and lr is not None:
            Fn.ray_maps(z_all, weights, depth, out[..., lr:lr + 3], False, 0, view, counters[1], want_surf=False)
        keep("rgb", res["rgb"])
        keep("depth", depth)
        keep("depth_std", std)
        keep("surf_idx", idx)
        at = idx.long().unsqueeze(-1)
        keep("sigma_s", surf[:, 3:4])
        for key, t in (("alpha_s", alphas), ("transparency_s", transparency), ("weight_s", weights)):
            keep(key, t.gather(1, at))                       # a copy of R values, no arithmetic
        keep("albedo", acc[:, 0:3])
        if an is not None:
            keep("normal_an", acc[:, an:an + 3])
        if lr is not None:
            keep("normal_lr", acc[:, lr:lr + 3])
        multi = bool(model.MultiBRDF)
        for (name, _, _), (c0, wdt) in zip(spec.heads[1:], spec.head_cols[1:]):
            key = _HEAD_KEYS.get(name)
            if key is not None and key in res:
                keep(key, acc[:, c0:c0 + wdt])
                if multi:
                    keep(key + "_s", surf[:, c0:c0 + wdt])
        for key in _RAY_KEYS + _AUX_KEYS:
            if key in res and res[key].dim() == 3 and res[key].shape[1] == 1:
                keep(key, res[key][:, 0, :])
        aux = {k: res[k] for k in _AUX_KEYS if k in res and res[k].dim() == 3 and res[k].shape[1] == z_all.shape[1] and multi}
        scratch = torch.zeros((len(RAY_MAP_COUNTERS),), dtype=torch.int64, device=dev)
        for X, cols in _blocks(aux):
            _, s_x, _, _, a_x, _ = Fn.ray_maps(z_all, weights, depth, X, True, None, None, scratch)
            for key, (c0, wdt) in cols.items():
                keep(key, a_x[:, c0:c0 + wdt])
                keep(key + "_s", s_x[:, c0:c0 + wdt])
        if cross_rows is not None:
            a, b = min(max(i, c_lo), j) - i, max(min(j, c_hi), i) - i           # empty where the chunk holds none of the row
            for key, t in (("z_vals", z_all), ("sigmas", out[..., 3]), ("alphas", alphas), ("transparency", transparency),
                           ("sort_idx", p.idx), ("depth", depth), ("std", std)):
                cross[key].append(t[a:max(a, b)].clone())

    if not parts:                       # the maps a rank keeps depend on the chunks it rendered: without one it cannot name them
        raise ValueError(f"view_maps: rank {walk.rank} of {walk.world} has no ray of a view of {rays.shape[0]} rays")
    maps = {key: walk.join(v, v[0].shape[1:]) for key, v in parts.items()}
    result = {"maps": maps, "brdf_type": brdf_type}
    if cross_rows is not None:
        result["cross"] = {key: walk.join(v, v[0].shape[1:]) for key, v in cross.items()}
    host = allreduce_(counters, group=group).cpu()
    c = host[main_row]
    n_an = int(host[0, 5]) if main_row == 0 else 0
    n_lr = int(host[1, 5])
    pct = lambda k, n: 100.0 * k / n if n else None
    result["counters"] = {"an": host[0], "lr": host[1], "main": main_row}
    result["stats"] = {"depth_std": fixed_mean(int(c[0]), int(c[1]), STD_FIX), "depth_std_skipped": int(c[2]),
                       "bad_nr_an%": pct(int(host[0, 3]), n_an), "nr_an0%": pct(int(host[0, 4]), n_an),
                       "bad_nr_lr%": pct(int(host[1, 3]), n_lr)}
    if frame is not None:
        maps["altitude"] = altitude_image(rays.float(), maps["depth"], frame).float()
        maps["nr_from_depth"] = depth_normals(rays, maps["depth"], frame, H, W, "reference" if round_f32 else "exact")
    return result


__all__ = ["ray_maps", "point_normals", "depth_normals", "view_maps", "RAY_MAP_COUNTERS", "CROSS_KEYS"]
