"""The reference's per-view evaluation line on the device: masked and rescaled PSNR, SSIM, and the normal-angle MAE of the DSM.

The reference prints `psnr / ssim / mae, mae_in, mae_out, mae_nr` and `psnr_scl / ssim_scl` per view (eval.py:467-479).  The
unmasked PSNR is render_image's and the altitude MAE is dsm.altitude_mae's; the rest is here:

  image_psnr         metrics.py:292-325 with valid_mask and scl=True, as eval.py:469 calls it (plain torch)
  image_ssim         metrics.py:327-341 (kornia 0.5.3 ssim, 3 x 3 Gaussian window, max_val = max(gt)) as eval.py:471 calls it:
                     bn_ssim_map, a float64 rule with an INTEGER sum - no kornia, no copy to the host
  dsm_normals        calc_normal_from_pts3d on get_pts3d_from_dsm (sat_utils.py:16-50, 175-183): bn_grid_normals
  normal_angle_mae   mae_nr, the mean angle between the normals of two DSMs (sat_utils.py:164-173, 251-257, 341, 346):
                     bn_normal_angle, integer sums again
  score_view         one call for the whole line: render, DSM, and every number above

The sums are integers (SSIM in units of 2^-30, angles in units of 2^-20 degree), so a number's bits do not depend on the block
order, on how an image's rows are split (rows=), or on how many GPUs shared the view: ranks merge by one SUM all-reduce.

The SSIM rule (include/brdfnerf_hip.h states it operation by operation) follows kornia 0.5.3 as documented; it was not checked
against the package, which this project does not depend on.  The xy registration of dsmr is register.py's (score_view's
register="xy").  Not covered: GeoTIFF I/O, LPIPS (commented out upstream).
"""
import math

import torch

from . import _lib as L
from . import functions as Fn

_LAYOUTS = ("reference", "image")
_BORDERS = {"reference": 0, "nan": 1}
SSIM_FIX = 2.0 ** 30
ANGLE_FIX = 2.0 ** 20


def gaussian_window(window, sigma=1.5):
    """The `window` normalised 1-D Gaussian weights in float64: exp(-x^2 / (2 sigma^2)) over their sum, x = k - window // 2."""
    check_window(window)
    e = [math.exp(-float((k - window // 2) ** 2) / (2.0 * sigma ** 2)) for k in range(window)]
    s = sum(e)
    return [v / s for v in e]


def check_window(window, H=None, W=None):
    if not isinstance(window, int) or window % 2 == 0 or not 3 <= window <= L.BN_SSIM_MAX_WINDOW:
        raise ValueError(f"ssim: window {window!r} must be odd, 3 to {L.BN_SSIM_MAX_WINDOW}")
    if H is not None and (H <= window // 2 or W <= window // 2):
        raise ValueError(f"ssim: image {H} x {W} is too small for the reflect padding of window {window} (needs more than "
                         f"{window // 2} rows and columns)")


def layout_strides(layout, C, H, W):
    """Element strides (plane, row, col) of plane c, row r, column col in an (H W, C) ray-major buffer.
    'reference': eval.py:471's .view(1, C, H, W) - a reinterpretation, not a permute: plane c is flat[c H W : (c + 1) H W].
    'image': the true image, channel c of pixel (r, col) at flat[(r W + col) C + c]."""
    if layout not in _LAYOUTS:
        raise ValueError(f"ssim: layout {layout!r} ('reference' or 'image')")
    return (H * W, W, 1) if layout == "reference" else (1, C * W, C)


def _mask_hw(mask, H, W, device):
    if mask is None:
        return None
    mask = torch.as_tensor(mask)
    if mask.numel() != H * W:
        raise ValueError(f"mask of {mask.numel()} elements for an image of {H} x {W}")
    return (mask.reshape(H, W) != 0).to(device=device, dtype=torch.uint8).contiguous()


@torch.no_grad()
def image_psnr(rgb, target, mask=None, scl=False):
    """metrics.py:292-325 as eval.py:469 calls it: -10 log10(mean((rgb - target)^2 / max(target)^2)), the mean over the elements
    the mask keeps and the normaliser the maximum of the WHOLE target, as upstream.  mask: one value per pixel (rows of rgb;
    upstream tiles it over the channels) or per element.  scl: also the PSNR of both images divided by max(target) (sclimg).
    Plain torch on the tensors' device.  -> (psnr, psnr_scl or -1); without a mask psnr is losses.psnr's."""
    keep = None
    if mask is not None:
        keep = torch.as_tensor(mask).to(rgb.device) != 0
        if keep.numel() == rgb.numel():
            keep = keep.reshape(rgb.shape)
        elif keep.numel() * rgb.shape[-1] == rgb.numel():
            keep = keep.reshape(rgb.shape[:-1] + (1,)).expand(rgb.shape)
        else:
            raise ValueError(f"image_psnr: mask of {keep.numel()} elements for an image of shape {tuple(rgb.shape)}")

    def one(a, b):
        value = (a - b) ** 2 / (torch.max(b) ** 2)
        if keep is not None:
            value = value[keep]
        return -10.0 * torch.log10(torch.mean(value))

    if not scl:
        return one(rgb, target), -1
    top = torch.max(target)
    return one(rgb, target), one(rgb / top, target / top)


def _ssim_sums(rgb, target, H, W, mask, window, layout, scl, rows, want_map):
    """-> (sums (2, 3) int64 on the device: [plain, rescaled] x [sum, count, skipped], maps or None, max_val)."""
    if rgb.shape != target.shape or rgb.numel() % (H * W) != 0 or rgb.numel() == 0:
        raise ValueError(f"ssim: images {tuple(rgb.shape)} and {tuple(target.shape)} are not both {H} x {W} pixels")
    C = rgb.numel() // (H * W)
    check_window(window, H, W)
    strides = layout_strides(layout, C, H, W)
    if rows is not None and not 0 <= rows[0] <= rows[1] <= H:
        raise ValueError(f"ssim: rows {tuple(rows)} outside [0, {H}]")
    rgb, target = Fn._f32(rgb), Fn._f32(target)
    m = _mask_hw(mask, H, W, rgb.device)
    planes = target.reshape(C, H, W) if layout == "reference" else target.reshape(H, W, C).permute(2, 0, 1)
    max_val = float(torch.max(planes if m is None else planes * m))
    if not math.isfinite(max_val):
        raise ValueError(f"ssim: max_val = max(target * mask) = {max_val} is not finite")
    g = gaussian_window(window)
    sums = torch.zeros((2, 3), dtype=torch.int64, device=rgb.device)
    maps = [None, None]
    for k, (div, mv) in enumerate([(1.0, max_val), (max_val, 1.0)][:2 if scl else 1]):
        if want_map:
            maps[k] = torch.full((C, H, W), float("nan"), dtype=torch.float32, device=rgb.device)
        Fn.ssim_map(rgb, target, C, H, W, strides, m, div, mv, window, g, sums[k], rows=rows, out=maps[k])
    return sums, maps, max_val


@torch.no_grad()
def image_ssim(rgb, target, H, W, mask=None, window=3, layout="reference", scl=False, rows=None, want_map=False):
    """metrics.py:327-341 as eval.py:471 calls it: the mean of the SSIM index map of the two masked images, Gaussian window
    (sigma 1.5) of `window` x `window` taps, reflect padding, max_val = max(target * mask).  rgb, target: (H W, C) float32 on
    the device (any shape of H W C elements).
    layout 'reference' reproduces eval.py:471 exactly: its .view(1, 3, H, W) of the (H W, 3) buffer is a reinterpretation,
    not a permute, so plane c is flat[c H W : (c + 1) H W] and the mask multiplies THOSE planes; 'image' is the true image.
    Both go through element strides: nothing is copied.  mask: (H, W) or (H W,), nonzero keeps.  scl: also the SSIM of both
    images divided by max_val with max_val = 1 (sclimg), a second launch.  rows = (row0, row1): only those output rows (the
    bands of several calls or ranks add up in `sums`).  want_map: the float32 index map(s) (C, H, W), NaN outside `rows`.
    -> (ssim, ssim_scl or -1, info): each sum / (count 2^30) in float64 on the host, NaN when no cell counted;
    info = {"skipped", "sums" (2, 3) int64 [plain, rescaled] x [sum, count, skipped], "max_val", "map", "map_scl"}.
    A cell whose index is not finite is left out of the mean and counted in `skipped` (upstream's mean would be NaN)."""
    sums, maps, max_val = _ssim_sums(rgb, target, H, W, mask, window, layout, scl, rows, want_map)
    host = sums.cpu()
    ssim, ssim_scl = (Fn.fixed_mean(s, n, SSIM_FIX) for s, n, _ in host.tolist())
    info = {"skipped": int(host[0, 2]), "sums": host, "max_val": max_val, "map": maps[0], "map_scl": maps[1]}
    return ssim, (ssim_scl if scl else -1), info


@torch.no_grad()
def dsm_normals(dsm, resolution):
    """The normals of an altitude grid as the reference forms them (calc_normal_from_pts3d on get_pts3d_from_dsm, sat_utils.py:
    16-50, 175-183): dsm (H, W) -> (H, W, 3) float32 on the device, zero on the border, NaN where a NaN altitude is read.
    The reference's axes are kept: y grows with the row, so the frame is left-handed and flat ground gives n_z = -1; the angle
    between two grids does not depend on that."""
    dsm = torch.as_tensor(dsm)
    if dsm.dim() != 2:
        raise ValueError(f"dsm_normals: an (H, W) grid, not {tuple(dsm.shape)}")
    if not (resolution > 0 and math.isfinite(resolution)):
        raise ValueError(f"dsm_normals: resolution {resolution} must be positive")
    return Fn.grid_normals(Fn._f32(dsm), resolution)


@torch.no_grad()
def normal_angle_mae(dsm, gt, resolution, mask=None, border="reference"):
    """mae_nr of the reference (sat_utils.py:251-257, 341): the mean angle in degrees between the normals of the predicted and
    the ground-truth DSM on the SAME grid, NaN cells left out (nanmean).  mask (nonzero inside; MaskDoD, :346): also the means
    over the cells inside and outside, else both -1 as upstream.  border 'reference': border cells have zero normals and so count
    as 90 degrees, as upstream; 'nan': they are left out.
    The z-registration shift of altitude_mae is NOT applied: normals are differences of altitudes, and the reference's shifted
    float32 grid differs from the unshifted one only by rounding.
    -> {"mae_nr", "diff_nr" (H, W) float32 angle map, "mae_nr_in", "mae_nr_out", "sums" (6,) int64}."""
    if border not in _BORDERS:
        raise ValueError(f"normal_angle_mae: border {border!r} ('reference' or 'nan')")
    dsm, gt = torch.as_tensor(dsm), torch.as_tensor(gt)
    if dsm.shape != gt.shape or dsm.dim() != 2:
        raise ValueError(f"normal_angle_mae: dsm {tuple(dsm.shape)} and ground truth {tuple(gt.shape)} are not on one grid")
    H, W = dsm.shape
    if mask is not None and torch.as_tensor(mask).numel() != H * W:
        raise ValueError(f"normal_angle_mae: mask of {torch.as_tensor(mask).numel()} cells for a grid of {H} x {W}")
    gt = gt.to(dsm.device)
    angle, sums = Fn.normal_angle(dsm_normals(dsm, resolution), dsm_normals(gt, resolution), _mask_hw(mask, H, W, dsm.device),
                                  _BORDERS[border])
    s = sums.cpu()
    mean = [Fn.fixed_mean(t, n, ANGLE_FIX) for t, n in s.reshape(3, 2).tolist()]            # all, inside, outside
    return {"mae_nr": mean[0], "diff_nr": angle, "sums": s, "mae_nr_in": mean[1] if mask is not None else -1,
            "mae_nr_out": mean[2] if mask is not None else -1}


@torch.no_grad()
def score_view(models, args, rays, rgbs, H, W, mask=None, frame=None, gt_dsm=None, grid=None, dsm_mask=None, group=None,
               window=3, layout="reference", radius=1, footprint="disc", resolution=0.5, register="z", sun_dir=None, shadow_dsm=None,
               shadow_eps=0.0, cast_dsm=None, **render_kw):
    """The reference's evaluation line of one view (eval.py:467-479) in one call: psnr, psnr_scl, ssim, ssim_scl and - with a
    `frame` - the DSM, and with `gt_dsm` on that grid mae, mae_in, mae_out (altitude_mae) and mae_nr (normal_angle_mae).
    rays (H W, >= 8), rgbs (H W, 3) the ground truth, mask the view's valid pixels ((H, W) or (H W,)), dsm_mask the DSM's
    inside cells; render_kw: chunk, apply_brdf, cos_irra_on, ... as render_image.
    The view is rendered ONCE, by evaluate.render_image, so `rgb` and `depth` are bitwise render_image's; with a frame each
    rank then splats its own share of the depths exactly as dsm.dsm_image does (same accumulator, same merge), so `dsm` is
    bitwise dsm_image's after the same torch.manual_seed.  Under data parallelism the image is the gathered one; each rank
    scores its own band of rows (image_ssim's rows=) and one SUM all-reduce of the integer triples merges them.
    register: 'z' - the z-only registration the reference falls back to without dsmr (altitude_mae; normals of the unshifted DSM);
    'xy' - its real path with dsmr (sat_utils.py:239-252): mae, mae_in, mae_out and shift from register.altitude_mae_xy, mae_nr*
    from the normals of the REGISTERED DSM, and also "dx", "dy", "rdsm".
    sun_dir (3,) = (east, north, up) towards the sun (needs a 'utm' frame): the PSNR split into sunlit and shadowed pixels by the
    GEOMETRIC shadow of a surface model (visibility.view_visibility of the view's own depth; shadow_eps its eps).  The raster
    marched is the first available of shadow_dsm (on `grid`), gt_dsm, fill_holes(dsm)["filled"]; "shadow_source" names it
    ('shadow_dsm', 'gt_dsm' or 'dsm').  Every rank marches all pixels of the gathered depth: no collective.  Adds "visibility"
    (H W,) uint8 (0 shadowed, 1 sunlit, 2 no data), "shadow_fraction" = shadowed / (shadowed + sunlit) over the pixels the mask
    keeps (NaN without one), "psnr_sunlit" and "psnr_shadow" = image_psnr under mask AND visibility == 1 / == 0, with upstream's
    whole-target normaliser; a class without a pixel gives -1.  sun_dir=None: nothing changes, no key and no bit.
    cast_dsm (needs a 'utm' frame and `grid`): a ground-truth surface model (grid.height, grid.width) float32 seen from the very
    pixels (raycast.cast_rays): "depth_gt" (H W,) float32, NaN where a ray met nothing, "cast_state" (H W,) uint8, "depth_mae" =
    the mean of |depth - depth_gt| range, in metres along the ray, and "alt_mae_view" = the mean of |altitude_image(rays, depth) -
    altitude_image(rays, depth_gt)|, both over the pixels the mask keeps and that were hit, from an int64 sum of round(|e| 2^20)
    and a count - independent of order and ranks; NaN without such a pixel.  cast_dsm=None: no key and no bit changes.
    -> {"psnr", "psnr_scl", "ssim", "ssim_scl", "ssim_skipped", "ssim_sums", "rgb", "depth"} (+ "dsm", "count", "grid",
    "skipped" with a frame; + "mae", "mae_in", "mae_out", "mae_nr", "mae_nr_in", "mae_nr_out", "shift" with gt_dsm)."""
    from .distributed import allreduce_, row_band
    from .dsm import DsmAccumulator, _cloud_grid, altitude_mae
    from .evaluate import render_image
    from .viewwalk import ViewWalk
    if rays.shape[0] != H * W:
        raise ValueError(f"score_view: {rays.shape[0]} rays for a view of {H} x {W}")
    if register not in ("z", "xy"):
        raise ValueError(f"score_view: register {register!r} ('z' or 'xy')")
    if gt_dsm is not None and frame is None:
        raise ValueError("score_view: gt_dsm needs the scene's frame (frame=) to build the DSM it is compared with")
    if sun_dir is not None:
        if frame is None:
            raise ValueError("score_view: sun_dir needs the scene's frame (frame=) to place the view's pixels on the surface model")
        if frame.cs == "ecef":
            raise ValueError("score_view: sun_dir is not served on an 'ecef' frame: its world axes are not (east, north, up)")
        sun_dir = Fn._vis_dirs("score_view", sun_dir)
        if sun_dir.shape[0] != 1:
            raise ValueError(f"score_view: sun_dir is ONE direction (3,), not {tuple(sun_dir.shape)}")
        Fn._vis_scalars("score_view", resolution, shadow_eps, 0.0)
        if shadow_dsm is not None and grid is not None and tuple(torch.as_tensor(shadow_dsm).shape) != (grid.height, grid.width):
            raise ValueError(f"score_view: shadow_dsm {tuple(torch.as_tensor(shadow_dsm).shape)} is not on the grid of "
                             f"{grid.height} x {grid.width} cells")
    if cast_dsm is not None:
        if frame is None or grid is None:
            raise ValueError("score_view: cast_dsm needs the scene's frame (frame=) and the grid the surface model is on (grid=)")
        if frame.cs == "ecef":
            raise ValueError("score_view: cast_dsm is not served on an 'ecef' frame: its world axes are not (east, north, up)")
        if tuple(torch.as_tensor(cast_dsm).shape) != (grid.height, grid.width):
            raise ValueError(f"score_view: cast_dsm {tuple(torch.as_tensor(cast_dsm).shape)} is not on the grid of "
                             f"{grid.height} x {grid.width} cells")
    check_window(window, H, W)
    view = render_image(models, args, rays, None, keys=("rgb", "depth"), group=group, **render_kw)
    rgb, depth = view["rgb"], view["depth"]
    rgbs = rgbs.to(rgb.device)
    res = {"rgb": rgb, "depth": depth}
    p, p_scl = image_psnr(rgb, rgbs, mask=mask, scl=True)
    res["psnr"], res["psnr_scl"] = float(p), float(p_scl)
    sums, _, _ = _ssim_sums(rgb, rgbs, H, W, mask, window, layout, True, row_band("score_view", H, None, group), False)
    host = allreduce_(sums, group=group).cpu()
    ssim, ssim_scl = (Fn.fixed_mean(s, n, SSIM_FIX) for s, n, _ in host.tolist())
    res.update(ssim=ssim, ssim_scl=ssim_scl, ssim_skipped=int(host[0, 2]), ssim_sums=host)
    if frame is not None:
        walk = ViewWalk(rays.shape[0], render_kw.get("chunk") or args.chunk, group)     # render_image's: the rays this rank rendered
        if grid is None:
            grid = _cloud_grid(rays, depth, frame, resolution)
        acc = DsmAccumulator(grid, rays.device, radius, footprint).add(rays[walk.lo:walk.hi], depth[walk.lo:walk.hi], frame).merge(group)
        dsm, count = acc.result()
        res.update(dsm=dsm, count=count, grid=grid, skipped=acc.skipped)
        if gt_dsm is not None:
            gt_dsm = torch.as_tensor(gt_dsm).to(dsm.device)
            if register == "xy":
                from .register import altitude_mae_xy
                alt = altitude_mae_xy(dsm, gt_dsm, mask=dsm_mask, group=group)
                nr = normal_angle_mae(alt["rdsm"], gt_dsm, grid.resolution, mask=dsm_mask)
                res.update(dx=alt["dx"], dy=alt["dy"], rdsm=alt["rdsm"])
            else:
                alt = altitude_mae(dsm, gt_dsm, mask=dsm_mask)
                nr = normal_angle_mae(dsm, gt_dsm, grid.resolution, mask=dsm_mask)
            res.update(mae=alt["mae"], shift=alt["shift"], mae_in=alt.get("mae_in", -1), mae_out=alt.get("mae_out", -1),
                       mae_nr=nr["mae_nr"], mae_nr_in=nr["mae_nr_in"], mae_nr_out=nr["mae_nr_out"])
        if sun_dir is not None:
            res.update(_shadow_split(rays, rgb, rgbs, depth, mask, frame, grid, dsm, gt_dsm, shadow_dsm, sun_dir, shadow_eps, group))
        if cast_dsm is not None:
            res.update(_cast_errors(rays, depth, mask, frame, grid, cast_dsm, group))
    return res


def _cast_errors(rays, depth, mask, frame, grid, cast_dsm, group):
    """score_view's cast_dsm keys: the surface model's depth along the view's own rays and the two image-space MAEs."""
    from .dsm import altitude_image
    from .raycast import cast_rays
    rays32 = Fn._f32(rays)
    cast = cast_rays(rays32, frame, Fn._f32(torch.as_tensor(cast_dsm).to(rays.device)), grid, group=group)
    depth_gt, hit = cast["depth"], cast["cell"] >= 0
    keep = hit if mask is None else hit & (torch.as_tensor(mask).to(hit.device).reshape(-1) != 0)
    if keep.numel() != depth.numel():
        raise ValueError(f"score_view: mask of {keep.numel()} elements for {depth.numel()} pixels")
    d = depth.reshape(-1).to(depth_gt.device)
    errors = {"depth_mae": (d.double() - depth_gt.double()).abs() * frame.range,
              "alt_mae_view": (altitude_image(rays32, d, frame) - altitude_image(rays32, depth_gt, frame)).abs()}
    out = {"depth_gt": depth_gt, "cast_state": cast["state"]}
    for key, e in errors.items():
        sel = keep & torch.isfinite(e)
        q = torch.round(torch.where(sel, e, torch.zeros_like(e)) * ANGLE_FIX).to(torch.int64)
        out[key] = Fn.fixed_mean(int(q.sum()), int(sel.sum()), ANGLE_FIX)
    return out


def _shadow_split(rays, rgb, rgbs, depth, mask, frame, grid, dsm, gt_dsm, shadow_dsm, sun_dir, eps, group):
    """score_view's sun_dir keys: the geometric shadow of the view's pixels and the PSNR of either class."""
    from .fill import fill_holes
    from .visibility import BLOCKED, VISIBLE, view_visibility
    if shadow_dsm is not None:
        raster, source = torch.as_tensor(shadow_dsm).to(dsm.device), "shadow_dsm"
        if tuple(raster.shape) != (grid.height, grid.width):
            raise ValueError(f"score_view: shadow_dsm {tuple(raster.shape)} is not on the grid of {grid.height} x {grid.width} cells")
    elif gt_dsm is not None:
        raster, source = gt_dsm, "gt_dsm"
    else:
        raster, source = fill_holes(dsm, group=group)["filled"], "dsm"
    vis = view_visibility(rays, depth, frame, Fn._f32(raster).contiguous(), grid, sun_dir, eps)["visible"][0]
    keep = torch.ones_like(vis, dtype=torch.bool) if mask is None else (torch.as_tensor(mask).to(vis.device).reshape(-1) != 0)
    if keep.numel() != vis.numel():
        raise ValueError(f"score_view: mask of {keep.numel()} elements for {vis.numel()} pixels")
    out = {"visibility": vis, "shadow_source": source}
    lit, dark = keep & (vis == VISIBLE), keep & (vis == BLOCKED)
    n_lit, n_dark = int(lit.sum()), int(dark.sum())
    out["shadow_fraction"] = n_dark / (n_lit + n_dark) if n_lit + n_dark else float("nan")
    out["psnr_sunlit"] = float(image_psnr(rgb, rgbs, mask=lit)[0]) if n_lit else -1
    out["psnr_shadow"] = float(image_psnr(rgb, rgbs, mask=dark)[0]) if n_dark else -1
    return out


__all__ = ["image_psnr", "image_ssim", "dsm_normals", "normal_angle_mae", "score_view", "gaussian_window", "layout_strides"]
