"""brdf_nerf_amd - MI355X (gfx950) native implementation of BRDF-NeRF's ray-batched volume-rendering
hot path (spsbrdf-nerf): fused field MLP (forward/backward), alpha compositing, depth-guided
resampling and RPV / Hapke / GGX BRDF shading as hand-written HIP kernels behind a C ABI
(include/brdfnerf_hip.h), exposed through the reference's own Python surface.

    from brdf_nerf_amd import load_model, render_rays      # replaces `models.load_model`, `rendering.render_rays`

The HIP library is mandatory: importing the compute entry points without it raises.
"""
from .field import SpSBRDFNeRF, load_model  # noqa: F401
from .rendering import render_rays, inference, get_z_vals, cal_weight  # noqa: F401
from . import functions  # noqa: F401
from .relight import render_surface, relight, relight_image, brdf_lobe, directions  # noqa: F401
from .shadows import render_shadow_surface, relight_shadowed, relight_image_shadowed, sun_visibility  # noqa: F401
from .dsm import SceneFrame, Grid, point_cloud, altitude_image, DsmAccumulator, dsm_image, tie_point_dsm, altitude_mae  # noqa: F401
from .metrics import image_psnr, image_ssim, dsm_normals, normal_angle_mae, score_view  # noqa: F401
from .register import register_xy, apply_registration, altitude_mae_xy  # noqa: F401
from .fill import fill_holes, apply_fill  # noqa: F401
from .maps import ray_maps, point_normals, depth_normals, view_maps  # noqa: F401
from .ortho import OrthoAccumulator, ortho_image  # noqa: F401
from .visibility import grid_visibility, point_visibility, view_visibility  # noqa: F401
from .horizon import azimuths, grid_horizon, sky_view_factor, point_sky_view, view_sky_view  # noqa: F401
from .orthophoto import world_pixels, grid_pixels, sample_image, orthophoto, ortho_psnr  # noqa: F401
from .mosaic import orthomosaic  # noqa: F401
from .sweep import altitude_sweep  # noqa: F401
from .aggregate import aggregate_costs  # noqa: F401
from .raycast import cast_rays, grid_to_view, surface_priors  # noqa: F401
from . import camera  # noqa: F401
from .camera import Rpc, view_rays, scene_bounds, ray_table, utm_zone, sun_direction, depth_priors, nearest_lines  # noqa: F401
from .camera import ecef_geodetic  # noqa: F401
from ._lib import set_deterministic  # noqa: F401

__all__ = ["SpSBRDFNeRF", "load_model", "render_rays", "inference", "get_z_vals", "cal_weight", "functions", "set_deterministic",
           "render_surface", "relight", "relight_image", "brdf_lobe", "directions", "render_shadow_surface", "relight_shadowed",
           "relight_image_shadowed", "sun_visibility", "SceneFrame", "Grid", "point_cloud", "altitude_image", "DsmAccumulator",
           "dsm_image", "tie_point_dsm", "altitude_mae", "image_psnr", "image_ssim", "dsm_normals", "normal_angle_mae",
           "score_view",
           "register_xy", "apply_registration", "altitude_mae_xy", "fill_holes", "apply_fill",
           "ray_maps", "point_normals", "depth_normals", "view_maps", "OrthoAccumulator", "ortho_image",
           "grid_visibility", "point_visibility", "view_visibility",
           "azimuths", "grid_horizon", "sky_view_factor", "point_sky_view", "view_sky_view",
           "world_pixels", "grid_pixels", "sample_image", "orthophoto", "ortho_psnr", "orthomosaic",
           "altitude_sweep", "aggregate_costs",
           "cast_rays", "grid_to_view", "surface_priors",
           "camera", "Rpc", "view_rays", "scene_bounds", "ray_table", "utm_zone", "sun_direction", "depth_priors",
           "nearest_lines", "ecef_geodetic"]
