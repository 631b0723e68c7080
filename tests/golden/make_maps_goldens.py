#!/usr/bin/env python
"""Generate the validation-map goldens (tests/golden/maps_*.npz) by running the REFERENCE's functions on synthetic inputs.

Run only where the reference tree is present (BRDFNERF_REFERENCE, default /root/reference, read-only):

    python tests/golden/make_maps_goldens.py

train_utils, metrics and sat_utils are imported with empty stub modules for torchvision, cv2, rasterio, kornia and rpcm, as the
other generators stub their I/O imports: those packages are used only inside functions that are not called here.

Ray fixtures (maps_rays_*): depth-sorted z, weights, depth, a per-sample tensor X with a normal column and unit view vectors
(tests/maps_cases.ray_inputs).  Recorded from the reference: calc_depth_std_2 / calc_depth_std and the np.mean of generate_std_img,
the np.argmin + get_surface_feature sequence of eval.py:409-414, visualize_accumulated_feature's sum (the line of its Accum=True
branch; the function itself goes on into ToImage / cv2), check_vec0 and NormalRegLoss's perc_ng_nr.
Point fixtures (maps_normals_*): calc_normal_from_pts3d on the float32-rounded points, as calc_normal_from_depth_v2 calls it,
without and with valid_depth; `gap` is the largest difference between the float64 statement on the rounded points
(tests/maps_cases.point_normals) and the reference's float32 result - measured here, not derivable; the CPU test allows 8 x gap.

CONDITIONS ON THE INPUTS (not tolerances on any code):
  * no |n . view| below 1e-4 and no normal's length within 1e-5 of 0.99999, so the float32 reading of the reference and the
    float64 one of the rule give the same counts;
  * neither H - 2 nor W - 2 is 3 (upstream's torch.cross without dim then takes the wrong axis);
  * the UTM fixture (coordinates about 3.7e5 / 3.3e6, points about 0.4 m apart) has a cell where the normals of the exact
    points and of the float32-rounded points differ by more than 5 degrees.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import maps_cases as M  # noqa: E402

REF = os.environ.get("BRDFNERF_REFERENCE", "/root/reference")

# name: (R, S, E, normal column, seed)
RAY_FIXTURES = {"maps_rays_s128": (48, 128, 8, 2, 41), "maps_rays_s24": (40, 24, 5, 0, 42)}


def load_reference():
    def stub(name, **attrs):
        mod = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(mod, k, v)
        sys.modules[name] = mod
        return mod
    tv = stub("torchvision")
    tv.transforms = stub("torchvision.transforms")
    stub("cv2", COLORMAP_RAINBOW=0, COLORMAP_JET=0)
    stub("rasterio")
    stub("rpcm")
    k = stub("kornia")
    k.losses = stub("kornia.losses", ssim=None)
    sys.path.insert(0, REF)
    import metrics
    import sat_utils
    import train_utils
    return train_utils, metrics, sat_utils


def run_rays(train_utils, metrics, name):
    R, S, E, nc, seed = RAY_FIXTURES[name]
    z, w, depth, X, view = M.ray_inputs(R, S, E, seed, normal_col=nc)
    n64, v64 = X[:, :, nc:nc + 3].astype(np.float64), view.astype(np.float64)[:, None, :]
    assert np.abs((n64 * v64).sum(-1)).min() >= 1e-4, f"{name}: a normal is within 1e-4 of grazing: choose other inputs"
    assert np.abs(np.linalg.norm(n64, axis=-1) - 0.99999).min() >= 1e-5, f"{name}: a normal's length is within 1e-5 of 0.99999"
    tz, tw, td, tX = (torch.from_numpy(a) for a in (z, w, depth, X))
    var = train_utils.calc_depth_std_2(tz, td, tw)
    std = train_utils.calc_depth_std(tz, td, tw)
    std_mean = np.mean(std.view(R, 1, 1).cpu().numpy())                              # generate_std_img's np.mean(x)
    deviation = torch.abs(tz - torch.tile(td.unsqueeze(-1), (1, S))).cpu().numpy()   # eval.py:409-414
    idx = np.argmin(deviation, axis=1)
    pairs = np.vstack((np.arange(0, idx.shape[0]), idx)).T
    surf = train_utils.get_surface_feature(tX.clone(), pairs)
    accum = torch.sum(tw.unsqueeze(-1) * tX, -2)                                     # visualize_accumulated_feature, Accum=True
    vec0 = train_utils.check_vec0("normal_an_coarse", tX[:, :, nc:nc + 3].contiguous())
    loss = metrics.NormalRegLoss(keyword="normal_an")
    _, _, bad = loss({"normal_an_coarse": tX[:, :, nc:nc + 3].contiguous(), "weights_coarse": tw,
                      "rays_d_coarse": torch.from_numpy(view).reshape(R, 1, 3)})
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, z=z, w=w, depth=depth, X=X, view=view, normal_col=np.int64(nc), ref_var=var.numpy(), ref_std=std.numpy(),
                        ref_std_mean=np.float64(std_mean), ref_idx=idx.astype(np.int64), ref_surf=surf.numpy(),
                        ref_accum=accum.numpy(), ref_vec0=np.float64(vec0), ref_bad=np.float64(float(bad)))
    print(f"{name}: R {R} S {S} E {E}: nr0% {vec0:.4f} bad% {float(bad):.4f} mean std {std_mean:.6f}, {os.path.getsize(path)} bytes")


def point_fixture(name):
    if name == "maps_normals_utm":
        return M.utm_points()                                    # the 9 x 11 probe at UTM-sized coordinates
    return M.utm_points(H=12, W=10, seed=8, east=35.0, north=-60.0, spacing=0.5)


def run_points(sat_utils, name):
    pts = point_fixture(name)
    H, W = pts.shape[:2]
    assert H - 2 != 3 and W - 2 != 3
    rng = np.random.default_rng(H * W)
    valid = np.where(rng.random((H, W)) < 0.2, 0.0, 1.0).astype(np.float32)
    valid[rng.random((H, W)) < 0.1] = np.float32(3e-6)           # below the 1e-5 test, yet not zero
    valid[rng.random((H, W)) < 0.1] = np.float32(0.5)
    p32 = torch.from_numpy(pts).type(torch.FloatTensor)          # calc_normal_from_depth_v2's cast
    ref, ones = sat_utils.calc_normal_from_pts3d(p32.reshape(H, W, 3), Flatten=False)
    ref_v, ref_valid = sat_utils.calc_normal_from_pts3d(p32.reshape(H, W, 3), valid_depth=torch.from_numpy(valid), Flatten=False)
    assert torch.equal(ref, ref_v) and bool((ones == 1).all())
    ref = ref.numpy()
    mine = M.point_normals(pts, round_f32=True)
    gap = float(np.abs(mine.astype(np.float64) - ref.astype(np.float64)).max())
    assert gap < 1e-5, f"{name}: the statement is {gap} from the reference"
    assert np.array_equal(M.valid_normal(valid).view(np.int32), ref_valid.numpy().view(np.int32))
    turn = float(M.angle_deg(M.point_normals(pts, round_f32=False), mine)[1:-1, 1:-1].max())
    if name == "maps_normals_utm":
        assert turn > 5.0, f"{name}: the float32 rounding turns no normal by 5 degrees ({turn}): choose other inputs"
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, points=pts, valid=valid, ref_normals=ref, ref_valid=ref_valid.numpy(), gap=np.float64(gap),
                        turn=np.float64(turn))
    print(f"{name}: {H} x {W}: gap to the reference {gap:.3e}, float32 rounding turns a normal by up to {turn:.2f} degrees, "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    tu, met, su = load_reference()
    for fixture in RAY_FIXTURES:
        run_rays(tu, met, fixture)
    for fixture in M.NORMAL_GOLDENS:
        run_points(su, fixture)
