"""GPU tests of the validation maps (brdf_nerf_amd/maps.py, bn_ray_maps / bn_point_normals).  Run on the MI355X box with
`pytest -m gpu`.  The kernels are held bit for bit to the numpy statements of tests/maps_cases.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import maps_cases as M
from test_gpu_parity import DEV, _free_port

pytestmark = pytest.mark.gpu
VIEW_H, VIEW_W, CHUNK = 12, 10, 50          # 120 rays: chunks of 50, 50 and 20


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


def same(a, b):
    """Bitwise on float32, NaN positions equal (the payload of an arithmetic NaN is the machine's)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.int32)[~nan], b.view(np.int32)[~nan])


def run(z, w, depth, X=None, normal_col=None, view=None, accumulate=False):
    from brdf_nerf_amd import functions as Fn
    idx, surf, var, std, accum, counters = Fn.ray_maps(dev(z), dev(w), dev(depth), X, accumulate, normal_col,
                                                       None if view is None else dev(view))
    np_ = lambda t: None if t is None else t.cpu().numpy()
    return {"surf_idx": np_(idx), "surf": np_(surf), "var": np_(var), "std": np_(std), "accum": np_(accum),
            "counters": dict(zip(M.COUNTERS, (int(v) for v in counters.cpu())))}


def check(got, want, what):
    assert got["surf_idx"].dtype == np.int32 and np.array_equal(got["surf_idx"], want["surf_idx"]), what
    for k in ("surf", "accum"):
        assert (got[k] is None) == (want[k] is None), (what, k)
        if want[k] is not None:
            assert np.array_equal(M.bits(got[k]), M.bits(want[k])) if k == "surf" else same(got[k], want[k]), (what, k)
    assert same(got["var"], want["var"]) and same(got["std"], want["std"]), what
    assert got["counters"] == want["counters"], (what, got["counters"], want["counters"])


@pytest.mark.parametrize("S", M.RAY_S)
def test_ray_maps_bit_equal_to_the_statement(S):
    """Every R in {1, 63, 64, 65, 257} x E in {0, 1, 3, 16, 28} at this S, with and without accum (the X tile then holds all E
    channels or only the normal's three), the normal column last in X."""
    for R in M.RAY_R:
        for E in M.RAY_E:
            nc = E - 3 if E >= 3 else None
            z, w, depth, X, view = M.ray_inputs(R, S, E, 1000 * S + 10 * R + E, normal_col=nc)
            for accumulate in ((False, True) if E else (False,)):
                got = run(z, w, depth, dev(X) if E else None, nc, view if nc is not None else None, accumulate)
                check(got, M.ray_statement(z, w, depth, X if E else None, nc, view, accumulate), (R, S, E, accumulate))


def test_strided_column_slice_is_read_in_place():
    """X = rows[..., 5:21] of (R, S, 28) field rows: no copy, strides (28 S, 28, 1); and a slice with a sample stride."""
    z, w, depth, rows, view = M.ray_inputs(130, 65, 28, 77, normal_col=18)
    big = dev(rows)
    X = big[..., 5:21]
    assert not X.is_contiguous() and X.data_ptr() == big.data_ptr() + 20
    for accumulate in (False, True):
        check(run(z, w, depth, X, 13, view, accumulate), M.ray_statement(z, w, depth, rows[..., 5:21], 13, view, accumulate), accumulate)
    wide = dev(np.concatenate([rows, rows], axis=1))[:, ::2]                 # every other sample of a (R, 2 S, 28) buffer
    assert wide.stride(1) == 56
    check(run(z, w, depth, wide, 18, view, True), M.ray_statement(z, w, depth, np.concatenate([rows, rows], axis=1)[:, ::2], 18, view, True), "step")


def test_ties_and_depth_outside_the_samples():
    """z symmetric about depth: the FIRST of two exactly tied samples; depth below z_0 -> 0, above z_{S-1} -> S - 1."""
    z, w, depth = M.tie_case()
    got = run(z, w, depth)
    check(got, M.ray_statement(z, w, depth), "ties")
    S = z.shape[1]
    assert (got["surf_idx"][1::3] == 0).all() and (got["surf_idx"][2::3] == S - 1).all()
    dev_ = np.abs(z[0::3] - depth[0::3, None])
    assert (got["surf_idx"][0::3] == np.argmax(dev_ == dev_.min(1, keepdims=True), 1)).all()         # the first of the two
    assert ((dev_ == dev_.min(1, keepdims=True)).sum(1) == 2).all()


def test_nan_inf_and_zero_weights():
    """NaN and inf in z (the first NaN wins; an all-inf row gives 0), all-zero weights (std 0, counted), a NaN weight (std NaN,
    std_skipped)."""
    z, w, depth, X, view = M.ray_inputs(70, 65, 3, 9, normal_col=0)
    z[3, 40] = z[3, 12] = np.nan
    z[4, 64] = np.nan
    z[5, 0] = -np.inf
    z[6, :] = np.inf
    z[7, 10] = np.inf
    w[8, :] = 0.0
    w[9, 33] = np.nan
    w[10, 5] = np.inf
    X[11, 7, :] = np.nan                                    # a NaN normal: counted as not unit, not counted as facing away
    got = run(z, w, depth, dev(X), 0, view, True)
    want = M.ray_statement(z, w, depth, X, 0, view, True)
    check(got, want, "nan")
    assert got["surf_idx"][3] == 12 and got["surf_idx"][4] == 64 and got["surf_idx"][6] == 0
    assert got["std"][8] == 0.0 and np.isnan(got["std"][9])
    assert got["counters"]["std_skipped"] == want["counters"]["std_skipped"] >= 5


def test_surface_copy_keeps_every_bit():
    """-0.0, denormals, infinities and NaN payloads in X come out of `surf` with their 32 bits."""
    z, w, depth, X, _ = M.ray_inputs(65, 33, 4, 21)
    raw = X.view(np.uint32)
    raw[:, :, 0] = 0x80000000                               # -0.0
    raw[:, :, 1] = np.arange(65 * 33, dtype=np.uint32).reshape(65, 33) + 1       # denormals
    raw[:, :, 2] = 0x7fc12345                               # a NaN with a payload
    raw[::2, :, 3] = 0xff800000                             # -inf
    got = run(z, w, depth, dev(X))
    want = M.surf(X, M.surf_idx(z, depth))
    assert np.array_equal(got["surf"].view(np.uint32), want.view(np.uint32))
    assert (got["surf"].view(np.uint32)[:, 0] == 0x80000000).all() and (got["surf"].view(np.uint32)[:, 2] == 0x7fc12345).all()


def test_counters_of_ray_subsets_add_up():
    """Three uneven subsets of the rays, each its own launch into its own counters: they add to the whole launch's, and into ONE
    counter array they accumulate to the same."""
    from brdf_nerf_amd import functions as Fn
    z, w, depth, X, view = M.ray_inputs(257, 65, 16, 13, normal_col=13)
    whole = run(z, w, depth, dev(X), 13, view)["counters"]
    total = dict.fromkeys(M.COUNTERS, 0)
    shared = torch.zeros(6, dtype=torch.int64, device=DEV)
    for a, b in ((0, 1), (1, 130), (130, 257)):
        part = run(z[a:b], w[a:b], depth[a:b], dev(X[a:b]), 13, view[a:b])["counters"]
        total = {k: total[k] + part[k] for k in total}
        Fn.ray_maps(dev(z[a:b]), dev(w[a:b]), dev(depth[a:b]), dev(X[a:b]), False, 13, dev(view[a:b]), shared)
    assert total == whole and dict(zip(M.COUNTERS, (int(v) for v in shared.cpu()))) == whole
    assert whole["nr_total"] == 257 * 65 and 0 < whole["bad_nr"] < whole["nr_total"] and whole["nr0"] > 0


@pytest.mark.parametrize("name", M.RAY_GOLDENS)
def test_ray_maps_on_the_goldens(name):
    """The kernel on the reference's inputs: the statement bit for bit, and so the reference's index and surface sample."""
    g = M.golden(name)
    nc = int(g["normal_col"])
    got = run(g["z"], g["w"], g["depth"], dev(g["X"]), nc, g["view"], True)
    check(got, M.ray_statement(g["z"], g["w"], g["depth"], g["X"], nc, g["view"], True), name)
    assert np.array_equal(got["surf_idx"].astype(np.int64), g["ref_idx"]) and np.array_equal(M.bits(got["surf"]), M.bits(g["ref_surf"]))


def normals(points, valid=None, round_f32=True):
    from brdf_nerf_amd import functions as Fn
    n, v = Fn.point_normals(dev(points), None if valid is None else dev(valid), round_f32)
    return n.cpu().numpy(), None if v is None else v.cpu().numpy()


@pytest.mark.parametrize("shape", M.POINT_SHAPES)
def test_point_normals_bit_equal_to_the_statement(shape):
    """Both round_f32 values, valid on and off, on UTM-sized points of every shape; coincident points (the floor of the
    normalisation applies: zero vectors) and a NaN point (the up to five cells that read it are NaN)."""
    H, W = shape
    pts = M.utm_points(H, W, seed=H * 1000 + W)
    if H >= 3 and W >= 3:
        pts[1, 1] = pts[1, 0]                               # coincident neighbours
        if W > 4:
            pts[H // 2, W - 2] = pts[H // 2, W - 3]
            pts[H // 2, 3 if W > 8 else 2, 1] = np.nan
    rng = np.random.default_rng(H + W)
    valid = rng.choice(np.array([0.0, 1.0, 1.0, 0.5, 3e-6], dtype=np.float32), size=(H, W))
    for round_f32 in (True, False):
        got, none = normals(pts, None, round_f32)
        assert none is None and got.dtype == np.float32 and same(got, M.point_normals(pts, round_f32)), (shape, round_f32)
        got_v, vout = normals(pts, valid, round_f32)
        assert same(got_v, got) and np.array_equal(M.bits(vout), M.bits(M.valid_normal(valid)))
    if W > 8:
        assert np.isnan(got[H // 2, 3]).all() and np.isnan(got).any(-1).sum() <= 5


def test_point_normals_on_the_goldens_and_both_precisions():
    """On the reference's fixtures: within 8 x the stored gap of the reference's float32 normals; on the UTM one 'exact' and
    'reference' differ by more than 5 degrees somewhere."""
    from brdf_nerf_amd import point_normals
    for name in M.NORMAL_GOLDENS:
        g = M.golden(name)
        ref, vout = point_normals(dev(g["points"]), dev(g["valid"]))
        exact, _ = point_normals(dev(g["points"]), precision="exact")
        assert np.abs(ref.cpu().numpy().astype(np.float64) - g["ref_normals"]).max() <= 8 * float(g["gap"])
        assert np.array_equal(M.bits(vout.cpu().numpy()), M.bits(g["ref_valid"]))
        assert same(exact.cpu().numpy(), M.point_normals(g["points"], False))
        if name == "maps_normals_utm":
            assert M.angle_deg(exact.cpu().numpy(), ref.cpu().numpy())[1:-1, 1:-1].max() > 5.0


def test_point_normals_of_grid_points_are_grid_normals():
    """On P = (c res, r res, z) bn_point_normals equals bn_grid_normals bit for bit (one chain, one header)."""
    from brdf_nerf_amd import functions as Fn
    rng = np.random.default_rng(4)
    for H, W, res in ((33, 65, 0.5), (64, 64, 0.3), (3, 300, 1.0)):
        z = (30.0 + 3.0 * rng.standard_normal((H, W))).astype(np.float32)
        z[H // 2, W // 2] = np.nan
        want = Fn.grid_normals(dev(z), res).cpu().numpy()
        for round_f32 in (False,):
            got, _ = normals(M.grid_points(z, res), None, round_f32)
            assert same(got, want), (H, W)


def test_refusals():
    """BN_EINVAL through the raw ABI, nothing launched or written; ValueError from the wrappers on device tensors."""
    from brdf_nerf_amd import _lib as L
    from brdf_nerf_amd import functions as Fn
    lib = L.lib()
    R, S, E = 10, 8, 5
    z, w, d = (torch.rand(R, S, device=DEV), torch.rand(R, S, device=DEV), torch.rand(R, device=DEV))
    X, view = torch.rand(R, S, E, device=DEV), torch.rand(R, 3, device=DEV)
    idx = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(6, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(z_=p(z), w_=p(w), d_=p(d), X_=p(X), xr=S * E, xs=E, xc=1, nc=-1, v_=p(view), vs=3, R_=R, S_=S, E_=E, surf=None, accum=None,
             cnt_=p(cnt)):
        return lib.bn_ray_maps(z_, w_, d_, X_, xr, xs, xc, nc, v_, vs, R_, S_, E_, p(idx), surf, None, None, accum, cnt_, None)

    for kw in (dict(z_=None), dict(w_=None), dict(d_=None), dict(cnt_=None), dict(R_=-1), dict(R_=(1 << 30) + 1), dict(S_=0), dict(S_=4097), dict(E_=-1),
               dict(E_=65), dict(X_=None), dict(nc=3), dict(nc=-2), dict(nc=0, v_=None), dict(xr=-1), dict(xs=-1), dict(xc=-1),
               dict(vs=-1), dict(E_=0, X_=None, surf=p(X)), dict(E_=0, X_=None, accum=p(X)), dict(E_=2, nc=0)):
        assert call(**kw) == -1, kw
        assert b"ray_maps" in lib.bn_last_error()
    assert call(R_=0) == 0
    torch.cuda.synchronize()
    assert (idx == -7).all() and (cnt == 0).all()
    assert call(nc=2) == 0
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), M.surf_idx(z.cpu().numpy(), d.cpu().numpy())) and int(cnt[5]) == R * S
    pts = torch.rand(5, 6, 3, dtype=torch.float64, device=DEV)
    out = torch.full((5, 6, 3), -7.0, device=DEV)
    v = torch.rand(5, 6, device=DEV)

    def pn(P=p(pts), H=5, W=6, rf=1, vi=None, o=p(out), vo=None):
        return lib.bn_point_normals(P, H, W, rf, vi, o, vo, None)

    for kw in (dict(P=None), dict(o=None), dict(H=0), dict(W=0), dict(H=-2), dict(H=1 << 16, W=1 << 15), dict(rf=2), dict(rf=-1), dict(vi=p(v)),
               dict(vo=p(v))):
        assert pn(**kw) == -1, kw
        assert b"point_normals" in lib.bn_last_error()
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert pn() == 0
    for kw, what in ((dict(z_vals=z.double()), "float32"), (dict(X=X, normal_col=3, view=view), "normal column"),
                     (dict(X=torch.rand(R, S, 65, device=DEV)), "channels"), (dict(depth=d.cpu()), "device")):
        args = dict(z_vals=z, weights=w, depth=d)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            Fn.ray_maps(**args)


# --------------------------------------------------------------------------------------------------------------- end to end
def view_case(kind):
    """The tiny models of the relight tests and the first 120 rays of their table as a 12 x 10 view."""
    if kind == "rpv_an":
        from test_gpu_relight import build, flags
        cfg, args, models, rays = build("rpv111")
        fl, cosi = flags("rpv111")
        fl = dict(fl, cos_irra_on=cosi)
    else:
        import relight_sample_cases as SC
        from test_gpu_relight_samples import build
        cfg, args, models, rays = build("microfacet")
        fl = SC.flags("microfacet")
    args.chunk = CHUNK
    return args, models, rays[:VIEW_H * VIEW_W].contiguous(), fl


@pytest.mark.parametrize("kind", ["rpv_an", "microfacet_multi"])
def test_view_maps_against_the_full_per_sample_dict(kind):
    """After the same seed: rgb and depth are bitwise render_image's; every map equals the statement applied to batched_inference's
    full per-sample dict; the maps taken from acc are bitwise the columns of render_surface's acc; cross_rows=6 returns exactly
    the slices of the dict; with a frame nr_from_depth is the statement on point_cloud's points."""
    from brdf_nerf_amd import point_cloud, render_surface, view_maps
    from brdf_nerf_amd.evaluate import batched_inference, render_image
    from test_gpu_dsm import frame
    args, models, rays, fl = view_case(kind)
    H, W = VIEW_H, VIEW_W
    seed = 23
    torch.manual_seed(seed)
    got = view_maps(models, args, rays, H, W, frame=frame(), chunk=CHUNK, cross_rows=6, **fl)
    maps, stats = got["maps"], got["stats"]
    torch.manual_seed(seed)
    img = render_image(models, args, rays, chunk=CHUNK, **fl)
    assert torch.equal(maps["rgb"], img["rgb"]) and torch.equal(maps["depth"], img["depth"])
    torch.manual_seed(seed)
    full = {k[:-len("_coarse")]: v for k, v in batched_inference(models, rays, None, args, **fl).items()}
    multi = kind == "microfacet_multi"
    torch.manual_seed(seed)
    surface = render_surface(models, args, rays, chunk=CHUNK, per_sample=multi, apply_brdf=fl["apply_brdf"], apply_theta=fl["apply_theta"])
    npy = lambda t: t.detach().cpu().numpy()
    z, w, depth = npy(full["z_vals"]), npy(full["weights"]), npy(full["depth"])
    assert z.shape == (H * W, args.n_samples + args.guided_samples)
    nkey = "normal_lr" if multi else "normal_an"
    view = npy(full["rays_d"])[:, 0, :]
    want = M.ray_statement(z, w, depth, npy(full[nkey]), 0, view)
    assert np.array_equal(npy(maps["surf_idx"]), want["surf_idx"]) and same(npy(maps["depth_std"]), want["std"])
    row = "lr" if multi else "an"
    assert dict(zip(M.COUNTERS, (int(v) for v in got["counters"][row]))) == want["counters"]
    c = want["counters"]
    assert stats["depth_std"] == c["std_sum"] / (c["std_count"] * M.STD_FIX) and stats["depth_std_skipped"] == 0
    assert stats[f"bad_nr_{row}%"] == 100.0 * c["bad_nr"] / c["nr_total"]
    if multi:
        assert stats["bad_nr_an%"] is None and stats["nr_an0%"] is None
    else:
        assert stats["nr_an0%"] == 100.0 * c["nr0"] / c["nr_total"] and stats["bad_nr_lr%"] is None
    idx = want["surf_idx"]
    for key, src in (("sigma_s", "sigmas"), ("alpha_s", "alphas"), ("transparency_s", "transparency"), ("weight_s", "weights")):
        t = npy(full[src]).reshape(H * W, -1, 1)
        assert np.array_equal(M.bits(npy(maps[key])), M.bits(M.surf(t, idx))), key
    # the accumulated field channels are the compositing kernel's acc, bit for bit
    acc = surface.acc
    spec = surface.spec
    assert torch.equal(maps["albedo"], acc[:, 0:3]) and torch.equal(maps["albedo"].clamp(0.0, 1.0), full["albedo_accu"])
    c0 = spec.ch_normal_lr if multi else spec.ch_normal_an
    assert torch.equal(maps[nkey], acc[:, c0:c0 + 3])
    from brdf_nerf_amd.maps import _HEAD_KEYS
    checked = 0
    for (name, _, _), (c0, wdt) in zip(spec.heads[1:], spec.head_cols[1:]):
        if _HEAD_KEYS.get(name) in full:
            assert torch.equal(maps[_HEAD_KEYS[name]], acc[:, c0:c0 + wdt]), name
            checked += 1
    assert checked >= 1
    for key in ("nr_vw", "nr_sun"):
        assert torch.equal(maps[key], full[key][:, 0, :])
    if multi:
        # per-sample BRDF auxiliaries: sum_s w K_s in float64 and the surface sample, against the statement
        for key in ("brdf", "glossy", "f", "g", "d", "l_dot_n", "v_dot_n", "halfvec", "n_h"):
            K = npy(full[key])
            assert K.shape[:2] == z.shape, key
            assert same(npy(maps[key]), M.accum(w, K)), key
            assert np.array_equal(M.bits(npy(maps[key + "_s"])), M.bits(M.surf(K, idx))), key
        assert np.array_equal(M.bits(npy(maps["roughness_s"])), M.bits(M.surf(npy(full["roughness"]), idx)))
    else:
        assert "brdf_s" not in maps and "roughness_s" not in maps
    # the cross-section of image row 6
    a, b = 6 * W, 7 * W
    cross = got["cross"]
    for key, src in (("z_vals", full["z_vals"]), ("sigmas", full["sigmas"][..., 0]), ("alphas", full["alphas"]),
                     ("transparency", full["transparency"]), ("sort_idx", full["sort_idx"]), ("depth", full["depth"])):
        assert torch.equal(cross[key], src[a:b]), key
    assert same(npy(cross["std"]), want["std"][a:b])
    # with a frame
    pts = npy(point_cloud(rays, maps["depth"], frame())).reshape(H, W, 3)
    assert same(npy(maps["nr_from_depth"]), M.point_normals(pts, True).reshape(H * W, 3))
    assert maps["altitude"].shape == (H * W,) and maps["altitude"].dtype == torch.float32
    torch.manual_seed(seed)
    exact = view_maps(models, args, rays, H, W, frame=frame(), chunk=CHUNK, precision="exact", **fl)
    assert same(npy(exact["maps"]["nr_from_depth"]), M.point_normals(pts, False).reshape(H * W, 3)) and "cross" not in exact
    assert torch.equal(exact["maps"]["rgb"], maps["rgb"])


def test_two_rank_view_maps_match_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_maps_worker.py), each child under its own time limit and started once."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_maps_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=_free_port(), WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, worker], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=300)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append("TIMEOUT\n" + p.communicate()[0])
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert all("RESULT" in o and "ok" in o for o in outs), "\n".join(outs)
