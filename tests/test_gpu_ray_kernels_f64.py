"""The lean step's per-ray kernels (bn_composite_guided, bn_merged_composite_forward / _backward, bn_lambert_tail,
bn_normal_spv_reduce) against the float64 reference of tests/ray_kernel_cases.py, evaluated on the CPU from the same float32
inputs, at every lane layout of the case table.  Tolerances: ray_kernel_cases.TOL, fixed on the CPU from the reference alone
(tests/test_ray_kernels_cpu.py)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_kernel_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


def _dev(t, misaligned=False):
    """The tensor on the device; misaligned: its storage starts 4 bytes off a 16-byte boundary (a flat buffer sliced at 1)."""
    if t is None:
        return None
    if not misaligned:
        return t.to(DEV).contiguous()
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _src(c):
    m = c["cvar"] == "4m"
    return _dev(c["z_all"]), _dev(c["idx"]), _dev(c["out1"], m), _dev(c["out2"], m)


def _grad_bufs(c):
    m = c["cvar"] == "4m"
    d1 = _dev(torch.full((c["R"], c["S1"], c["C"]), float("nan")), m)
    d2 = _dev(torch.full((c["R"], c["S2"] - c["S1"], c["C"]), float("nan")), m) if c["out2"] is not None else None
    return d1, d2


def _check(tag, got, ref, c):
    e = K.compare(got, ref, c)
    print(tag, {q: f"{v:.1e}" for q, v in e.items()})
    for q, v in e.items():
        assert v <= K.TOL[q], f"{tag}: {q} error {v:.2e} > {K.TOL[q]:.0e}"
    return e


def _nreg_dev(Fn, c, nr):
    if nr is None:
        return None, None
    R = c["R"]
    rays = torch.zeros(R, 11, device=DEV)
    rays[:, 3:6] = c["rays_d"].to(DEV)
    spv_ray, spv_tot = torch.zeros(R, 2, device=DEV), torch.zeros(4, device=DEV)
    return Fn.normal_reg(rays[:, 3:6], nr["spv_an"], nr["spv_lr"], nr["lam_an"], nr["lam_lr"], nr["lam_spv"], spv_ray, spv_tot), spv_tot


WANT = ("alphas", "trans", "weights", "depth", "acc", "wsum", "var")


def _forward(Fn, c, src, nr=None, noise=None):
    nreg, spv_tot = _nreg_dev(Fn, c, nr)
    o = Fn.merged_composite_forward(*src, want=WANT, nreg=nreg, noise=noise)
    if nr is not None and nr["lam_spv"]:
        loss = torch.zeros(1, device=DEV)
        Fn.normal_spv_reduce(nreg, c["R"], c["S2"], ray_loss=loss)
        o["spv_ray"], o["spv_tot"], o["spv_loss"] = nreg._keep[1], spv_tot[:3].clone(), loss[0]
        assert float(spv_tot[3]) == 0.0
    return o, nreg


@pytest.mark.parametrize("name", list(K.CASES))
def test_merged_forward_and_reduce(name):
    from brdf_nerf_amd import functions as Fn
    c = K.CASES[name]
    nr = K.nreg_of(c, spv=True)
    got, _ = _forward(Fn, c, _src(c), nr)
    _check(name, got, K.forward_ref(*K.inputs(c, F64), nr), c)


@pytest.mark.parametrize("name", list(K.CASES))
def test_merged_backward_terms(name):
    from brdf_nerf_amd import functions as Fn
    c = K.CASES[name]
    src = _src(c)
    ref_in = K.inputs(c, F64)
    for term in K.TERMS:
        kw = K.backward_args(c, term, F64)
        if kw is None:
            continue
        nr = kw["nreg"]
        fwd, nreg = _forward(Fn, c, src, nr)
        d1, d2 = _grad_bufs(c)
        cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
        dv = lambda k: None if kw[k] is None else _dev(c[k])
        Fn.merged_composite_backward(*src, dv("d_w"), dv("d_depth"), dv("d_acc"), d1, d2, d_wsum=dv("d_wsum"), nonfinite=cnt,
                                     hs_scale=kw["hs_scale"], depth=fwd["depth"], nreg=nreg)
        q = K.grad_key(term)
        _check(f"{name}/{term}", {q: (d1, d2)}, {q: K.backward_ref(*ref_in, **kw)}, c)
        assert cnt.tolist() == [0, 0]


@pytest.mark.parametrize("name", [n for n, c in K.CASES.items() if "moderate" in c["patterns"] and c["S2"] >= 3])
def test_merged_backward_counts_nonfinite_like_the_reference(name):
    """One NaN and one Inf planted in d_weights of a ray whose densities are all positive (where sigma <= 0 torch's relu
    backward writes 0 whatever arrives, the kernel multiplies by d alpha / d sigma = 0: NaN; such rays carry no plant)."""
    from brdf_nerf_amd import functions as Fn
    c = K.CASES[name]
    r = c["patterns"].index("moderate")
    d_w = c["d_w"].clone()
    d_w[r, c["S2"] // 3] = float("nan")
    d_w[r, (2 * c["S2"]) // 3] = float("inf")
    g = K.backward_ref(*K.inputs(c, F64), d_w=d_w.double(), d_depth=c["d_depth"].double(), d_acc=c["d_acc"].double())
    flat = torch.cat([t.reshape(-1) for t in g if t is not None])
    want = [int(torch.isnan(flat).sum()), int(torch.isinf(flat).sum())]
    assert want[0] > 0 and want[1] > 0
    d1, d2 = _grad_bufs(c)
    cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    Fn.merged_composite_backward(*_src(c), _dev(d_w), _dev(c["d_depth"]), _dev(c["d_acc"]), d1, d2, nonfinite=cnt)
    assert cnt.tolist() == want
    assert bool(torch.isfinite(d1).all()) and (d2 is None or bool(torch.isfinite(d2).all()))


def _tail(Fn, c, src, cfg, noise=None):
    R = c["R"]
    d1, d2 = _grad_bufs(c)
    o = dict(ray_loss=torch.empty(R, device=DEV), loss_acc=torch.zeros(16, device=DEV), rgb=torch.empty(R, 3, device=DEV),
             weights=torch.empty(R, c["S2"], device=DEV), depth=torch.empty(R, device=DEV))
    kw = {}
    if cfg["prior"]:
        depths, tstd, valid = _dev(c["depths"]), _dev(c["tstd"]), _dev(c["valid"])
        kw = dict(valid_depth=valid, target_depth=depths[:, 0], target_weight=depths[:, 1], target_std=tstd, lambda_ds=K.LAMBDA_DS,
                  usealldepth=cfg.get("usealldepth", False))
    Fn.lambert_tail(*src, _dev(c["rgbs"]), K.PAD, K.LAMBDA_RGB, d1, d2, noise=noise, **o, **kw)
    o["grad_tail"] = (d1, d2)
    return o


@pytest.mark.parametrize("name", list(K.CASES))
def test_lambert_tail(name):
    from brdf_nerf_amd import functions as Fn
    c = K.CASES[name]
    src = _src(c)
    z, idx, o1, o2 = K.inputs(c, F64)
    for cname, cfg in K.TAIL_CONFIGS.items():
        want = K.tail_ref(z, idx, o1, o2, c["rgbs"].double(), K.PAD, K.LAMBDA_RGB, K.prior_of(c, F64) if cfg["prior"] else None,
                          K.LAMBDA_DS if cfg["prior"] else 0.0, cfg.get("usealldepth", False))
        _check(f"{name}/{cname}", _tail(Fn, c, src, cfg), want, c)


@pytest.mark.parametrize("S2", sorted(K.ALIGN_PAIRS))
def test_c4_on_misaligned_blocks_gives_the_aligned_numbers(S2):
    """C = 4 with every block 4 bytes off alignment takes the generic branch: the same operations in the same order, so the
    same bits as the float4 branch."""
    from brdf_nerf_amd import functions as Fn
    c = K.ALIGN_PAIRS[S2]
    res = []
    for cvar in ("4a", "4m"):
        cc = dict(c, cvar=cvar)
        src = _src(cc)
        f, _ = _forward(Fn, cc, src)
        t = _tail(Fn, cc, src, K.TAIL_CONFIGS["alldepth"])
        d1, d2 = _grad_bufs(cc)
        Fn.merged_composite_backward(*src, _dev(c["d_w"]), _dev(c["d_depth"]), _dev(c["d_acc"]), d1, d2, d_wsum=_dev(c["d_wsum"]),
                                     hs_scale=K.HS, depth=f["depth"])
        res.append([f[k] for k in WANT] + [t["rgb"], t["ray_loss"], *[g for g in t["grad_tail"] if g is not None], d1] + ([d2] if d2 is not None else []))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    _check(f"align{S2}", dict(zip(WANT, res[1][:len(WANT)])), K.forward_ref(*K.inputs(c, F64)), c)


def test_identity_index_without_a_second_block_is_admitted():
    """S1 = S2 with an explicit identity sort index and out2 = None passes merged_check and reads out1 alone (every
    `identity` case of the table runs that way; here: the same bits as idx = None)."""
    from brdf_nerf_amd import functions as Fn
    c = next(v for v in K.CASES.values() if v["split"] == "identity" and v["S2"] == 449)
    z, idx, o1, _ = _src(c)
    a = Fn.merged_composite_forward(z, idx, o1, None, want=WANT)
    b = Fn.merged_composite_forward(z, None, o1, None, want=WANT)
    assert all(torch.equal(a[k], b[k]) for k in WANT)


@pytest.mark.parametrize("R", K.REDUCE_R)
def test_normal_spv_reduce_alone(R):
    from brdf_nerf_amd import functions as Fn
    sr = K.reduce_case(R)
    spv_ray, spv_tot = sr.to(DEV), torch.zeros(4, device=DEV)
    nreg = Fn.normal_reg(None, 4, 7, 0.0, 0.0, K.LAM_SPV, spv_ray, spv_tot)
    loss, part = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    Fn.normal_spv_reduce(nreg, R, 2, ray_loss=loss, loss_acc=part)
    want = K.spv_tot_ref(sr.double(), R, 2, K.LAM_SPV)
    for i in range(3):
        e = K.err_rays(spv_tot[i], want[i])
        print(f"reduce R={R} tot[{i}] {e:.1e}")
        assert e <= K.TOL["spv_tot"]
    assert K.err_rays(loss[0], want[2]) <= K.TOL["spv_loss"] and K.err_rays(part[0], want[2]) <= K.TOL["spv_loss"]


# ------------------------------------------------------------------------------------------------ noise
NOISE_CASES = [n for n, c in K.CASES.items() if c["S2"] in (65, 449) and c["R"] > 1][::3]


@pytest.mark.parametrize("ray_offset", [0, 7])
@pytest.mark.parametrize("name", NOISE_CASES)
def test_in_kernel_noise_on_the_merged_kernels(name, ray_offset):
    """noise_arg draws are Philox normals indexed (ray + ray_offset) * S2 + sorted position: the same draws as an array
    (bn_rng_normal) feed the float64 reference.  Launch-argument and step-state forms of noise_std."""
    from brdf_nerf_amd import functions as Fn, _lib as L
    c = K.CASES[name]
    R, S2 = c["R"], c["S2"]
    st = Fn.new_step_state(DEV, 99, 5e-4)
    stream = L.BN_RNG_NOISE_MERGED
    draws = Fn.rng_normal(st, stream, (R + ray_offset) * S2).view(R + ray_offset, S2)[ray_offset:].cpu().double()
    std = float(torch.tensor(K.NOISE_STD, dtype=torch.float32))           # what the kernels multiply by
    src = _src(c)
    z, idx, o1, o2 = K.inputs(c, F64)
    nr = K.nreg_of(c, spv=True)
    kw = K.backward_args(c, "all", F64)
    cfg = K.TAIL_CONFIGS["alldepth"]
    Fn.set_state_noise(st, K.NOISE_STD)
    for from_state in (False, True):
        noise = Fn.noise_arg(st, K.NOISE_STD, stream, ray_offset, from_state=from_state)
        tag = f"{name}/off{ray_offset}/{'state' if from_state else 'arg'}"
        fwd, nreg = _forward(Fn, c, src, nr, noise)
        _check(tag + "/fwd", fwd, K.forward_ref(z, idx, o1, o2, nr, draws, std), c)
        want = K.tail_ref(z, idx, o1, o2, c["rgbs"].double(), K.PAD, K.LAMBDA_RGB, K.prior_of(c, F64), K.LAMBDA_DS, True, draws, std)
        _check(tag + "/tail", _tail(Fn, c, src, cfg, noise), want, c)
        d1, d2 = _grad_bufs(c)
        Fn.merged_composite_backward(*src, _dev(c["d_w"]), _dev(c["d_depth"]), _dev(c["d_acc"]), d1, d2, d_wsum=_dev(c["d_wsum"]),
                                     hs_scale=K.HS, depth=fwd["depth"], nreg=nreg, noise=noise)
        _check(tag + "/bwd", {"grad_bwd": (d1, d2)}, {"grad_bwd": K.backward_ref(z, idx, o1, o2, noise=draws, noise_std=std, **kw)}, c)


# ------------------------------------------------------------------------------------------------ bn_composite_guided
def _guided(Fn, c, u=None, u_t=None, state=None, ray_offset=0, noise=None, table=False):
    R, S, G = c["R"], c["S"], c["G"]
    z = _dev(c["z"])
    if table:                                           # sigma = channel 3 of a [R][S][7] pass-1 output
        out1 = torch.rand(R, S, 7, device=DEV)
        out1[..., 3] = _dev(c["sigma"])
        sig = dict(out1=out1)
    else:
        sig = dict(out1=None, sigma=_dev(c["sigma"]))
    kw = {}
    if c["prior"]:
        depths, tstd = _dev(c["depths"]), _dev(c["tstd"])
        valid2 = torch.stack([_dev(c["valid"]), torch.zeros(R, device=DEV)], -1).contiguous()
        kw = dict(use_target=valid2[:, 0], target_depth=depths[:, 0], target_std=tstd[:, 0])          # strided views of [R][2] tables
    nf = torch.tensor([0.0, K.FAR], device=DEV)
    z2, z_all, idx, w1, d1 = Fn.composite_guided(z, sig["out1"], G, nf, 3.0, u=u, u_target=u_t if c["prior"] else None, state=state,
                                                 want_pass1=True, ray_offset=ray_offset, sigma=sig.get("sigma"), noise=noise, **kw)
    return {"weights": w1, "depth": d1, "z2": z2, "z_all": z_all, "idx": idx}


def _check_guided(tag, got, ref, c):
    R, S, G = c["R"], c["S"], c["G"]
    _check(tag, {k: v for k, v in got.items() if k != "idx"}, ref, c)
    z_all, idx = got["z_all"], got["idx"]
    assert bool((z_all[:, 1:] >= z_all[:, :-1]).all()), tag
    assert torch.equal(torch.sort(idx, -1)[0].cpu(), torch.arange(S + G).expand(R, -1)), tag
    assert torch.equal(torch.gather(torch.cat([_dev(c["z"]), got["z2"]], -1), 1, idx), z_all), tag
    mism, share = K.idx_mismatches(idx, ref, 4 * K.TOL["z2"])
    print(tag, "idx: near-tie share", f"{share:.3f}")
    assert mism == 0, f"{tag}: {mism} sort indices differ away from near-ties"


@pytest.mark.parametrize("name", list(K.GUIDED_CASES))
def test_composite_guided(name):
    from brdf_nerf_amd import functions as Fn, _lib as L
    c = K.GUIDED_CASES[name]
    R, G = c["R"], c["G"]
    # draws handed over as arrays
    _check_guided(name + "/arrays", _guided(Fn, c, u=_dev(c["u"]), u_t=_dev(c["u_t"]), table=True), K.guided_reference(c, F64), c)
    # in-kernel draws, with and without a ray offset
    st = Fn.new_step_state(DEV, 31, 5e-4)
    for off in (0, 7):
        u = Fn.rng_uniform(st, L.BN_RNG_GUIDED, (R + off) * G).view(R + off, G)[off:].cpu()
        u_t = Fn.rng_uniform(st, L.BN_RNG_GUIDED_TARGET, (R + off) * G).view(R + off, G)[off:].cpu()
        _check_guided(f"{name}/rng{off}", _guided(Fn, c, state=st, ray_offset=off), K.guided_reference(c, F64, u=u, u_t=u_t), c)


@pytest.mark.parametrize("ray_offset", [0, 7])
@pytest.mark.parametrize("name", [n for n, c in K.GUIDED_CASES.items() if c["S"] in (65, 449)])
def test_composite_guided_with_noise(name, ray_offset):
    from brdf_nerf_amd import functions as Fn, _lib as L
    c = K.GUIDED_CASES[name]
    R, S = c["R"], c["S"]
    st = Fn.new_step_state(DEV, 57, 5e-4)
    stream = L.BN_RNG_NOISE_COARSE
    draws = Fn.rng_normal(st, stream, (R + ray_offset) * S).view(R + ray_offset, S)[ray_offset:].cpu()
    Fn.set_state_noise(st, K.NOISE_STD)
    ref = K.guided_reference(c, F64, noise=draws)
    for from_state in (False, True):
        noise = Fn.noise_arg(st, K.NOISE_STD, stream, ray_offset, from_state=from_state)
        got = _guided(Fn, c, u=_dev(c["u"]), u_t=_dev(c["u_t"]), noise=noise)
        _check_guided(f"{name}/noise{ray_offset}/{'state' if from_state else 'arg'}", got, ref, c)
