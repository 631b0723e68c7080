"""NormalLoss against the tie-point normals (--nr_spv_type 2 / 3) through the training step, the ray table and the loop: the
launch-lean step (bn_normal_target_loss between the shading and the backward compositing; eager, then replayed from its HIP
graph) against the general step's torch statement, as test_gpu_lean.py's test_lean_step_with_normal_loss_matches_general_step
does for type 1 and within that test's bounds; the ways the term is off, bit for bit; ray_table(want_normals=True); TrainLoop."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle.config import FieldConfig  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R, S, G = 96, 16, 16
LAM = 0.5


def _batch(seed):
    from test_gpu_lean import _sat_rays
    g = torch.Generator().manual_seed(seed)
    rays = _sat_rays(R, g).to(DEV)
    rgbs = torch.rand(R, 3, generator=g).to(DEV)
    valid = (torch.rand(R, generator=g) < 0.6).float().to(DEV)
    depths = torch.stack([0.8 + 0.4 * torch.rand(R, generator=g), torch.rand(R, generator=g)], -1).to(DEV)
    dstd = (0.03 * torch.rand(R, generator=g)).to(DEV)
    n = torch.cat([0.4 * torch.randn(R, 2, generator=g), torch.ones(R, 1)], -1)
    normals = (n / n.norm(dim=-1, keepdim=True)).to(DEV)
    vn = (torch.rand(R, generator=g) < 0.7).float().to(DEV)
    assert ((valid > 0) & (vn == 0)).sum() >= 5 and ((valid == 0) & (vn == 1)).sum() >= 5
    return rays, rgbs, dict(valid_depth=valid, depths=depths, depth_std=dstd), dict(normals=normals, valid_normal=vn)


def _new_normals(seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.cat([0.8 * torch.randn(R, 2, generator=g), torch.ones(R, 1)], -1)
    return (n / n.norm(dim=-1, keepdim=True)).to(DEV)


CASES = {
    "an3": (dict(funcM=1, funcF=1, funcH=1, normal="analystic"), 3, False, False),
    "an3_reg_gsam": (dict(funcM=1, funcF=1, funcH=1, normal="analystic"), 3, True, True),
    "anlr3_reg": (dict(funcM=1, funcF=1, funcH=1, normal="analystic_learned"), 3, True, False),
    "anlr3_gsam": (dict(funcM=1, funcF=1, funcH=1, normal="analystic_learned"), 3, False, True),
    "lr2": (dict(funcM=1, funcF=1, funcH=1, normal="learned"), 2, False, False),
    "lr2_reg_gsam": (dict(funcM=1, funcF=1, funcH=1, normal="learned"), 2, True, True),
    "multibrdf_microfacet": (dict(roughness=True, normal="analystic", MultiBRDF=True), 3, False, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_lean_step_with_target_normals_matches_general_step(name):
    """with_reg: together with the hard-surface and normal regularisers and DepthLoss (ds_lambda 10), otherwise alone (ds_lambda 0).
    Loss within 2e-5 relative, flat gradient within 5e-4 of its largest entry, over 4 steps; then: the staged normals changed in
    place are followed by the replayed graph; depth_loss_on=False leaves the term on; lambda 0 gives another loss."""
    import brdf_nerf_amd
    from test_gpu_parity import build_model, make_args, Replay, diag
    from brdf_nerf_amd import functions as Fn
    from brdf_nerf_amd.trainer import FusedTrainer
    kw, typ, with_reg, gsam = CASES[name]
    cfg = FieldConfig(feat=64, n_samples=16, guided_samples=16, **kw)
    args = make_args(cfg, "fp32")
    rays, rgbs, prior, tgt = _batch(7)
    flags = dict(apply_brdf=True, apply_theta=True, cos_irra_on=True, gsam_only=gsam)
    lam = dict(nr_spv_lambda=LAM, nr_spv_type=typ, ds_lambda=10.0 if with_reg else 0.0,
               **(dict(hs_lambda=0.1, nr_reg_an_lambda=0.2, nr_reg_lr_lambda=0.1) if with_reg else {}))
    prev = brdf_nerf_amd.set_deterministic(True)
    try:
        torch.manual_seed(17)
        ma, mb = build_model(cfg, 29, "fp32"), build_model(cfg, 29, "fp32")
        ta = FusedTrainer(ma, args, lr=5e-4, strict_rng=False, **lam)
        tb = FusedTrainer(mb, args, lr=5e-4, strict_rng=False, **lam)
        ta.lean = False
        tb.graph_after = 1
        tb.keep_grads = True
        worst = [0.0]

        def both(what, **over):
            tb.flat_param.copy_(ta.flat_param)
            tb.exp_avg.copy_(ta.exp_avg)
            tb.exp_avg_sq.copy_(ta.exp_avg_sq)
            draws = [Fn.rng_uniform(tb.state, 1, R * S).view(R, S), Fn.rng_uniform(tb.state, 2, R * G).view(R, G),
                     Fn.rng_uniform(tb.state, 3, R * G).view(R, G)]
            kw_step = dict(flags, **prior, **tgt, **over)
            with Replay(draws) as rp:
                la, _ = ta.step(rays, rgbs, **kw_step)
                assert rp.draws == []
            lb, _ = tb.step(rays, rgbs, **kw_step)
            la, lb = float(la), float(lb)
            assert abs(la - lb) <= 2e-5 * abs(la) + 1e-7, (name, what, la, lb)
            ga, gb = ta.flat_grad, tb.flat_grad
            e = float((ga - gb).abs().max()) / float(ga.abs().max())
            worst[0] = max(worst[0], e)
            assert e <= 5e-4, (name, what, e)
            return lb

        for step in range(4):
            lb = both(step)
        assert len(tb._graphs) == 1, "the lean step was not captured into a HIP graph"
        assert any(k[0] == "nt_count" for k in tb._bufs), "the step did not run bn_normal_target_loss"
        if cfg.MultiBRDF:
            assert any(k[0] == "B_full" for k in tb._bufs), "a MultiBRDF step with the term takes the full-width copy"
        # new contents at the staged address: the replayed graph (and the general step) follow them
        tgt["normals"].copy_(_new_normals(99))
        l_new = both("new normals")
        assert len(tb._graphs) == 1 and abs(l_new - lb) > 1e-4 * abs(lb)
        # the depth stage does not switch the term off (upstream adds it whatever ds_drop says) ...
        l_nd = both("depth_loss_on=False", depth_loss_on=False)
        # ... and lambda 0 gives another loss, in both depth stages
        tb.reg["nr_spv"] = 0.0
        l0, _ = tb.step(rays, rgbs, **dict(flags, **prior, **tgt))
        l0_nd, _ = tb.step(rays, rgbs, **dict(flags, **prior, **tgt), depth_loss_on=False)
        tb.reg["nr_spv"] = LAM
        assert abs(float(l0) - l_new) > 1e-4 * abs(l_new) and abs(float(l0_nd) - l_nd) > 1e-4 * abs(l_nd)
        diag(f"lean step with NormalLoss against target normals {name}: worst flat-gradient difference {worst[0]:.2e} of the largest entry")
    finally:
        brdf_nerf_amd.set_deterministic(prev)


@pytest.mark.parametrize("normal,typ", [("analystic", 3), ("learned", 2)])
def test_term_off_is_bitwise_the_step_without_it(normal, typ):
    """Lambda 0, normals=None and a batch with no valid row: loss, rgb and parameters over three steps (eager, captured, replayed)
    are bit for bit those of a trainer built without the new arguments; with the term on they are not."""
    import brdf_nerf_amd
    from test_gpu_parity import build_model, make_args
    from brdf_nerf_amd.trainer import FusedTrainer
    cfg = FieldConfig(feat=64, n_samples=16, guided_samples=16, funcM=1, funcF=1, funcH=1, normal=normal)
    args = make_args(cfg, "fp32")
    rays, rgbs, prior, tgt = _batch(11)
    none_valid = dict(prior, valid_depth=torch.zeros_like(prior["valid_depth"]))
    flags = dict(apply_brdf=True, apply_theta=True, cos_irra_on=True)

    def run(ctor, step_kw, pr):
        torch.manual_seed(31)
        tr = FusedTrainer(build_model(cfg, 41, "fp32"), args, lr=5e-4, ds_lambda=10.0, strict_rng=False, hs_lambda=0.1, **ctor)
        tr.graph_after = 1
        out = []
        for _ in range(3):
            loss, rgb = tr.step(rays, rgbs, **flags, **pr, **step_kw)
            out.append((loss.clone(), rgb.clone(), tr.flat_param.clone()))
        assert len(tr._graphs) == 1
        return out

    def same(a, b):
        return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for sa, sb in zip(a, b) for x, y in zip(sa, sb))

    prev = brdf_nerf_amd.set_deterministic(True)
    try:
        today = run({}, {}, prior)
        assert same(today, run({}, {}, prior)), "the step does not repeat: nothing can be compared bit for bit"
        on = dict(nr_spv_lambda=LAM, nr_spv_type=typ)
        assert same(today, run(dict(nr_spv_lambda=0.0, nr_spv_type=typ), tgt, prior))
        assert same(today, run(on, {}, prior))
        assert same(today, run(on, dict(tgt, normals=None), prior))
        assert same(today, run(on, dict(tgt, valid_normal=None), prior))
        with_term = run(on, tgt, prior)
        assert not same(today, with_term) and same(with_term, run(on, tgt, prior))
        assert same(run({}, {}, none_valid), run(on, tgt, none_valid))
    finally:
        brdf_nerf_amd.set_deterministic(prev)


def test_a_type_without_its_normal_field_is_refused_at_construction():
    from test_gpu_parity import build_model, make_args
    from brdf_nerf_amd.trainer import FusedTrainer
    for normal, typ in (("learned", 3), ("analystic", 2), ("none", 3)):
        cfg = FieldConfig(feat=64, n_samples=16, guided_samples=16, funcM=1, funcF=1, funcH=1, normal=normal)
        with pytest.raises(ValueError, match="nr_spv_type"):
            FusedTrainer(build_model(cfg, 3, "fp32"), make_args(cfg, "fp32"), nr_spv_lambda=0.1, nr_spv_type=typ)
    with pytest.raises(ValueError, match="nr_spv_type"):
        FusedTrainer(build_model(cfg, 3, "fp32"), make_args(cfg, "fp32"), nr_spv_type=4)


def test_ray_table_with_normals():
    """Two views of the 33 x 65 z17 fixture, the second without priors: the new columns are depth_priors' per-view results and the
    padding (0, 0, 1) / 0; every other column is bitwise the table's without them."""
    import camera_cases as M
    import priors_cases as P
    from test_gpu_priors import rpc_of, scene, tie_data
    from brdf_nerf_amd.camera import depth_priors, ray_table
    H, W = 33, 65
    sc = scene("z17", 11, H, W)
    view = {"rpc": sc["d"], "H": H, "W": W, "min_alt": sc["lo"], "max_alt": sc["hi"], "sun": M.SUN}
    px = P.hard_ties(H, W, 257, 21)
    pts, cor = tie_data(sc, px, 5)
    images = [torch.rand(H * W, 3), torch.rand(H * W, 3)]
    pri = {"pts2d": px, "pts3d": pts, "correl": cor}
    kw = dict(zone=17, device=DEV, priors=[pri, None])
    table = ray_table([view, view], images, sc["center"], sc["rng"], want_normals=True, **kw)
    plain = ray_table([view, view], images, sc["center"], sc["rng"], **kw)
    assert set(table.data) == set(plain.data) | {"normals", "valid_normal"}
    for k in plain.data:
        assert torch.equal(table.data[k].view(torch.int32), plain.data[k].view(torch.int32)), k
    one = depth_priors(rpc_of(sc["d"]), H, W, px, pts, cor, sc["lo"], sc["hi"], sc["center"], sc["rng"], zone=17, margin=1e-4, device=DEV)
    n = H * W
    nrm, vn = table.data["normals"], table.data["valid_normal"]
    assert nrm.shape == (2 * n, 3) and vn.shape == (2 * n,) and nrm.dtype == vn.dtype == torch.float32
    assert torch.equal(nrm[:n].view(torch.int32), one["normals"].float().view(torch.int32)) and torch.equal(vn[:n], one["valid_normal"].float())
    assert vn[:n].sum().item() > 0
    assert torch.equal(nrm[n:], torch.tensor([0.0, 0.0, 1.0], device=DEV).expand(n, 3)) and not vn[n:].any()
    with pytest.raises(ValueError, match="want_normals"):
        ray_table([view, view], images, sc["center"], sc["rng"], zone=17, device=DEV, want_normals=True)


def test_train_loop_with_target_normals():
    """Three steps with --normal analystic, --nr_spv_type 0 (resolved to 3 as opt.py:328-334 does) and --nr_spv_lambda 0.1: finite
    losses that differ from the lambda-0 run; the same loop on a table without the columns names what is missing."""
    from test_gpu_parity import make_args, mini
    from brdf_nerf_amd.raytable import synthetic_table
    from brdf_nerf_amd.train import TrainLoop
    cfg = mini(funcM=1, funcF=1, funcH=1, normal="analystic")

    def losses_of(lam, with_normals=True):
        a = make_args(cfg)
        for k, v in dict(batch_size=64, lr=5e-4, max_train_steps=40, brdf_on=0.0, cos_irra_on=0.0, nrrg_on=0.0, ds_drop=0.5, ds_lambda=10.0,
                         gsam_only_on=1.0, nr_reg_lr_lambda=0.0, hs_lambda=0.0, in_ckpts="none", nr_spv_type=0, nr_spv_lambda=lam).items():
            setattr(a, k, v)
        torch.manual_seed(0)
        loop = TrainLoop(a, synthetic_table(640, device=DEV, seed=4, with_normals=with_normals), compute_dtype="fp32", near_far=(0.0, 2.0))
        assert loop.trainer.nr_spv_type == 3
        torch.manual_seed(1)
        return [float(loop.step()["loss"]) for _ in range(3)]

    on, off = losses_of(0.1), losses_of(0.0)
    assert np.isfinite(on).all() and np.isfinite(off).all()
    assert all(abs(a - b) > 1e-5 * abs(b) for a, b in zip(on, off)), (on, off)
    with pytest.raises(ValueError, match=r"'normals'.*want_normals=True"):
        losses_of(0.1, with_normals=False)
    assert np.isfinite(losses_of(0.0, with_normals=False)).all()
