"""Worker of test_two_rank_relight_matches_one_rank (tests/test_gpu_relight.py): rank r of 2, both on cuda:0, gloo.

Each rank renders the surface of its contiguous share of the rays inside relight_image (shard_bounds) and the rows are
all-gathered; the result must equal, bitwise, what the same process computes alone for all rays.  The evaluation draws
(perturb = 1) are served from full-view tensors seeded on the host, each call taking the rows it renders, so both runs see the
same numbers.
"""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class RowDraws:
    """torch.rand / rand_like / randn of the render_rays calls over the row spans [(lo, hi), ...]: the reference's draw order per
    call (rand_like (R,S), randn (R,S), rand (R,G), randn (R,S+G)) served from full-view tensors."""

    def __init__(self, full, spans, dev):
        self.feed = [t[lo:hi].to(dev) for lo, hi in spans for t in full]

    def __enter__(self):
        self._o = (torch.rand, torch.rand_like, torch.randn)

        def nxt(shape):
            t = self.feed.pop(0)
            assert tuple(t.shape) == tuple(shape), (tuple(t.shape), tuple(shape))
            return t

        def rand(*size, **kw):
            size = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
            return nxt(size)

        torch.rand = torch.randn = rand
        torch.rand_like = lambda x, **kw: nxt(x.shape)
        return self

    def __exit__(self, *a):
        torch.rand, torch.rand_like, torch.randn = self._o
        assert a[0] is not None or not self.feed


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import relight_cases as RC
    from test_gpu_parity import make_args
    from brdf_nerf_amd import load_model, relight_image
    from brdf_nerf_amd.distributed import shard_bounds
    from brdf_nerf_amd.raytable import synthetic_table

    name = "rpv111"
    fl = RC.CASES[name][1]
    cfg = RC.config(name)
    args = make_args(cfg, "fp32")
    model = load_model(args)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in cfg.make_params(RC.MODEL_SEED).items()})
    models = {"coarse": model.to(dev)}
    R, S, G = 257, cfg.n_samples, cfg.guided_samples          # odd: the two shares differ in size
    rays = synthetic_table(R, device=dev, seed=RC.RAYS_SEED).data["rays"]
    g = torch.Generator().manual_seed(23)
    full = [torch.rand(R, S, generator=g), torch.randn(R, S, generator=g), torch.rand(R, G, generator=g), torch.randn(R, S + G, generator=g)]
    suns = RC.sun_directions().to(dev)
    kw = dict(apply_brdf=fl["apply_brdf"], cos_irra_on=fl["cos_irra_on"], return_surface=True)

    lo, hi = shard_bounds(R, rank, world)
    with RowDraws(full, [(lo, hi)], dev):
        two = relight_image(models, args, rays, suns, **kw)            # data parallel: the default group
    # the single-rank result, computed by this process alone: a group of one rank
    groups = [dist.new_group([r]) for r in range(world)]           # (every rank must take part in every new_group call)
    # render_rays clamps the guided samples to the (near, far) of the FIRST ray of each call (rendering.py:133,144, kept as upstream),
    # so a view is a function of its chunk boundaries: the one-rank run is chunked where the two ranks split
    cut = shard_bounds(R, 0, world)[1]
    with RowDraws(full, [(0, cut), (cut, R)], dev):
        one = relight_image(models, args, rays, suns, group=groups[rank], chunk=cut, **kw)
    ok = tuple(two["rgb"].shape) == (suns.shape[0], R, 3) and torch.equal(two["rgb"], one["rgb"]) and \
        torch.equal(two["depth"], one["depth"]) and torch.equal(two["surface"].acc, one["surface"].acc) and \
        torch.equal(two["surface"].wsum, one["surface"].wsum)
    print(f"RESULT rank {rank}: rays {lo}:{hi} of {R}, rgb max |two - one| = {float((two['rgb'] - one['rgb']).abs().max()):.3e} -> "
          f"{'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
