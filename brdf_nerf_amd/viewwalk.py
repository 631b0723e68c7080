"""The walk over the rays of a view that every view-level caller shares: this rank's contiguous share (shard_bounds), cut into
chunks, and the way back - the per-chunk results joined along the ray axis and all-gathered in rank order.

The chunk boundaries are part of a result: render_rays clamps the guided samples to the (near, far) of the FIRST ray of each call
and consumes the draws per call, so two callers agree bit for bit only where they cut the rays at the same places.  ViewWalk is
the one spelling of those places; evaluate.render_image, dsm.dsm_image, relight, shadows and maps.view_maps keep their own
`for i, j in walk.chunks():` loop and per-chunk work, and hand the parts back here.
"""
import torch

from .distributed import gather_rows, shard_bounds, world_info


def check_out(out, shape):
    """A caller's `out` must be float32 of exactly the result's shape (None passes)."""
    if out is not None and (tuple(out.shape) != tuple(shape) or out.dtype != torch.float32):
        raise ValueError(f"out must be float32 {tuple(shape)}, got {out.dtype} {tuple(out.shape)}")


class ViewWalk:
    """n_rays rays in chunks of `chunk` under `group`: rank, world, this rank's rays [lo, hi).  Every (i, j) is an absolute ray
    range.  rank_world=(rank, world) states the place in a group instead of asking torch.distributed (bounds only)."""

    def __init__(self, n_rays, chunk, group=None, rank_world=None):
        self.n_rays, self.chunk, self.group = int(n_rays), int(chunk), group
        self.rank, self.world = world_info(group) if rank_world is None else rank_world
        self.lo, self.hi = shard_bounds(self.n_rays, self.rank, self.world)

    def _chunks_of(self, rank):
        lo, hi = shard_bounds(self.n_rays, rank, self.world)
        return [(i, min(hi, i + self.chunk)) for i in range(lo, hi, self.chunk)]

    def chunks(self):
        """This rank's (i, j) ranges: one render_rays-sized call each."""
        return self._chunks_of(self.rank)

    def all_chunks(self):
        """The ranges of every rank, in rank order: the calls the joined result was rendered by."""
        return [c for r in range(self.world) for c in self._chunks_of(r)]

    def join(self, parts, tail_shape, dtype=torch.float32, device=None):
        """This rank's per-chunk rows -> the rows of all rays: concatenated (a rank without a part brings zero rows of
        tail_shape), all-gathered along the ray axis in rank order, contiguous."""
        t = torch.cat(parts, 0) if parts else torch.zeros((0,) + tuple(tail_shape), dtype=dtype, device=device)
        return gather_rows(t, self.group).contiguous()

    def join_attrs(self, parts, table, device=None):
        """join() of each attribute of this rank's chunk objects: table of (attribute, trailing shape) -> {attribute: rows}."""
        return {k: self.join([getattr(c, k) for c in parts], tail, device=device) for k, tail in table}

    def planes(self, K, tail_shape, out=None, device=None):
        """A direction-major float32 result (K, n_rays) + tail_shape, optionally the caller's `out` -> Planes."""
        return Planes(self, K, tail_shape, out, device)


class Planes:
    """A direction-major result (K, R, ...) filled chunk by chunk: `mine` holds this rank's rays - the result itself on one rank
    (the caller's `out` when given), else a (K, hi - lo, ...) buffer that result() gathers along the ray axis."""

    def __init__(self, walk, K, tail_shape, out, device):
        shape = (K, walk.n_rays) + tuple(tail_shape)
        check_out(out, shape)
        self.walk, self.out = walk, out
        if walk.world == 1:
            self.mine = torch.empty(shape, dtype=torch.float32, device=device) if out is None else out
        else:
            self.mine = torch.empty((K, walk.hi - walk.lo) + tuple(tail_shape), dtype=torch.float32, device=device)

    def chunk(self, i, j):
        """The (K, j - i, ...) slice the rays [i, j) of this rank are shaded into."""
        return self.mine[:, i - self.walk.lo:j - self.walk.lo]

    def result(self):
        """The full (K, R, ...): `out` when one was given."""
        if self.walk.world == 1:
            return self.mine
        full = gather_rows(self.mine.transpose(0, 1).contiguous(), self.walk.group).transpose(0, 1)    # (R, K, ...) rows in rank order
        if self.out is None:
            return full.contiguous()
        self.out.copy_(full)
        return self.out


__all__ = ["ViewWalk", "Planes", "check_out"]
