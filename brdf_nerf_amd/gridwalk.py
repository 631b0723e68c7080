"""The walk over the rows of a DSM grid that every grid-level caller shares: this process's band of rows (distributed.row_band),
the buffers a band is written into, and the way back - the bands gathered along the row axis in rank order, the counters merged
by an all-reduce.

The band semantics are part of a result: every bit of what grid_visibility, fill_holes, orthophoto and orthomosaic return depends
on the inputs alone, not on row bands or ranks.  With a group of more than one rank the bands must partition [0, H) in rank order
and every rank returns the single-process result; a band without a group (`alone`) leaves the other rows "unseen".  GridWalk is
the one spelling of that; the callers keep their own launches and say what unseen means for each output - NODATA, -1, NaN or 0
handed to buffer(), and for fill_holes the rows "as they came", which no constant states (it keeps its torch.where).
"""
import torch

from .distributed import allreduce_, gather_rows, row_band, shard_bounds, world_info


class GridWalk:
    """The rows [rows[0], rows[1]) of an H-row grid that this process works on under `group`: `rows` as given, else this rank's
    shard_bounds.  rank, world; alone: a band without a group.  `name` is the caller's, for the ValueErrors.  rank_world=(rank,
    world) states the place in a group instead of asking torch.distributed (bounds only)."""

    def __init__(self, name, H, rows=None, group=None, rank_world=None):
        self.name, self.H, self.group = name, int(H), group
        self.rank, self.world = world_info(group) if rank_world is None else rank_world
        self.rows = row_band(name, self.H, shard_bounds(self.H, self.rank, self.world) if rows is None else rows, group)
        self.alone = self.world == 1 and self.rows != (0, self.H)

    def buffer(self, shape, dtype, unseen, device):
        """An output the launches write this band of: `unseen` everywhere for a lone band, else uninitialised - a whole grid is
        written by this process, a band under a group is cut out by join()."""
        return torch.full(shape, unseen, dtype=dtype, device=device) if self.alone else torch.empty(shape, dtype=dtype, device=device)

    def join(self, t, row_axis=0):
        """This rank's band of `t`, whose axis `row_axis` has the H rows -> the rows of all ranks, gathered in rank order,
        contiguous; on one rank, t as it came.  ValueError where the ranks' bands do not add up to H rows."""
        if self.world == 1:
            return t
        band = t.narrow(row_axis, self.rows[0], self.rows[1] - self.rows[0]).movedim(row_axis, 0).contiguous()
        full = gather_rows(band, self.group)
        if full.shape[0] != self.H:
            raise ValueError(f"{self.name}: the ranks' bands cover {full.shape[0]} rows of {self.H}")
        return full.movedim(0, row_axis).contiguous()

    def merge(self, counts, op=None):
        """The ranks' counters merged in place by one all-reduce (op None: SUM); on one rank, counts as they came."""
        return allreduce_(counts, op, self.group)


__all__ = ["GridWalk"]
