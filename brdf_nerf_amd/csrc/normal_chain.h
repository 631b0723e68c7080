// The float64 per-cell chain of calc_normal_from_pts3d (sat_utils.py:16-50), shared by bn_grid_normals (metrics.hip) and
// bn_point_normals (view_maps.hip): l2_normalize with its float32-eps floor, the cross product over the coordinate axis, and the
// normal of a cell from the vectors to its south, north, east and west neighbours.  Every operation is rounded on its own: both
// files are built with fp contraction off and the pragma below covers the functions here wherever they are included.
#pragma once
#pragma clang fp contract(off)

namespace normal_chain {

constexpr double EPS32 = 1.1920928955078125e-07;      // 2^-23: torch.finfo(float32).eps, the floor of l2_normalize

struct V3 { double x, y, z; };

__device__ __forceinline__ V3 unit(V3 v) {
  // train_utils.l2_normalize: v / sqrt(max(sum(v^2), eps32)); a NaN norm stays NaN, as torch.maximum keeps it
  const double n = (v.x * v.x + v.y * v.y) + v.z * v.z;
  const double d = sqrt(n < EPS32 ? EPS32 : n);
  return {v.x / d, v.y / d, v.z / d};
}

__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// S, N, E, W: the (not yet normalised) vectors from the cell to its south (r + 1), north (r - 1), east (c + 1) and west (c - 1)
// neighbours -> n = N((((n1 + n2) + n3) + n4) / 4), n1 = N(E x N), n2 = N(W x S), n3 = N(N x W), n4 = N(S x E)
__device__ __forceinline__ V3 cell_normal(V3 south, V3 north, V3 east, V3 west) {
  const V3 S = unit(south), N = unit(north), E = unit(east), Wv = unit(west);
  const V3 n1 = unit(cross(E, N)), n2 = unit(cross(Wv, S)), n3 = unit(cross(N, Wv)), n4 = unit(cross(S, E));
  return unit({(((n1.x + n2.x) + n3.x) + n4.x) / 4.0, (((n1.y + n2.y) + n3.y) + n4.y) / 4.0,
               (((n1.z + n2.z) + n3.z) + n4.z) / 4.0});
}

}  // namespace normal_chain
