// The hole filling of a DSM (eval.py:107-151: quickly_interpolate_nans_from_singlechannel_img, griddata(method='nearest'), the
// *_Grid.tif of save_dsm_grid) on the device: every NaN cell takes the bits of its nearest known cell.  On a raster that is an
// exact Euclidean distance transform with a feature map, and it needs integers only:
//
// bn_grid_nearest_col  per column, the row of the nearest known cell (ties to the smaller row): a lane per column, one sweep
//                      down (the last known row at or above) and one sweep up (the next known row below, and the choice).
// bn_grid_fill         per cell of rows [row0, row1), the minimum of (dx^2 + dy^2, row, column) over the columns' nearest rows.
//
// There is no float arithmetic in this file: a cell is read, tested and written as 32 bits, so -0.0, denormals and infinities
// keep their bits and no contraction flag matters.  counts are an integer add and an integer max: the results' bits do not
// depend on the block order or on how the rows are split over launches or devices.
//
// bn_grid_fill, the mapping.  One block of 256 lanes owns one output row and stages that row of near_row into LDS once (4 W
// bytes, 32 KB at W = 8192).  Its lanes take the row's cells in strides of 256.  A lane starts from its own column's nearest row
// and walks outwards, columns i - k and i + k at step k, until k^2 > best d2: the comparison is STRICT, because at k^2 == best a
// known cell of the lane's own row (dy = 0, d2 = k^2) still ties with, and by its smaller (row, column) may beat, the best so far.
// LDS banks: at step k the 32 lanes of a ds_read_b32 group read words i - k of 32 consecutive i: 32 distinct banks, at every k.
// The scan is bounded by the distance to the nearest known cell: a dense DSM with holes of a few cells costs a few LDS reads
// per cell, a grid with a single known cell W reads per cell.
// BN_FILL_NO_LDS (A/B builds only, profiles/fill_throughput.py): the lanes read near_row through L2 instead of staging it.
#include "common.h"
#include "brdfnerf_hip.h"

namespace {

constexpr int COL_BLOCK = 64;
constexpr int ROW_BLOCK = 256;
constexpr int NO_SOURCE = 0x7fffffff;

__device__ __forceinline__ bool is_hole(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }   // NaN, any payload

__global__ __launch_bounds__(COL_BLOCK)
void nearest_col_kernel(const uint32_t *__restrict__ src, int H, int W, int *__restrict__ near_row) {
  const int i = (int)blockIdx.x * COL_BLOCK + (int)threadIdx.x;
  if (i >= W) return;
  int last = -1;                               // down: the last known row at or above j
#pragma unroll 8
  for (int j = 0; j < H; ++j) {
    const int64_t at = (int64_t)j * W + i;
    if (!is_hole(src[at])) last = j;
    near_row[at] = last;
  }
  int next = -1;                               // up: the next known row below j
  for (int j = H - 1; j >= 0; --j) {
    const int64_t at = (int64_t)j * W + i;
    const int above = near_row[at];
    if (above == j) {                          // a known cell is its own nearest
      next = j;
      continue;
    }
    // (|j - j'|, j') minimal: the row above wins a tie
    if (next >= 0 && (above < 0 || next - j < j - above)) near_row[at] = next;
  }
}

__global__ __launch_bounds__(ROW_BLOCK)
void fill_row_kernel(const uint32_t *__restrict__ src, const int *__restrict__ near_row, int W, int row0, uint32_t *__restrict__ dst,
                     int *__restrict__ source, int *__restrict__ dist2, unsigned long long *__restrict__ counts) {
  extern __shared__ int staged[];
  __shared__ int red[2 * ROW_BLOCK / 64];
  const int tid = (int)threadIdx.x, j = row0 + (int)blockIdx.x;
  const int *grow = near_row + (int64_t)j * W;
#ifdef BN_FILL_NO_LDS
  const int *nr = grow;
#else
  for (int i = tid; i < W; i += ROW_BLOCK) staged[i] = grow[i];
  __syncthreads();
  const int *nr = staged;
#endif
  int holes = 0, far = 0;
  for (int i = tid; i < W; i += ROW_BLOCK) {
    int br = nr[i], bc = i, best = NO_SOURCE;
    if (br >= 0) best = (j - br) * (j - br);
    if (best != 0) {
      holes += 1;
      for (int k = 1; i - k >= 0 || i + k < W; ++k) {
        const int k2 = k * k;
        if (k2 > best) break;                  // strict: see the head of the file
        for (int side = 0; side < 2; ++side) {
          const int c = side ? i + k : i - k;
          if (c < 0 || c >= W) continue;
          const int r = nr[c];
          if (r < 0) continue;
          const int d = k2 + (j - r) * (j - r);
          if (d < best || (d == best && (r < br || (r == br && c < bc)))) {
            best = d;
            br = r;
            bc = c;
          }
        }
      }
    }
    const int64_t at = (int64_t)j * W + i;
    const bool found = best != NO_SOURCE;      // false only on a grid without a known cell
    dst[at] = found ? src[(int64_t)br * W + bc] : src[at];
    if (source) source[at] = found ? br * W + bc : -1;
    if (dist2) dist2[at] = found ? best : -1;
    if (found && best > far) far = best;
  }
  if (!counts) return;
  for (int off = 32; off > 0; off >>= 1) {
    holes += __shfl_down(holes, off, 64);
    const int o = __shfl_down(far, off, 64);
    far = o > far ? o : far;
  }
  if ((tid & 63) == 0) {
    red[2 * (tid >> 6)] = holes;
    red[2 * (tid >> 6) + 1] = far;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < ROW_BLOCK / 64; ++w) {
      holes += red[2 * w];
      far = red[2 * w + 1] > far ? red[2 * w + 1] : far;
    }
    if (holes != 0) {
      atomicAdd(counts, (unsigned long long)holes);
      atomicMax(counts + 1, (unsigned long long)far);
    }
  }
}

}  // namespace

extern "C" int bn_grid_nearest_col(const float *src, int32_t H, int32_t W, int32_t *near_row, void *stream) {
  BN_REQUIRE(src && near_row, "grid_nearest_col: null argument");
  BN_REQUIRE(H >= 1 && W >= 1 && H <= BN_FILL_MAX_SIDE && W <= BN_FILL_MAX_SIDE, "grid_nearest_col: grid %d x %d (1 to %d a side)", H, W,
             BN_FILL_MAX_SIDE);
  nearest_col_kernel<<<(unsigned)((W + COL_BLOCK - 1) / COL_BLOCK), COL_BLOCK, 0, (hipStream_t)stream>>>(
      reinterpret_cast<const uint32_t *>(src), H, W, near_row);
  BN_LAUNCH_CHECK("grid_nearest_col");
  return 0;
}

extern "C" int bn_grid_fill(const float *src, const int32_t *near_row, int32_t H, int32_t W, int32_t row0, int32_t row1, float *dst,
                            int32_t *source, int32_t *dist2, long long *counts, void *stream) {
  BN_REQUIRE(src && near_row && dst, "grid_fill: null argument");
  BN_REQUIRE(H >= 1 && W >= 1 && H <= BN_FILL_MAX_SIDE && W <= BN_FILL_MAX_SIDE, "grid_fill: grid %d x %d (1 to %d a side)", H, W,
             BN_FILL_MAX_SIDE);
  BN_REQUIRE(0 <= row0 && row0 <= row1 && row1 <= H, "grid_fill: rows [%d, %d) outside [0, %d)", row0, row1, H);
  if (row0 == row1) return 0;
#ifdef BN_FILL_NO_LDS
  const size_t lds = 0;
#else
  const size_t lds = (size_t)W * sizeof(int);
#endif
  fill_row_kernel<<<(unsigned)(row1 - row0), ROW_BLOCK, lds, (hipStream_t)stream>>>(
      reinterpret_cast<const uint32_t *>(src), near_row, W, row0, reinterpret_cast<uint32_t *>(dst), source, dist2,
      reinterpret_cast<unsigned long long *>(counts));
  BN_LAUNCH_CHECK("grid_fill");
  return 0;
}
