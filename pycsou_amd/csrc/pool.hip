// Block pooling and unpooling of a C-order array of 1 to 3 dimensions (Pooling, pycsou/linop/sampling.py:394-536
// -> skimage.measure.block_reduce with cval = 0, and the np.repeat unpooling of Pooling.adjoint).
//
// Shapes are padded in front to three axes (n0, n1, n2) with blocks (B0, B1, B2); the pooled array has
// m_k = ceil(n_k / B_k) entries per axis.  A block at a ragged edge is summed over its real cells only, which
// is the zero padding of block_reduce; `scale` multiplies the sum (1 for 'sum', 1 / prod(block) for 'mean',
// which therefore divides by the full block size in a partial block too).
//
// Forward: a workgroup takes G = max(1, 256 / B2) consecutive blocks of one pooled row (b0, b1), a span of
// G B2 input columns.  Thread t owns columns t, t + 256, ... of the span (one column while B2 <= 256) and adds
// them over the B0 x B1 input rows of the block in row order: lanes walk the contiguous axis, every input
// element is read once.  The column sums go to LDS; thread g < G then adds the B2 columns of block g in column
// order (for B2 > 256, thread 0 adds the 256 strided sums in thread order) and stores scale * sum.  Sums are
// carried in fp64 and rounded once; the order is a function of the shapes alone; no atomics.
// Adjoint: one thread per element of the unpooled array, out[p] = scale * y[block of p]: coalesced stores.
// HBM model: word N (1 + 1 / prod(block)) bytes either way.
#include "common.hpp"

namespace pcs {

constexpr int kPoolBlock = 256;

struct PoolShape {
  int64_t n0, n1, n2, B0, B1, B2, m0, m1, m2;
};

// Work is laid out on a 3-D grid -- (column group, pooled row b1, pooled plane b0), each axis a uniform
// grid-stride loop -- so no thread divides a flat index; the adjoint's i / B per axis is a 32-bit division
// whenever the operands fit.
template <typename T>
__global__ __launch_bounds__(kPoolBlock) void k_pool_fwd(const T* __restrict__ x, T* __restrict__ out, PoolShape s,
                                                         int64_t G, int64_t groups, double scale) {
  __shared__ double col[kPoolBlock];
  const int64_t span = G * s.B2;
  for (int64_t b0 = blockIdx.z; b0 < s.m0; b0 += gridDim.z)
    for (int64_t b1 = blockIdx.y; b1 < s.m1; b1 += gridDim.y)
      for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int64_t c0 = grp * span;  // first input column of the span
        const int64_t r0lo = b0 * s.B0, r0hi = r0lo + s.B0 < s.n0 ? r0lo + s.B0 : s.n0;
        const int64_t r1lo = b1 * s.B1, r1hi = r1lo + s.B1 < s.n1 ? r1lo + s.B1 : s.n1;
        double acc = 0.0;
        for (int64_t c = threadIdx.x; c < span; c += kPoolBlock) {
          const int64_t i2 = c0 + c;
          if (i2 >= s.n2) break;
          for (int64_t i0 = r0lo; i0 < r0hi; ++i0)
            for (int64_t i1 = r1lo; i1 < r1hi; ++i1) acc += (double)x[(i0 * s.n1 + i1) * s.n2 + i2];
        }
        __syncthreads();  // the previous trip's readers are done with col[]
        col[threadIdx.x] = acc;
        __syncthreads();
        const int64_t b2 = grp * G + threadIdx.x;
        if ((int64_t)threadIdx.x < G && b2 < s.m2) {
          const int64_t lo = s.B2 <= kPoolBlock ? threadIdx.x * s.B2 : 0;
          const int64_t cnt = s.B2 <= kPoolBlock ? s.B2 : kPoolBlock;
          double sum = 0.0;
          for (int64_t k = 0; k < cnt; ++k) sum += col[lo + k];
          out[(b0 * s.m1 + b1) * s.m2 + b2] = (T)(scale * sum);
        }
      }
}

__device__ __forceinline__ int64_t pool_div(int64_t a, int64_t b) {
  return ((a | b) >> 32) == 0 ? (int64_t)((uint32_t)a / (uint32_t)b) : a / b;
}

// one thread per element of the unpooled array: (column tile, row i1, plane i0)
template <typename T>
__global__ __launch_bounds__(kPoolBlock) void k_pool_adj(const T* __restrict__ y, T* __restrict__ out, PoolShape s,
                                                         int64_t tiles, double scale) {
  for (int64_t i0 = blockIdx.z; i0 < s.n0; i0 += gridDim.z)
    for (int64_t i1 = blockIdx.y; i1 < s.n1; i1 += gridDim.y) {
      const int64_t yrow = (pool_div(i0, s.B0) * s.m1 + pool_div(i1, s.B1)) * s.m2, orow = (i0 * s.n1 + i1) * s.n2;
      for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t i2 = tile * kPoolBlock + threadIdx.x;
        if (i2 < s.n2) out[orow + i2] = (T)(scale * (double)y[yrow + pool_div(i2, s.B2)]);
      }
    }
}

// 1 on success, 0 for an empty array, PCS_EINVAL for bad arguments
static int pool_shape(int ndim, const int64_t* dims, const int64_t* block, PoolShape* s) {
  if (ndim < 1 || ndim > 3 || !dims || !block) return PCS_EINVAL;
  int64_t n[3] = {1, 1, 1}, B[3] = {1, 1, 1};
  for (int k = 0; k < ndim; ++k) {
    if (dims[k] < 0 || block[k] < 1) return PCS_EINVAL;
    n[3 - ndim + k] = dims[k];
    B[3 - ndim + k] = block[k] < dims[k] || dims[k] == 0 ? block[k] : dims[k];  // a block past the axis: one block
  }
  *s = PoolShape{n[0], n[1], n[2], B[0], B[1], B[2], (n[0] + B[0] - 1) / B[0], (n[1] + B[1] - 1) / B[1],
                 (n[2] + B[2] - 1) / B[2]};
  return n[0] * n[1] * n[2] > 0 ? 1 : 0;
}

// At most grid_for's 8192 workgroups over the three loop axes, x first: a workgroup that would move a few hundred
// bytes takes several trips of its grid-stride loops instead.
static dim3 pool_grid(int64_t nx, int64_t ny, int64_t nz) {
  const unsigned gx = grid_for(nx, 1), gy = grid_for(ny, 1, 8192 / gx), gz = grid_for(nz, 1, 8192 / (gx * gy));
  return dim3(gx, gy, gz);
}

template <typename T>
static int pool_fwd(const void* x, void* out, const PoolShape& s, double scale, hipStream_t st) {
  const int64_t G = s.B2 >= kPoolBlock ? 1 : kPoolBlock / s.B2;
  const int64_t groups = (s.m2 + G - 1) / G;
  const dim3 grid = pool_grid(groups, s.m1, s.m0);
  k_pool_fwd<T><<<grid, kPoolBlock, 0, st>>>((const T*)x, (T*)out, s, G, groups, scale);
  return launch_status();
}

template <typename T>
static int pool_adj(const void* y, void* out, const PoolShape& s, double scale, hipStream_t st) {
  const int64_t tiles = (s.n2 + kPoolBlock - 1) / kPoolBlock;
  const dim3 grid = pool_grid(tiles, s.n1, s.n0);
  k_pool_adj<T><<<grid, kPoolBlock, 0, st>>>((const T*)y, (T*)out, s, tiles, scale);
  return launch_status();
}

}  // namespace pcs

using namespace pcs;

extern "C" {

int pcs_pool_fwd(int dt, const void* x, void* out, int ndim, const int64_t* dims, const int64_t* block, double scale,
                 hipStream_t st) {
  PoolShape s;
  const int rc = pool_shape(ndim, dims, block, &s);
  if (rc < 0 || (dt != PCS_F32 && dt != PCS_F64)) return PCS_EINVAL;
  if (rc == 0) return PCS_OK;
  if (!x || !out || x == out) return PCS_EINVAL;
  return dt == PCS_F32 ? pool_fwd<float>(x, out, s, scale, st) : pool_fwd<double>(x, out, s, scale, st);
}

int pcs_pool_adj(int dt, const void* y, void* out, int ndim, const int64_t* dims, const int64_t* block, double scale,
                 hipStream_t st) {
  PoolShape s;
  const int rc = pool_shape(ndim, dims, block, &s);
  if (rc < 0 || (dt != PCS_F32 && dt != PCS_F64)) return PCS_EINVAL;
  if (rc == 0) return PCS_OK;
  if (!y || !out || y == out) return PCS_EINVAL;
  return dt == PCS_F32 ? pool_adj<float>(y, out, s, scale, st) : pool_adj<double>(y, out, s, scale, st);
}

}  // extern "C"
