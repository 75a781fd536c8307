// CSR sparse matrix times a row-major dense matrix, along either axis of the dense one (the sparse factors of
// KroneckerProduct / KroneckerSum, pycsou/linop/base.py:715-886: B X and X A^T for X of shape (m, l)).
//
//   axis 0:  out (nrows x nb) = A X,    X (ncols x nb)   -- every CSR entry multiplies a contiguous row of X
//   axis 1:  out (nb x nrows) = X A^T,  X (nb x ncols)   -- every row of X is one SpMV
// `accumulate` makes it out = out + ..., the sum still rounded once: out = (T)((double)out + acc).
//
// Axis 0, nb > 1 (k_spmm_cols): W lanes (a power of two, at most a wave, chosen by the host from nb) lie across
// W consecutive columns of one row of out, 256 / W rows per workgroup trip, the column tiles on grid y.  A lane
// walks its row's entries in order: vals[k] and colind[k] are the same address in the W lanes (one broadcast
// load), X[colind[k] * nb + j] and the store are consecutive in j, so coalesced.  No cross-lane step at all.  A
// long row is walked like any other (its W columns still run side by side).
//
// Axis 1 (k_spmm_rows / k_spmm_chunks / k_spmm_long_rows): the lane-group, chunk and long-row scheme of
// pcs_csr_spmv (spmv.hip) with the batch b on grid y: x = X + b ncols, out = out + b nrows, partials + b nchunks.
// The statements that sum are the ones of spmv.hip in the same order, so batch row b holds the bits pcs_csr_spmv
// returns for that row of X.  With nb == 1 the two layouts are the same vector product and both axes run this
// path: the result is pcs_csr_spmv's bit for bit.
//
// Sums are carried in fp64 for both dtypes (an fp32 product is exact in fp64) and rounded once at the store.
// Every order of summation is a function of (rowptr, lanes, axis, nb == 1) alone: two calls return the same
// bits.  No atomics.
// HBM model, axis 0: nnz (word + 4) + 8 nrows + word nb (ncols + nrows) bytes when the rows of X that a
// workgroup's rows share stay in L2 (nnz word nb of gathered reads otherwise); accumulate adds word nb nrows.
// Axis 1: nb times the vector model of spmv.hip less the matrix, which the batch re-reads from L2 / Infinity
// Cache: nnz (word + 4) + 8 nrows + word nb (ncols + nrows) + 16 nb nchunks bytes.
#include "common.hpp"

namespace pcs {

constexpr int kSpmmBlock = 256;

template <typename T>
__device__ __forceinline__ double spmm_span(const T* __restrict__ vals, const int32_t* __restrict__ colind,
                                            const T* __restrict__ x, int64_t k, int64_t e, int64_t stride) {
  double acc = 0.0;
  for (; k < e; k += stride) acc = fma((double)vals[k], (double)x[colind[k]], acc);
  return acc;
}

template <typename T>
__device__ __forceinline__ void spmm_store(T* p, double acc, int accumulate) {
  *p = (T)(accumulate ? (double)*p + acc : acc);
}

// axis 0: W lanes across the columns of one row
template <typename T>
__global__ __launch_bounds__(kSpmmBlock) void k_spmm_cols(int64_t nrows, int64_t nb, int W,
                                                          const int64_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ colind,
                                                          const T* __restrict__ vals, const T* __restrict__ X,
                                                          T* __restrict__ out, int accumulate) {
  const int64_t rpb = kSpmmBlock / W;
  const int64_t g = threadIdx.x / W;
  const int64_t ntiles = (nb + W - 1) / W;
  for (int64_t tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
    const int64_t j = tile * W + threadIdx.x % W;
    for (int64_t base = blockIdx.x * rpb; base < nrows; base += (int64_t)gridDim.x * rpb) {
      const int64_t r = base + g;
      if (r >= nrows || j >= nb) continue;
      const int64_t e = rowptr[r + 1];
      double acc = 0.0;
      for (int64_t k = rowptr[r]; k < e; ++k) acc = fma((double)vals[k], (double)X[(int64_t)colind[k] * nb + j], acc);
      spmm_store(out + r * nb + j, acc, accumulate);
    }
  }
}

// axis 1: L lanes per row, the batch on grid y
template <typename T, int L>
__global__ __launch_bounds__(kSpmmBlock) void k_spmm_rows(int64_t nrows, int64_t ncols, int64_t nb,
                                                          const int64_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ colind,
                                                          const T* __restrict__ vals, const T* __restrict__ X,
                                                          T* __restrict__ out, int accumulate) {
  constexpr int64_t RPB = kSpmmBlock / L;
  const int j = threadIdx.x % L;
  const int64_t g = threadIdx.x / L;
  for (int64_t b = blockIdx.y; b < nb; b += gridDim.y) {
    const T* x = X + b * ncols;
    for (int64_t base = blockIdx.x * RPB; base < nrows; base += (int64_t)gridDim.x * RPB) {
      const int64_t r = base + g;
      int64_t s = 0, e = 0;
      if (r < nrows) {
        s = rowptr[r];
        e = rowptr[r + 1];
      }
      const bool is_long = e - s > PCS_SPMV_LONG_ROW;
      double acc = is_long ? 0.0 : spmm_span<T>(vals, colind, x, s + j, e, L);
#pragma unroll
      for (int o = L / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
      if (j == 0 && r < nrows && !is_long) spmm_store(out + b * nrows + r, acc, accumulate);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kSpmmBlock) void k_spmm_chunks(int64_t nchunks, int64_t ncols, int64_t nb,
                                                            const int64_t* __restrict__ chunk_row,
                                                            const int64_t* __restrict__ chunk_start,
                                                            const int64_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ colind,
                                                            const T* __restrict__ vals, const T* __restrict__ X,
                                                            double* __restrict__ partials) {
  __shared__ double sm[kSpmmBlock / kWave];
  for (int64_t b = blockIdx.y; b < nb; b += gridDim.y) {
    const T* x = X + b * ncols;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
      const int64_t s = chunk_start[c], row_end = rowptr[chunk_row[c] + 1];
      const int64_t e = s + PCS_SPMV_CHUNK < row_end ? s + PCS_SPMV_CHUNK : row_end;
      double v[1] = {spmm_span<T>(vals, colind, x, s + threadIdx.x, e, kSpmmBlock)};
      block_sum<1>(v, sm);
      if (threadIdx.x == 0) partials[b * nchunks + c] = v[0];
    }
  }
}

template <typename T>
__global__ void k_spmm_long_rows(int64_t nlong, int64_t nrows, int64_t nchunks, int64_t nb,
                                 const int64_t* __restrict__ long_row, const int64_t* __restrict__ long_first,
                                 const double* __restrict__ partials, T* __restrict__ out, int accumulate) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nlong) return;
  for (int64_t b = blockIdx.y; b < nb; b += gridDim.y) {
    double acc = 0.0;
    for (int64_t c = long_first[i]; c < long_first[i + 1]; ++c) acc += partials[b * nchunks + c];
    spmm_store(out + b * nrows + long_row[i], acc, accumulate);
  }
}

static unsigned grid_y(int64_t n) { return (unsigned)(n < 1 ? 1 : n > 65535 ? 65535 : n); }

template <typename T, int L>
static void launch_spmm_rows(int64_t nrows, int64_t ncols, int64_t nb, const int64_t* rowptr, const int32_t* colind,
                             const void* vals, const void* X, void* out, int accumulate, hipStream_t st) {
  const int64_t rpb = kSpmmBlock / L;
  const dim3 grid(grid_for((nrows + rpb - 1) / rpb, 1, 65536), grid_y(nb));
  k_spmm_rows<T, L><<<grid, kSpmmBlock, 0, st>>>(nrows, ncols, nb, rowptr, colind, (const T*)vals, (const T*)X,
                                                 (T*)out, accumulate);
}

template <typename T>
static int spmm(int axis, int accumulate, int64_t nrows, int64_t ncols, const int64_t* rowptr, const int32_t* colind,
                const void* vals, const void* X, void* out, int64_t nb, int lanes, int64_t nchunks,
                const int64_t* chunk_row, const int64_t* chunk_start, int64_t nlong, const int64_t* long_row,
                const int64_t* long_first, double* partials, hipStream_t st) {
  if (axis == 0 && nb > 1) {
    int W = 1;
    while (W < kWave && W < nb) W *= 2;
    const int64_t rpb = kSpmmBlock / W;
    const dim3 grid(grid_for((nrows + rpb - 1) / rpb, 1, 65536), grid_y((nb + W - 1) / W));
    k_spmm_cols<T><<<grid, kSpmmBlock, 0, st>>>(nrows, nb, W, rowptr, colind, (const T*)vals, (const T*)X, (T*)out,
                                                accumulate);
    return launch_status();
  }
  switch (lanes) {
    case 1: launch_spmm_rows<T, 1>(nrows, ncols, nb, rowptr, colind, vals, X, out, accumulate, st); break;
    case 2: launch_spmm_rows<T, 2>(nrows, ncols, nb, rowptr, colind, vals, X, out, accumulate, st); break;
    case 4: launch_spmm_rows<T, 4>(nrows, ncols, nb, rowptr, colind, vals, X, out, accumulate, st); break;
    case 8: launch_spmm_rows<T, 8>(nrows, ncols, nb, rowptr, colind, vals, X, out, accumulate, st); break;
    case 16: launch_spmm_rows<T, 16>(nrows, ncols, nb, rowptr, colind, vals, X, out, accumulate, st); break;
    case 32: launch_spmm_rows<T, 32>(nrows, ncols, nb, rowptr, colind, vals, X, out, accumulate, st); break;
    default: launch_spmm_rows<T, 64>(nrows, ncols, nb, rowptr, colind, vals, X, out, accumulate, st); break;
  }
  if (nchunks > 0) {
    k_spmm_chunks<T><<<dim3(grid_for(nchunks, 1, 65536), grid_y(nb)), kSpmmBlock, 0, st>>>(
        nchunks, ncols, nb, chunk_row, chunk_start, rowptr, colind, (const T*)vals, (const T*)X, partials);
    k_spmm_long_rows<T><<<dim3(grid_for(nlong, 64), grid_y(nb)), 64, 0, st>>>(nlong, nrows, nchunks, nb, long_row,
                                                                              long_first, partials, (T*)out,
                                                                              accumulate);
  }
  return launch_status();
}

static bool spmm_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

}  // namespace pcs

using namespace pcs;

extern "C" {

int pcs_csr_spmm(int dt, int axis, int accumulate, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* rowptr,
                 const int32_t* colind, const void* vals, const void* X, void* out, int64_t nb, int lanes,
                 int64_t nchunks, const int64_t* chunk_row, const int64_t* chunk_start, int64_t nlong,
                 const int64_t* long_row, const int64_t* long_first, void* partials, int64_t partials_len,
                 hipStream_t st) {
  if (dt != PCS_F32 && dt != PCS_F64) return PCS_EINVAL;
  if ((axis != 0 && axis != 1) || (accumulate != 0 && accumulate != 1)) return PCS_EINVAL;
  if (nrows < 0 || ncols < 0 || nnz < 0 || nb < 0 || nchunks < 0 || nlong < 0 || partials_len < 0 ||
      ncols >= ((int64_t)1 << 31))
    return PCS_EINVAL;
  // element counts of X and out stay far inside int64
  const int64_t big = (int64_t)1 << 40;
  if (nb > big || nrows > big || (nb > 0 && (nrows > big / nb || ncols > big / nb))) return PCS_EINVAL;
  if (lanes < 1 || lanes > 64 || (lanes & (lanes - 1))) return PCS_EINVAL;
  const bool work = nrows > 0 && nb > 0;
  if (!rowptr || (work && !out) || (nnz > 0 && (!colind || !vals || ncols == 0 || nrows == 0 || (nb > 0 && !X))))
    return PCS_EINVAL;
  if ((nchunks > 0) != (nlong > 0) || nlong > nchunks || nchunks > nnz / PCS_SPMV_CHUNK + nlong) return PCS_EINVAL;
  const bool by_rows = axis == 1 || nb == 1;
  if (nchunks > 0 && (!chunk_row || !chunk_start || !long_row || !long_first)) return PCS_EINVAL;
  if (nchunks > 0 && by_rows && nb > 0 &&
      (!partials || ((uintptr_t)partials & 7) || partials_len / nb < nchunks))
    return PCS_EINVAL;
  const int64_t w = dt == PCS_F32 ? 4 : 8;
  if (work && X && ncols > 0 && spmm_overlap(out, nrows * nb * w, X, ncols * nb * w)) return PCS_EINVAL;
  if (!work) return PCS_OK;
  return dt == PCS_F32 ? spmm<float>(axis, accumulate, nrows, ncols, rowptr, colind, vals, X, out, nb, lanes, nchunks,
                                     chunk_row, chunk_start, nlong, long_row, long_first, (double*)partials, st)
                       : spmm<double>(axis, accumulate, nrows, ncols, rowptr, colind, vals, X, out, nb, lanes, nchunks,
                                      chunk_row, chunk_start, nlong, long_row, long_first, (double*)partials, st);
}

}  // extern "C"
