// CSR sparse matrix-vector product  out = A x  (SparseLinearOperator, the sparse MappedDistanceMatrix and the
// adjoint of NNSampling: pycsou/linop/base.py:121-137, pycsou/linop/sampling.py:680-687, 975-1007 ->
// scipy.sparse csr_matrix.dot).
//
// Short rows (at most PCS_SPMV_LONG_ROW entries): a group of L lanes serves one row, L in {1, 2, ..., 64}
// chosen by the host once per matrix from nnz / nrows.  Lane j sums entries j, j + L, ... of its row in that
// order, then the group combines with a fixed __shfl_xor tree (offsets L/2, ..., 1).  Consecutive lanes read
// consecutive vals / colind, so those two streams are coalesced; the gather of x relies on L2 and Infinity
// Cache.  Every lane of the block runs the same number of trips of the row loop and takes part in every
// shuffle: a group past the last row sums nothing.
//
// Long rows (the transpose of a tall thin matrix has a few rows of very many entries): the host cuts every
// row of more than PCS_SPMV_LONG_ROW entries into chunks of PCS_SPMV_CHUNK entries at construction (the
// matrix is fixed).  k_chunks: one workgroup sums one chunk -- thread t takes entries t, t + 256, ... in
// order, then the fixed wave tree and the waves in order -- into partials[chunk].  k_long_rows: one thread per
// long row adds that row's partials in chunk order and stores the row.  The short kernel skips long rows, so
// every row of `out` is written exactly once.
//
// Sums are carried in fp64 for both dtypes (an fp32 product is exact in fp64) and rounded once at the store.
// Every order of summation is a function of (rowptr, L) alone: two calls return the same bits.  No atomics.
// HBM model: nnz (word + 4) + 8 nrows + word (ncols + nrows) bytes.
#include "common.hpp"

namespace pcs {

constexpr int kSpmvBlock = 256;

template <typename T>
__device__ __forceinline__ double spmv_span(const T* __restrict__ vals, const int32_t* __restrict__ colind,
                                            const T* __restrict__ x, int64_t k, int64_t e, int64_t stride) {
  double acc = 0.0;
  for (; k < e; k += stride) acc = fma((double)vals[k], (double)x[colind[k]], acc);
  return acc;
}

// L lanes per row, kSpmvBlock / L rows per workgroup trip
template <typename T, int L>
__global__ __launch_bounds__(kSpmvBlock) void k_spmv_rows(int64_t nrows, const int64_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ colind,
                                                          const T* __restrict__ vals, const T* __restrict__ x,
                                                          T* __restrict__ out) {
  constexpr int64_t RPB = kSpmvBlock / L;
  const int j = threadIdx.x % L;
  const int64_t g = threadIdx.x / L;
  for (int64_t base = blockIdx.x * RPB; base < nrows; base += (int64_t)gridDim.x * RPB) {
    const int64_t r = base + g;
    int64_t s = 0, e = 0;
    if (r < nrows) {
      s = rowptr[r];
      e = rowptr[r + 1];
    }
    const bool is_long = e - s > PCS_SPMV_LONG_ROW;
    double acc = is_long ? 0.0 : spmv_span<T>(vals, colind, x, s + j, e, L);
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
    if (j == 0 && r < nrows && !is_long) out[r] = (T)acc;
  }
}

template <typename T>
__global__ __launch_bounds__(kSpmvBlock) void k_spmv_chunks(int64_t nchunks, const int64_t* __restrict__ chunk_row,
                                                            const int64_t* __restrict__ chunk_start,
                                                            const int64_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ colind,
                                                            const T* __restrict__ vals, const T* __restrict__ x,
                                                            double* __restrict__ partials) {
  __shared__ double sm[kSpmvBlock / kWave];
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t s = chunk_start[c], row_end = rowptr[chunk_row[c] + 1];
    const int64_t e = s + PCS_SPMV_CHUNK < row_end ? s + PCS_SPMV_CHUNK : row_end;
    double v[1] = {spmv_span<T>(vals, colind, x, s + threadIdx.x, e, kSpmvBlock)};
    block_sum<1>(v, sm);
    if (threadIdx.x == 0) partials[c] = v[0];
  }
}

template <typename T>
__global__ void k_spmv_long_rows(int64_t nlong, const int64_t* __restrict__ long_row,
                                 const int64_t* __restrict__ long_first, const double* __restrict__ partials,
                                 T* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nlong) return;
  double acc = 0.0;
  for (int64_t c = long_first[i]; c < long_first[i + 1]; ++c) acc += partials[c];
  out[long_row[i]] = (T)acc;
}

template <typename T, int L>
static void launch_rows(int64_t nrows, const int64_t* rowptr, const int32_t* colind, const void* vals, const void* x,
                        void* out, hipStream_t st) {
  const int64_t rpb = kSpmvBlock / L;
  k_spmv_rows<T, L><<<grid_for((nrows + rpb - 1) / rpb, 1, 65536), kSpmvBlock, 0, st>>>(
      nrows, rowptr, colind, (const T*)vals, (const T*)x, (T*)out);
}

template <typename T>
static int spmv(int64_t nrows, const int64_t* rowptr, const int32_t* colind, const void* vals, const void* x,
                void* out, int lanes, int64_t nchunks, const int64_t* chunk_row, const int64_t* chunk_start,
                int64_t nlong, const int64_t* long_row, const int64_t* long_first, double* partials, hipStream_t st) {
  switch (lanes) {
    case 1: launch_rows<T, 1>(nrows, rowptr, colind, vals, x, out, st); break;
    case 2: launch_rows<T, 2>(nrows, rowptr, colind, vals, x, out, st); break;
    case 4: launch_rows<T, 4>(nrows, rowptr, colind, vals, x, out, st); break;
    case 8: launch_rows<T, 8>(nrows, rowptr, colind, vals, x, out, st); break;
    case 16: launch_rows<T, 16>(nrows, rowptr, colind, vals, x, out, st); break;
    case 32: launch_rows<T, 32>(nrows, rowptr, colind, vals, x, out, st); break;
    default: launch_rows<T, 64>(nrows, rowptr, colind, vals, x, out, st); break;
  }
  if (nchunks > 0) {
    k_spmv_chunks<T><<<grid_for(nchunks, 1, 65536), kSpmvBlock, 0, st>>>(nchunks, chunk_row, chunk_start, rowptr,
                                                                        colind, (const T*)vals, (const T*)x, partials);
    k_spmv_long_rows<T><<<grid_for(nlong, 64), 64, 0, st>>>(nlong, long_row, long_first, partials, (T*)out);
  }
  return launch_status();
}

static bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

}  // namespace pcs

using namespace pcs;

extern "C" {

int pcs_csr_spmv(int dt, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* rowptr, const int32_t* colind,
                 const void* vals, const void* x, void* out, int lanes, int64_t nchunks, const int64_t* chunk_row,
                 const int64_t* chunk_start, int64_t nlong, const int64_t* long_row, const int64_t* long_first,
                 void* partials, hipStream_t st) {
  if (dt != PCS_F32 && dt != PCS_F64) return PCS_EINVAL;
  if (nrows < 0 || ncols < 0 || nnz < 0 || nchunks < 0 || nlong < 0 || ncols >= ((int64_t)1 << 31)) return PCS_EINVAL;
  if (lanes < 1 || lanes > 64 || (lanes & (lanes - 1))) return PCS_EINVAL;
  if (!rowptr || (nrows > 0 && !out) || (nnz > 0 && (!colind || !vals || !x || ncols == 0 || nrows == 0)))
    return PCS_EINVAL;
  // a chunk belongs to a long row and a long row has chunks; a long row holds more than one chunk's entries
  if ((nchunks > 0) != (nlong > 0) || nlong > nchunks || nchunks > nnz / PCS_SPMV_CHUNK + nlong) return PCS_EINVAL;
  if (nchunks > 0 && (!chunk_row || !chunk_start || !long_row || !long_first || !partials ||
                      ((uintptr_t)partials & 7)))
    return PCS_EINVAL;
  const int64_t w = dt == PCS_F32 ? 4 : 8;
  if (nrows > 0 && x && ncols > 0 && overlap(out, nrows * w, x, ncols * w)) return PCS_EINVAL;
  if (nrows == 0) return PCS_OK;
  return dt == PCS_F32 ? spmv<float>(nrows, rowptr, colind, vals, x, out, lanes, nchunks, chunk_row, chunk_start,
                                     nlong, long_row, long_first, (double*)partials, st)
                       : spmv<double>(nrows, rowptr, colind, vals, x, out, lanes, nchunks, chunk_row, chunk_start,
                                      nlong, long_row, long_first, (double*)partials, st);
}

}  // extern "C"
