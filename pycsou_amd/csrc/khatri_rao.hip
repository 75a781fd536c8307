// Khatri-Rao product of two dense row-major factors A (k x l) and B (n x l) (KhatriRaoProduct,
// pycsou/linop/base.py:889-989, the dense branch):
//   forward  Y (n x k) = sum_c x[c] B[:, c] A[:, c]^T  = (B * x) A^T
//   adjoint  out[c]    = B[:, c]^T Y A[:, c]           = sum(((A^T Y^T)^T * B), axis 0)
// for a small output n k and a long l (tens of sensors against 10^4 - 10^5 directions).  There the product is
// bound by reading A and B once; the unfused composition writes and re-reads an n x l intermediate.
//
// Forward.  The columns are cut into slabs of PCS_KR_SLAB = 64 (one 256- or 512-byte segment per matrix row:
// every global load is coalesced).  Workgroup g takes `spg` consecutive slabs (the host's plan: at most
// PCS_KR_MAX_GROUPS workgroups).  Per slab it stages A's slab (k x 64, dtype) and the x-scaled slab of B
// (n x 64, as fp64: an fp32 product is exact there) in LDS, rows padded by one element so that the 64 lanes,
// which read 64 different rows of A's slab at one column, hit different banks; the B operand is one address
// per output row (broadcast).  Thread t owns the output entries e = t, t + 256, ... (at most 4) and adds the
// slab's 64 columns to them in column order, slab after slab, in registers; the workgroup writes
// partials[g][e].  k_kr_reduce: 8 lanes per entry add the groups g = q, q + 8, ... in order, then the 8 sums are
// added in lane order, and the entry is rounded once.
// Adjoint.  A workgroup of four waves takes 64 consecutive columns, one lane per column c in every wave: every
// load of A and B is coalesced; Y lies in LDS as fp64 and every read of it is a broadcast.  Rows of Y are taken
// 8 at a time (t[8] in registers); wave w takes the row blocks w, w + 4, ... in order, so A's column is read
// ceil(n / 8) times (from L1/L2 after the first) by waves that run side by side; the four waves' sums are added
// in wave order through LDS.  No shuffle, no atomics.
//
// The fused limit: n k <= PCS_KR_MAX_NK = 1024 (4 accumulators per thread of a 256-thread workgroup, Y = 8 KiB of
// LDS in the adjoint, a group's partials at most 8 KiB against the >= 16 KiB it reads per slab at k + n >= 64)
// and k + n <= PCS_KR_MAX_ROWS = 120 (forward LDS (8 n + word k) 65 <= 120 * 65 * 8 = 62400 bytes, under the
// 64 KiB a workgroup may ask for, two workgroups per CU of 160 KiB).  Beyond it the caller composes the product.
//
// Sums are carried in fp64 for both dtypes and rounded once at the store.  Every order of summation is a
// function of (k, n, l, spg) alone: two calls return the same bits.  No atomics.
// HBM model: forward  word (k + n + 1) l + 16 n k ngroups + word n k;  adjoint  word (k + n + 1) l + word n k.
#include "common.hpp"

namespace pcs {

constexpr int kKrBlock = 256;
constexpr int kKrAdjBlock = 256;
constexpr int kKrAdjWaves = kKrAdjBlock / kWave;
constexpr int kKrRedEntries = 32;
constexpr int kKrRedLanes = 8;
constexpr int kKrLd = PCS_KR_SLAB + 1;
constexpr int kKrOwn = PCS_KR_MAX_NK / kKrBlock;
constexpr int kKrJb = 8;

template <typename T>
__global__ __launch_bounds__(kKrBlock) void k_kr_fwd(const T* __restrict__ A, const T* __restrict__ B,
                                                     const T* __restrict__ x, int64_t k, int64_t n, int64_t l,
                                                     int64_t spg, double* __restrict__ partials) {
  extern __shared__ __align__(16) unsigned char kr_smem[];
  double* sB = (double*)kr_smem;          // n x kKrLd
  T* sA = (T*)(sB + n * kKrLd);           // k x kKrLd
  const int64_t nk = n * k, nslabs = (l + PCS_KR_SLAB - 1) / PCS_KR_SLAB;
  const int64_t s0 = blockIdx.x * spg, s1 = s0 + spg < nslabs ? s0 + spg : nslabs;
  const int col = threadIdx.x % PCS_KR_SLAB, row0 = threadIdx.x / PCS_KR_SLAB;
  double acc[kKrOwn];
  int rowA[kKrOwn], rowB[kKrOwn];
#pragma unroll
  for (int q = 0; q < kKrOwn; ++q) {
    const int64_t e = threadIdx.x + q * kKrBlock;
    acc[q] = 0.0;
    rowB[q] = e < nk ? (int)(e / k) * kKrLd : 0;
    rowA[q] = e < nk ? (int)(e % k) * kKrLd : 0;
  }
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t c0 = s * PCS_KR_SLAB;
    __syncthreads();
    {
      // a thread stages one column of the slab, every fourth row: the loads of a pass are unconditional (a column
      // past l re-reads column l - 1 and stores 0), so the unrolled passes have their loads in flight together
      const bool in = c0 + col < l;
      const int64_t cc = in ? c0 + col : l - 1;
      const double xv = (double)x[cc];
#pragma unroll 8
      for (int64_t row = row0; row < n; row += kKrBlock / PCS_KR_SLAB) {
        const double v = xv * (double)B[row * l + cc];
        sB[row * kKrLd + col] = in ? v : 0.0;
      }
#pragma unroll 8
      for (int64_t row = row0; row < k; row += kKrBlock / PCS_KR_SLAB) {
        const T v = A[row * l + cc];
        sA[row * kKrLd + col] = in ? v : T(0);
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kKrOwn; ++q) {
      if (threadIdx.x + q * kKrBlock < nk) {
        const double* b = sB + rowB[q];
        const T* a = sA + rowA[q];
        double v = acc[q];
        for (int c = 0; c < PCS_KR_SLAB; ++c) v = fma(b[c], (double)a[c], v);
        acc[q] = v;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kKrOwn; ++q) {
    const int64_t e = threadIdx.x + q * kKrBlock;
    if (e < nk) partials[blockIdx.x * nk + e] = acc[q];
  }
}

// 32 consecutive entries per workgroup, 8 lanes of groups each: lane q adds groups q, q + 8, ... in order, then the
// 8 sums are added in lane order
template <typename T>
__global__ __launch_bounds__(kKrRedEntries * kKrRedLanes) void k_kr_reduce(int64_t nk, int64_t ngroups,
                                                                          const double* __restrict__ partials,
                                                                          T* __restrict__ out) {
  __shared__ double sm[kKrRedLanes][kKrRedEntries];
  const int el = threadIdx.x % kKrRedEntries, q = threadIdx.x / kKrRedEntries;
  const int64_t e = blockIdx.x * (int64_t)kKrRedEntries + el;
  double acc = 0.0;
  if (e < nk) {
#pragma unroll 4
    for (int64_t g = q; g < ngroups; g += kKrRedLanes) acc += partials[g * nk + e];
  }
  sm[q][el] = acc;
  __syncthreads();
  if (q == 0 && e < nk) {
    double s = sm[0][el];
#pragma unroll
    for (int i = 1; i < kKrRedLanes; ++i) s += sm[i][el];
    out[e] = (T)s;
  }
}

template <typename T>
__global__ __launch_bounds__(kKrAdjBlock) void k_kr_adj(const T* __restrict__ A, const T* __restrict__ B,
                                                        const T* __restrict__ Y, int64_t k, int64_t n, int64_t l,
                                                        T* __restrict__ out) {
  __shared__ double sY[PCS_KR_MAX_NK];
  __shared__ double sP[kKrAdjWaves][kWave];
  for (int64_t e = threadIdx.x; e < n * k; e += kKrAdjBlock) sY[e] = (double)Y[e];
  __syncthreads();
  const int cl = threadIdx.x % kWave, w = threadIdx.x / kWave;
  const int64_t ntiles = (l + kWave - 1) / kWave;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t c = tile * kWave + cl;
    double acc = 0.0;
    if (c < l) {
      for (int64_t j0 = (int64_t)w * kKrJb; j0 < n; j0 += kKrAdjWaves * kKrJb) {
        const int nj = n - j0 < kKrJb ? (int)(n - j0) : kKrJb;
        double t[kKrJb];
#pragma unroll
        for (int jj = 0; jj < kKrJb; ++jj) t[jj] = 0.0;
#pragma unroll 4
        for (int64_t i = 0; i < k; ++i) {
          const double a = (double)A[i * l + c];
#pragma unroll
          for (int jj = 0; jj < kKrJb; ++jj)
            if (jj < nj) t[jj] = fma(sY[(j0 + jj) * k + i], a, t[jj]);
        }
#pragma unroll
        for (int jj = 0; jj < kKrJb; ++jj)
          if (jj < nj) acc = fma((double)B[(j0 + jj) * l + c], t[jj], acc);
      }
    }
    sP[w][cl] = acc;
    __syncthreads();
    if (w == 0 && c < l) {
      double s = sP[0][cl];
#pragma unroll
      for (int i = 1; i < kKrAdjWaves; ++i) s += sP[i][cl];
      out[c] = (T)s;
    }
    __syncthreads();
  }
}

static bool kr_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return na > 0 && nb > 0 && a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

static bool kr_shape_ok(int dt, int64_t k, int64_t n, int64_t l) {
  if (dt != PCS_F32 && dt != PCS_F64) return false;
  if (k < 0 || n < 0 || l < 0 || l > ((int64_t)1 << 40)) return false;
  return k + n <= PCS_KR_MAX_ROWS && k * n <= PCS_KR_MAX_NK;
}

template <typename T>
static int kr_fwd(const void* A, const void* B, const void* x, void* out, int64_t k, int64_t n, int64_t l,
                  int64_t spg, int64_t ngroups, double* partials, hipStream_t st) {
  if (ngroups > 0) {
    const size_t lds = (size_t)kKrLd * ((size_t)n * sizeof(double) + (size_t)k * sizeof(T));
    k_kr_fwd<T><<<(unsigned)ngroups, kKrBlock, lds, st>>>((const T*)A, (const T*)B, (const T*)x, k, n, l, spg,
                                                          partials);
  }
  k_kr_reduce<T><<<grid_for(n * k, kKrRedEntries), kKrRedEntries * kKrRedLanes, 0, st>>>(n * k, ngroups, partials,
                                                                                        (T*)out);
  return launch_status();
}

}  // namespace pcs

using namespace pcs;

extern "C" {

int pcs_khatri_rao_fwd(int dt, const void* A, const void* B, const void* x, void* out, int64_t k, int64_t n,
                       int64_t l, int64_t spg, int64_t ngroups, void* partials, int64_t partials_len,
                       hipStream_t st) {
  if (!kr_shape_ok(dt, k, n, l)) return PCS_EINVAL;
  const int64_t nslabs = (l + PCS_KR_SLAB - 1) / PCS_KR_SLAB;
  if (spg < 1 || ngroups < 0 || ngroups > PCS_KR_MAX_GROUPS || ngroups != (nslabs + spg - 1) / spg || partials_len < 0)
    return PCS_EINVAL;
  if (k * n == 0) return PCS_OK;
  if (!out || (l > 0 && (!A || !B || !x))) return PCS_EINVAL;
  if (ngroups > 0 && (!partials || ((uintptr_t)partials & 7) || partials_len / (k * n) < ngroups)) return PCS_EINVAL;
  const int64_t w = dt == PCS_F32 ? 4 : 8;
  if (kr_overlap(out, n * k * w, A, k * l * w) || kr_overlap(out, n * k * w, B, n * l * w) ||
      kr_overlap(out, n * k * w, x, l * w) || kr_overlap(out, n * k * w, partials, ngroups * n * k * 8))
    return PCS_EINVAL;
  return dt == PCS_F32 ? kr_fwd<float>(A, B, x, out, k, n, l, spg, ngroups, (double*)partials, st)
                       : kr_fwd<double>(A, B, x, out, k, n, l, spg, ngroups, (double*)partials, st);
}

int pcs_khatri_rao_adj(int dt, const void* A, const void* B, const void* Y, void* out, int64_t k, int64_t n,
                       int64_t l, hipStream_t st) {
  if (!kr_shape_ok(dt, k, n, l)) return PCS_EINVAL;
  if (l == 0) return PCS_OK;
  if (!out || (k * n > 0 && (!A || !B || !Y))) return PCS_EINVAL;
  const int64_t w = dt == PCS_F32 ? 4 : 8;
  if (kr_overlap(out, l * w, A, k * l * w) || kr_overlap(out, l * w, B, n * l * w) ||
      kr_overlap(out, l * w, Y, n * k * w))
    return PCS_EINVAL;
  const unsigned grid = grid_for(l, kWave, 8192);
  if (dt == PCS_F32)
    k_kr_adj<float><<<grid, kKrAdjBlock, 0, st>>>((const float*)A, (const float*)B, (const float*)Y, k, n, l,
                                                  (float*)out);
  else
    k_kr_adj<double><<<grid, kKrAdjBlock, 0, st>>>((const double*)A, (const double*)B, (const double*)Y, k, n, l,
                                                   (double*)out);
  return launch_status();
}

}  // extern "C"
