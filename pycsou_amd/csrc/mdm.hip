// Matrix-free MappedDistanceMatrix (pycsou/linop/sampling.py:772-1058) for the Green functions of green_core.hpp:
//   out[i] = sum_j phi(d(P_i, Q_j)) x[j],   P (nrows x dim), Q (ncols x dim) row-major, dim <= PCS_MDM_MAX_DIM,
// every entry formed in registers and used once: O(nrows + ncols) memory, an N-body-style compute-bound product.
// Both distances are symmetric, so the adjoint is the same call with P and Q exchanged.
//
// The columns are cut into slabs of PCS_MDM_SLAB = 256; `ngroups` column groups take `spg` consecutive slabs each
// (the caller's plan).  With one group the result is stored directly; otherwise group g writes the doubles
// partials[g * nrows + i] and k_mdm_reduce adds the groups in group order and rounds once.
//
// Row form (nrows > PCS_MDM_SMALL_ROWS).  A 256-thread workgroup owns PCS_MDM_ROWS = 64 consecutive rows: lane = row
// in each of its four waves, the row's point in registers (dim <= 4 values).  Per slab the 256 threads stage one
// column each in LDS as a structure of arrays -- dim coordinate arrays in T and x as fp64 -- and wave w walks the
// columns [64 w, 64 w + 64) of the slab in order: every LDS read of the inner loop is one address for the whole wave
// (a broadcast: no bank conflict).  A wave carries its sum in one fp64 register per lane over all slabs of the
// group; the four sums are added in wave order through LDS.
//   LDS: 256 (4 dim + 8) + 4 * 64 * 8 bytes <= 8 KiB in fp32, <= 12 KiB in fp64 -- never what limits residency.
//   Registers: dim + 2 values of state per lane besides the temporaries of phi (pow and exp in fp64 are the
//   largest); the launch bound of 256 threads leaves the compiler the whole budget of one wave per SIMD.
// Column form (nrows <= PCS_MDM_SMALL_ROWS = 16: the adjoint of a "few knots, many samples" operator, where the row
// form would leave 60 of 64 lanes idle).  Lane = column: thread t takes column t of every slab of the group with
// the column's point and x in registers, the few row points lie in LDS (broadcast reads), and each lane holds
// PCS_MDM_SMALL_ROWS fp64 accumulators.  The workgroup then halves 256 -> 1 sums per row through LDS with fixed
// partners (t += t + s, s = 128 .. 1).
//   LDS: 16 * 4 * 8 + 16 * 256 * 8 bytes = 32.5 KiB;  registers: 16 fp64 accumulators = 32 VGPRs, dim + 1 values.
//
// fp32: distance and phi in fp32; fp64: in fp64.  In both every product phi * x and every sum is carried in fp64
// and rounded once at the store.  No atomics, no shuffles: the bits depend on (nrows, ncols, dim, spg, ngroups) and
// the data alone.  A column past ncols is never evaluated (phi of an arbitrary argument may be NaN; NaN * 0 is not 0).
#include "green_core.hpp"

namespace pcs {

constexpr int kMdmBlock = 256;
constexpr int kMdmWaves = kMdmBlock / kWave;
static_assert(kMdmBlock == PCS_MDM_SLAB, "one staged column per thread");
static_assert(PCS_MDM_ROWS == kWave, "row form: one lane per row");
static_assert(PCS_MDM_SLAB == kMdmWaves * kWave, "row form: a quarter of the slab per wave");

template <typename T>
struct MdmArgs {
  GreenSpec<T> g;
  int dk;
  T ord, inv_ord;
  const T *P, *Q, *x;
  T* out;
  double* partials;   // null: store to out
  int64_t nrows, ncols, spg;
};

template <typename T, int DIM>
__global__ __launch_bounds__(kMdmBlock) void k_mdm_row(const MdmArgs<T> a) {
  __shared__ T sQ[DIM][PCS_MDM_SLAB];
  __shared__ double sX[PCS_MDM_SLAB];
  __shared__ double sW[kMdmWaves][kWave];
  const int lane = threadIdx.x % kWave, w = threadIdx.x / kWave;
  const int64_t row = (int64_t)blockIdx.x * PCS_MDM_ROWS + lane;
  const int64_t rr = row < a.nrows ? row : a.nrows - 1;   // a lane past the last row repeats it and stores nothing
  T p[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) p[d] = a.P[rr * DIM + d];
  const int64_t nslabs = (a.ncols + PCS_MDM_SLAB - 1) / PCS_MDM_SLAB;
  const int64_t s0 = (int64_t)blockIdx.y * a.spg, s1 = s0 + a.spg < nslabs ? s0 + a.spg : nslabs;
  double acc = 0.0;
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t c0 = s * PCS_MDM_SLAB;
    const int cnt = a.ncols - c0 < PCS_MDM_SLAB ? (int)(a.ncols - c0) : PCS_MDM_SLAB;
    __syncthreads();
    {
      const int t = threadIdx.x;
      const int64_t cc = t < cnt ? c0 + t : a.ncols - 1;   // in bounds; columns past cnt are never read back
#pragma unroll
      for (int d = 0; d < DIM; ++d) sQ[d][t] = a.Q[cc * DIM + d];
      sX[t] = (double)a.x[cc];
    }
    __syncthreads();
    const int c1 = (w + 1) * kWave < cnt ? (w + 1) * kWave : cnt;
#pragma unroll 4
    for (int c = w * kWave; c < c1; ++c) {
      T q[DIM];
#pragma unroll
      for (int d = 0; d < DIM; ++d) q[d] = sQ[d][c];
      const T v = green_phi(a.g, mdm_dist<T, DIM>(a.dk, a.ord, a.inv_ord, p, q));
      acc = fma((double)v, sX[c], acc);
    }
  }
  sW[w][lane] = acc;
  __syncthreads();
  if (w == 0 && row < a.nrows) {
    double sum = sW[0][lane];
#pragma unroll
    for (int i = 1; i < kMdmWaves; ++i) sum += sW[i][lane];
    if (a.partials)
      a.partials[(int64_t)blockIdx.y * a.nrows + row] = sum;
    else
      a.out[row] = (T)sum;
  }
}

template <typename T, int DIM>
__global__ __launch_bounds__(kMdmBlock) void k_mdm_col(const MdmArgs<T> a) {
  __shared__ T sP[PCS_MDM_SMALL_ROWS][DIM];
  __shared__ double sR[PCS_MDM_SMALL_ROWS][kMdmBlock];
  const int t = threadIdx.x, nr = (int)a.nrows;
  if (t < nr * DIM) sP[t / DIM][t % DIM] = a.P[t];
  __syncthreads();
  double acc[PCS_MDM_SMALL_ROWS];
#pragma unroll
  for (int r = 0; r < PCS_MDM_SMALL_ROWS; ++r) acc[r] = 0.0;
  const int64_t nslabs = (a.ncols + PCS_MDM_SLAB - 1) / PCS_MDM_SLAB;
  const int64_t s0 = (int64_t)blockIdx.x * a.spg, s1 = s0 + a.spg < nslabs ? s0 + a.spg : nslabs;
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t c = s * PCS_MDM_SLAB + t;
    if (c < a.ncols) {
      T q[DIM];
#pragma unroll
      for (int d = 0; d < DIM; ++d) q[d] = a.Q[c * DIM + d];
      const double xv = (double)a.x[c];
#pragma unroll
      for (int r = 0; r < PCS_MDM_SMALL_ROWS; ++r) {
        if (r < nr) {
          T p[DIM];
#pragma unroll
          for (int d = 0; d < DIM; ++d) p[d] = sP[r][d];
          const T v = green_phi(a.g, mdm_dist<T, DIM>(a.dk, a.ord, a.inv_ord, p, q));
          acc[r] = fma((double)v, xv, acc[r]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < PCS_MDM_SMALL_ROWS; ++r)
    if (r < nr) sR[r][t] = acc[r];
  __syncthreads();
  for (int h = kMdmBlock / 2; h > 0; h >>= 1) {
    if (t < h)
      for (int r = 0; r < nr; ++r) sR[r][t] += sR[r][t + h];
    __syncthreads();
  }
  if (t < nr) {
    if (a.partials)
      a.partials[(int64_t)blockIdx.x * a.nrows + t] = sR[t][0];
    else
      a.out[t] = (T)sR[t][0];
  }
}

// one thread per row adds the groups in group order and rounds once
template <typename T>
__global__ __launch_bounds__(kMdmBlock) void k_mdm_reduce(int64_t nrows, int64_t ngroups,
                                                          const double* __restrict__ partials, T* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kMdmBlock + threadIdx.x;
  if (i >= nrows) return;
  double s = 0.0;
  for (int64_t g = 0; g < ngroups; ++g) s += partials[g * nrows + i];
  out[i] = (T)s;
}

template <typename T>
__global__ __launch_bounds__(kMdmBlock) void k_green_eval(const GreenSpec<T> g, const T* r, T* out, int64_t n) {
  // no __restrict__: out == r (in place) is allowed
  for (int64_t i = (int64_t)blockIdx.x * kMdmBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kMdmBlock)
    out[i] = green_phi(g, r[i]);
}

template <typename T>
static GreenSpec<T> green_spec(int kind, int k, double p0, double p1) {
  return GreenSpec<T>{kind, k, (T)p0, (T)p1};
}

template <typename T, int DIM>
static void mdm_launch(const MdmArgs<T>& a, int64_t ngroups, hipStream_t st) {
  if (a.nrows > PCS_MDM_SMALL_ROWS) {
    const dim3 grid((unsigned)((a.nrows + PCS_MDM_ROWS - 1) / PCS_MDM_ROWS), (unsigned)ngroups);
    k_mdm_row<T, DIM><<<grid, kMdmBlock, 0, st>>>(a);
  } else {
    k_mdm_col<T, DIM><<<(unsigned)ngroups, kMdmBlock, 0, st>>>(a);
  }
}

template <typename T>
static int mdm_apply(int kind, int k, double p0, double p1, int mode, double ord, int dim, const void* P,
                     int64_t nrows, const void* Q, int64_t ncols, const void* x, void* out, int64_t spg,
                     int64_t ngroups, double* partials, hipStream_t st) {
  MdmArgs<T> a;
  a.g = green_spec<T>(kind, k, p0, p1);
  a.dk = dist_kind(mode, ord);
  a.ord = (T)ord;
  a.inv_ord = (T)(1.0 / ord);
  a.P = (const T*)P, a.Q = (const T*)Q, a.x = (const T*)x, a.out = (T*)out;
  a.partials = ngroups > 1 ? partials : nullptr;
  a.nrows = nrows, a.ncols = ncols, a.spg = spg;
  switch (dim) {
    case 1: mdm_launch<T, 1>(a, ngroups, st); break;
    case 2: mdm_launch<T, 2>(a, ngroups, st); break;
    case 3: mdm_launch<T, 3>(a, ngroups, st); break;
    default: mdm_launch<T, 4>(a, ngroups, st); break;
  }
  if (ngroups > 1)
    k_mdm_reduce<T><<<(unsigned)((nrows + kMdmBlock - 1) / kMdmBlock), kMdmBlock, 0, st>>>(nrows, ngroups, partials,
                                                                                          (T*)out);
  return launch_status();
}

static bool mdm_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && na > 0 && nb > 0 && a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

constexpr int64_t kMdmMaxPoints = ((int64_t)1 << 31) - 1;

}  // namespace pcs

using namespace pcs;

extern "C" {

int pcs_green_eval(int dt, int kind, int k, double p0, double p1, const void* r, void* out, int64_t n,
                   hipStream_t st) {
  if ((dt != PCS_F32 && dt != PCS_F64) || !green_params_ok(kind, k, p0, p1) || n < 0) return PCS_EINVAL;
  if (n == 0) return PCS_OK;
  if (!r || !out) return PCS_EINVAL;
  const int64_t w = dt == PCS_F32 ? 4 : 8;
  if (r != out && mdm_overlap(out, n * w, r, n * w)) return PCS_EINVAL;   // in place is fine, a shifted view is not
  const unsigned grid = grid_for(n, kMdmBlock, 4096);
  if (dt == PCS_F32)
    k_green_eval<float><<<grid, kMdmBlock, 0, st>>>(green_spec<float>(kind, k, p0, p1), (const float*)r, (float*)out, n);
  else
    k_green_eval<double><<<grid, kMdmBlock, 0, st>>>(green_spec<double>(kind, k, p0, p1), (const double*)r,
                                                    (double*)out, n);
  return launch_status();
}

int64_t pcs_mdm_partials_len(int64_t nrows, int64_t ncols, int64_t ngroups) {
  if (nrows < 0 || ncols < 0 || nrows > kMdmMaxPoints || ncols > kMdmMaxPoints || ngroups < 1 ||
      ngroups > PCS_MDM_MAX_GROUPS)
    return -1;
  return ngroups > 1 ? ngroups * nrows : 0;
}

int pcs_mdm_apply(int dt, int kind, int k, double p0, double p1, int mode, double ord, int dim, const void* P,
                  int64_t nrows, const void* Q, int64_t ncols, const void* x, void* out, int64_t spg, int64_t ngroups,
                  void* partials, int64_t partials_len, hipStream_t st) {
  if ((dt != PCS_F32 && dt != PCS_F64) || !green_params_ok(kind, k, p0, p1)) return PCS_EINVAL;
  if (mode != PCS_MDM_RADIAL && mode != PCS_MDM_ZONAL) return PCS_EINVAL;
  if (mode == PCS_MDM_RADIAL && !(ord > 0.0)) return PCS_EINVAL;   // rejects NaN as well
  if (dim < 1 || dim > PCS_MDM_MAX_DIM) return PCS_EINVAL;
  if (nrows < 0 || ncols < 0 || nrows > kMdmMaxPoints || ncols > kMdmMaxPoints) return PCS_EINVAL;
  const int64_t nslabs = (ncols + PCS_MDM_SLAB - 1) / PCS_MDM_SLAB, ntile = nslabs > 0 ? nslabs : 1;
  if (spg < 1 || spg > ntile || ngroups < 1 || ngroups > PCS_MDM_MAX_GROUPS || ngroups != (ntile + spg - 1) / spg ||
      partials_len < 0)
    return PCS_EINVAL;
  if (ngroups > 1 && (!partials || ((uintptr_t)partials & 7) || partials_len / ngroups < nrows)) return PCS_EINVAL;
  if (nrows == 0) return PCS_OK;
  if (!P || !out || (ncols > 0 && (!Q || !x))) return PCS_EINVAL;
  const int64_t w = dt == PCS_F32 ? 4 : 8;
  if (mdm_overlap(out, nrows * w, P, nrows * dim * w) || mdm_overlap(out, nrows * w, Q, ncols * dim * w) ||
      mdm_overlap(out, nrows * w, x, ncols * w) ||
      (ngroups > 1 && (mdm_overlap(out, nrows * w, partials, ngroups * nrows * 8) ||
                       mdm_overlap(partials, ngroups * nrows * 8, P, nrows * dim * w) ||
                       mdm_overlap(partials, ngroups * nrows * 8, Q, ncols * dim * w) ||
                       mdm_overlap(partials, ngroups * nrows * 8, x, ncols * w))))
    return PCS_EINVAL;
  return dt == PCS_F32 ? mdm_apply<float>(kind, k, p0, p1, mode, ord, dim, P, nrows, Q, ncols, x, out, spg, ngroups,
                                          (double*)partials, st)
                       : mdm_apply<double>(kind, k, p0, p1, mode, ord, dim, P, nrows, Q, ncols, x, out, spg, ngroups,
                                           (double*)partials, st);
}

}  // extern "C"
