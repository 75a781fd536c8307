// Batched conjugate gradients on the normal equations (A^T A + eps^2 I) x = A^T y: the vector work and the
// scalar recurrences between two applications of the operator (LinearOperator.pinv, pycsou/core/linop.py:397-420
// -> pylops NormalEquationsInversion -> scipy.sparse.linalg.cg; LinOpPinv, linop.py:618-629).
//
// nb independent systems, system j = row j of contiguous (nb, n) arrays (the layout of _apply_cols(T, axis=1)).
// One iteration, SciPy's recurrences operation for operation (this file is built with -ffp-contract=off: a
// contracted beta * p + r would round once where NumPy rounds twice):
//   pcs_cg_dir      p = beta p + r                       (p = r while Ctrl::it == 0)      reads 2n, writes n
//   (caller)        q = A^T (A p)
//   pcs_cg_dot      pq = sum p (q + eps2 p), alpha = rho / pq                             reads 2n
//   pcs_cg_update   x += alpha p, r -= alpha (q + eps2 p), rho' = sum r r,                reads 4n, writes 2n
//                   beta = rho' / rho, the stop test, Ctrl::it += 1, one history row
// 11 n words per system and iteration, the minimum of unpipelined CG; q is never rewritten (the eps2 term is
// formed on the fly, twice).
//
// Vectors are in T; every sum and every scalar is fp64, scalars are rounded to T where they multiply a vector.
// Reductions: per-workgroup partials (block_sum) into partials[j][blockIdx.x], then a finalising launch sums a
// system's partials in a fixed order -- thread t adds partials t, t + 256, ... in order, then block_sum -- so the
// bits depend on n alone (not on nb, the alignment path or the run).  The finalising launches are the only
// writers of the state and of the control block and run after every reader; no float atomics.
//
// Grid: blockIdx.y = system, blockIdx.x < blocks per system = min(ceil(n / 256), PCS_CG_MAX_BLOCKS), grid-stride
// over n.  16-byte loads and stores when n sizeof(T) is a multiple of 16 and every base is 16-byte aligned,
// element-wise otherwise.  Per-element arithmetic is the same on both paths; they deal the elements to the
// threads differently, so an inexact sum may differ in its last bits between them.  A solve stays on one path.
#include "common.hpp"
#include "pds_ctrl.hpp"
#include "vecio.hpp"

namespace pcs {

constexpr int kCgThreads = 256;
constexpr int kCgCap = PCS_CG_MAX_BLOCKS;

struct CgState {
  double rho, pq, alpha, beta, tol, bnrm, active, breakdown;
};
static_assert(sizeof(CgState) == 64, "cg state layout");

inline unsigned cg_bps(int64_t n) { return grid_for(n, kCgThreads, kCgCap); }

// The launch gate: nothing is written once the loop has stopped, and never for an inactive system.
__device__ __forceinline__ bool cg_skip(const CgState* st, const Ctrl* c, int j) {
  return c->stopped != 0 || st[j].active == 0.0;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kCgThreads) void k_cg_dir(const T* __restrict__ r, T* __restrict__ p, int64_t n,
                                                       const CgState* __restrict__ st, const Ctrl* __restrict__ c) {
  const int j = blockIdx.y;
  if (cg_skip(st, c, j)) return;
  const bool first = c->it == 0;  // p holds nothing yet
  const T beta = (T)st[j].beta;
  r += (int64_t)j * n;
  p += (int64_t)j * n;
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  if constexpr (VEC) {
    constexpr int VN = V16<T>::N;
    for (int64_t i = t0; i < n / VN; i += stride) {
      V16<T> pv = ldv(r + i * VN);
      if (!first) {
        const V16<T> o = ldv(p + i * VN);
#pragma unroll
        for (int e = 0; e < VN; ++e) pv.v[e] = beta * o.v[e] + pv.v[e];
      }
      stv(p + i * VN, pv);
    }
  } else {
    for (int64_t i = t0; i < n; i += stride) p[i] = first ? r[i] : beta * p[i] + r[i];
  }
}

// partials[j][blockIdx.x] = this workgroup's share of sum p (q + eps2 p).  GATED false: pcs_cg_init's sums
// (the state is not written yet).
template <typename T, bool VEC, bool GATED>
__global__ __launch_bounds__(kCgThreads) void k_cg_dot(const T* __restrict__ p, const T* __restrict__ q, int64_t n,
                                                       T eps2, const CgState* __restrict__ st,
                                                       const Ctrl* __restrict__ c, double* __restrict__ partials) {
  __shared__ double sm[kCgThreads / kWave];
  const int j = blockIdx.y;
  if (GATED && cg_skip(st, c, j)) return;
  p += (int64_t)j * n;
  q += (int64_t)j * n;
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  double v[1] = {0.0};
  if constexpr (VEC) {
    constexpr int VN = V16<T>::N;
    for (int64_t i = t0; i < n / VN; i += stride) {
      const V16<T> pv = ldv(p + i * VN), qv = ldv(q + i * VN);
#pragma unroll
      for (int e = 0; e < VN; ++e) v[0] += (double)pv.v[e] * (double)(T)(qv.v[e] + eps2 * pv.v[e]);
    }
  } else {
    for (int64_t i = t0; i < n; i += stride) v[0] += (double)p[i] * (double)(T)(q[i] + eps2 * p[i]);
  }
  block_sum<1>(v, sm);
  if (threadIdx.x == 0) partials[(int64_t)j * gridDim.x + blockIdx.x] = v[0];
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kCgThreads) void k_cg_update(T* __restrict__ x, T* __restrict__ r,
                                                          const T* __restrict__ p, const T* __restrict__ q, int64_t n,
                                                          T eps2, const CgState* __restrict__ st,
                                                          const Ctrl* __restrict__ c, double* __restrict__ partials) {
  __shared__ double sm[kCgThreads / kWave];
  const int j = blockIdx.y;
  if (cg_skip(st, c, j)) return;
  const T alpha = (T)st[j].alpha;
  x += (int64_t)j * n;
  r += (int64_t)j * n;
  p += (int64_t)j * n;
  q += (int64_t)j * n;
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  double v[1] = {0.0};
  if constexpr (VEC) {
    constexpr int VN = V16<T>::N;
    for (int64_t i = t0; i < n / VN; i += stride) {
      const V16<T> pv = ldv(p + i * VN), qv = ldv(q + i * VN);
      V16<T> xv = ldv(x + i * VN), rv = ldv(r + i * VN);
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        const T qf = qv.v[e] + eps2 * pv.v[e];
        xv.v[e] = xv.v[e] + alpha * pv.v[e];
        rv.v[e] = rv.v[e] - alpha * qf;
        v[0] += (double)rv.v[e] * (double)rv.v[e];
      }
      stv(x + i * VN, xv);
      stv(r + i * VN, rv);
    }
  } else {
    for (int64_t i = t0; i < n; i += stride) {
      const T pi = p[i], qf = q[i] + eps2 * pi;
      x[i] = x[i] + alpha * pi;
      const T ri = r[i] - alpha * qf;
      r[i] = ri;
      v[0] += (double)ri * (double)ri;
    }
  }
  block_sum<1>(v, sm);
  if (threadIdx.x == 0) partials[(int64_t)j * gridDim.x + blockIdx.x] = v[0];
}

// ---------------------------------------------------------------- the finalising launches (one workgroup per system)

// Sum of system j's partials in the fixed order; valid in thread 0.
__device__ __forceinline__ double cg_total(const double* __restrict__ partials, int bps, int j, double* sm) {
  double v[1] = {0.0};
  for (int i = threadIdx.x; i < bps; i += blockDim.x) v[0] += partials[(int64_t)j * bps + i];
  block_sum<1>(v, sm);
  return v[0];
}

// stage 0: ||b_j|| and tol_j from sum b b; stage 1: rho_j and active_j from sum r r, every other field cleared
__global__ __launch_bounds__(kCgThreads) void k_cg_fin_init(const double* __restrict__ partials, int bps,
                                                            CgState* __restrict__ st, int stage, double rtol,
                                                            double atol) {
  __shared__ double sm[kCgThreads / kWave];
  const int j = blockIdx.x;
  const double v = cg_total(partials, bps, j, sm);
  if (threadIdx.x != 0) return;
  CgState& s = st[j];
  if (stage == 0) {
    s.bnrm = sqrt(v);
    const double t = rtol * s.bnrm;
    s.tol = atol > t ? atol : t;  // scipy _get_atol_rtol: max(atol, rtol * ||b||)
  } else {
    s.rho = v;
    s.pq = s.alpha = s.beta = s.breakdown = 0.0;
    // scipy cg: `if bnrm2 == 0: return b` and, at the head of the loop, `if norm(r) < atol: return x`
    s.active = (s.bnrm > 0.0 && !(sqrt(v) < s.tol)) ? 1.0 : 0.0;
  }
}

__global__ __launch_bounds__(kCgThreads) void k_cg_fin_dot(const double* __restrict__ partials, int bps,
                                                           CgState* __restrict__ st, const Ctrl* __restrict__ c) {
  __shared__ double sm[kCgThreads / kWave];
  const int j = blockIdx.x;
  if (cg_skip(st, c, j)) return;  // uniform
  const double pq = cg_total(partials, bps, j, sm);
  if (threadIdx.x != 0) return;
  CgState& s = st[j];
  s.pq = pq;
  if (pq > 0.0 && pq < __builtin_huge_val()) {
    s.alpha = s.rho / pq;
  } else {  // not positive or not finite: SciPy would go on with inf / NaN; this system stops here
    s.breakdown = 1.0;
    s.active = 0.0;
  }
}

// History row and loop control from the systems' state; whole workgroup, one workgroup.
__device__ __forceinline__ void cg_ctrl_step(const CgState* __restrict__ st, int nb, Ctrl* c, double* hist, bool init,
                                             int max_iter, int hist_len, double* smx, double* scnt) {
  double mx = 0.0, cnt = 0.0;
  for (int j = threadIdx.x; j < nb; j += blockDim.x) {
    const double ratio = st[j].bnrm > 0.0 ? sqrt(st[j].rho) / st[j].bnrm : 0.0;
    mx = ratio > mx || ratio != ratio ? ratio : mx;
    cnt += st[j].active;
  }
  smx[threadIdx.x] = mx;
  scnt[threadIdx.x] = cnt;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int t = 1; t < (int)blockDim.x; ++t) {
    mx = smx[t] > mx || smx[t] != smx[t] ? smx[t] : mx;
    cnt += scnt[t];
  }
  if (init) {
    c->it = 0;
    c->stopped = (cnt == 0.0 || max_iter == 0) ? 1 : 0;
    c->min_iter = 0;
    c->max_iter = max_iter;
    c->has_dual = 0;
    c->hist_len = hist_len;
    c->pend = 0;
    c->pad1 = 0;
    c->thr = 0.0;
    c->pad2 = 0.0;
    return;
  }
  const int it = c->it;
  if (2 * it + 1 < c->hist_len) {
    hist[2 * it] = mx;
    hist[2 * it + 1] = cnt;
  }
  const int nx = it + 1;
  c->it = nx;
  if (cnt == 0.0 || nx >= c->max_iter || 2 * nx + 1 >= c->hist_len) c->stopped = 1;
}

// FUSED (nb == 1, one workgroup): the control step in the same launch, after the system's state is written.
template <bool FUSED>
__global__ __launch_bounds__(kCgThreads) void k_cg_fin_update(const double* __restrict__ partials, int bps,
                                                              CgState* __restrict__ st, Ctrl* c, double* hist) {
  __shared__ double sm[kCgThreads / kWave];
  __shared__ double smx[kCgThreads], scnt[kCgThreads];
  const int j = blockIdx.x;
  if (c->stopped != 0) return;
  if (st[j].active != 0.0) {  // uniform
    const double rho_new = cg_total(partials, bps, j, sm);
    if (threadIdx.x == 0) {
      CgState& s = st[j];
      s.beta = rho_new / s.rho;
      s.rho = rho_new;
      if (sqrt(rho_new) < s.tol) s.active = 0.0;
    }
  }
  if (FUSED) {
    __syncthreads();  // thread 0's state stores, read back by the workgroup
    cg_ctrl_step(st, 1, c, hist, false, 0, 0, smx, scnt);
  }
}

__global__ __launch_bounds__(kCgThreads) void k_cg_ctrl(const CgState* __restrict__ st, int nb, Ctrl* c, double* hist,
                                                        int init, int max_iter, int hist_len) {
  __shared__ double smx[kCgThreads], scnt[kCgThreads];
  if (!init && c->stopped != 0) return;
  cg_ctrl_step(st, nb, c, hist, init != 0, max_iter, hist_len, smx, scnt);
}

inline bool cg_a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool cg_overlap(const void* a, const void* b, int64_t bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}
inline bool cg_dtype_ok(int dt) { return dt == PCS_F32 || dt == PCS_F64; }
inline bool cg_scalar_ok(double v) { return v >= 0.0 && v < __builtin_huge_val(); }
inline int64_t cg_esize(int dt) { return dt == PCS_F32 ? 4 : 8; }
// sizes every entry shares: PCS_OK, or the status to return
inline int cg_sizes(int dt, int64_t n, int64_t nb) {
  if (!cg_dtype_ok(dt) || n < 0 || nb < 1) return PCS_EINVAL;
  if (nb > 65535) return PCS_EUNSUPPORTED;
  return PCS_OK;
}

}  // namespace pcs

using namespace pcs;

#define PCS_CG_DISPATCH(dt, vec, ...)  \
  do {                                 \
    if ((dt) == PCS_F32) {             \
      using T = float;                 \
      if (vec) {                       \
        constexpr bool VEC = true;     \
        __VA_ARGS__;                   \
      } else {                         \
        constexpr bool VEC = false;    \
        __VA_ARGS__;                   \
      }                                \
    } else {                           \
      using T = double;                \
      if (vec) {                       \
        constexpr bool VEC = true;     \
        __VA_ARGS__;                   \
      } else {                         \
        constexpr bool VEC = false;    \
        __VA_ARGS__;                   \
      }                                \
    }                                  \
  } while (0)

extern "C" {

int64_t pcs_cg_state_bytes(int64_t nb) { return nb < 1 ? PCS_EINVAL : nb * (int64_t)sizeof(CgState); }

int64_t pcs_cg_nblocks(int64_t n, int64_t nb) { return (n < 0 || nb < 1) ? PCS_EINVAL : nb * (int64_t)cg_bps(n); }

int pcs_cg_init(int dt, const void* b, const void* r, int64_t n, int64_t nb, double rtol, double atol, int max_iter,
                void* state, double* partials, void* ctrl, double* hist, int hist_len, hipStream_t s) {
  const int rc = cg_sizes(dt, n, nb);
  if (rc != PCS_OK) return rc;
  if (!b || !r || !state || !partials || !ctrl || !hist || hist_len < 2 || max_iter < 0 || !cg_scalar_ok(rtol) ||
      !cg_scalar_ok(atol))
    return PCS_EINVAL;
  const unsigned bps = cg_bps(n);
  const dim3 grid(bps, (unsigned)nb);
  const bool vec = n > 0 && (n * cg_esize(dt)) % 16 == 0 && cg_a16(b) && cg_a16(r);
  CgState* st = (CgState*)state;
  PCS_CG_DISPATCH(dt, vec, k_cg_dot<T, VEC, false><<<grid, kCgThreads, 0, s>>>((const T*)b, (const T*)b, n, T(0), st,
                                                                                (const Ctrl*)ctrl, partials));
  k_cg_fin_init<<<(unsigned)nb, kCgThreads, 0, s>>>(partials, (int)bps, st, 0, rtol, atol);
  PCS_CG_DISPATCH(dt, vec, k_cg_dot<T, VEC, false><<<grid, kCgThreads, 0, s>>>((const T*)r, (const T*)r, n, T(0), st,
                                                                                (const Ctrl*)ctrl, partials));
  k_cg_fin_init<<<(unsigned)nb, kCgThreads, 0, s>>>(partials, (int)bps, st, 1, rtol, atol);
  k_cg_ctrl<<<1, kCgThreads, 0, s>>>(st, (int)nb, (Ctrl*)ctrl, hist, 1, max_iter, hist_len);
  return launch_status();
}

int pcs_cg_dir(int dt, const void* r, void* p, int64_t n, int64_t nb, const void* state, const void* ctrl,
               hipStream_t s) {
  const int rc = cg_sizes(dt, n, nb);
  if (rc != PCS_OK) return rc;
  if (!r || !p || !state || !ctrl || cg_overlap(r, p, nb * n * cg_esize(dt))) return PCS_EINVAL;
  const dim3 grid(cg_bps(n), (unsigned)nb);
  const bool vec = n > 0 && (n * cg_esize(dt)) % 16 == 0 && cg_a16(r) && cg_a16(p);
  PCS_CG_DISPATCH(dt, vec, k_cg_dir<T, VEC><<<grid, kCgThreads, 0, s>>>((const T*)r, (T*)p, n, (const CgState*)state,
                                                                         (const Ctrl*)ctrl));
  return launch_status();
}

int pcs_cg_dot(int dt, const void* p, const void* q, int64_t n, int64_t nb, double eps2, void* state, double* partials,
               const void* ctrl, hipStream_t s) {
  const int rc = cg_sizes(dt, n, nb);
  if (rc != PCS_OK) return rc;
  if (!p || !q || !state || !partials || !ctrl || !cg_scalar_ok(eps2) || cg_overlap(p, q, nb * n * cg_esize(dt)))
    return PCS_EINVAL;
  const unsigned bps = cg_bps(n);
  const dim3 grid(bps, (unsigned)nb);
  const bool vec = n > 0 && (n * cg_esize(dt)) % 16 == 0 && cg_a16(p) && cg_a16(q);
  CgState* st = (CgState*)state;
  PCS_CG_DISPATCH(dt, vec, k_cg_dot<T, VEC, true><<<grid, kCgThreads, 0, s>>>((const T*)p, (const T*)q, n, (T)eps2, st,
                                                                               (const Ctrl*)ctrl, partials));
  k_cg_fin_dot<<<(unsigned)nb, kCgThreads, 0, s>>>(partials, (int)bps, st, (const Ctrl*)ctrl);
  return launch_status();
}

int pcs_cg_update(int dt, void* x, void* r, const void* p, const void* q, int64_t n, int64_t nb, double eps2,
                  void* state, double* partials, void* ctrl, double* hist, hipStream_t s) {
  const int rc = cg_sizes(dt, n, nb);
  if (rc != PCS_OK) return rc;
  if (!x || !r || !p || !q || !state || !partials || !ctrl || !hist || !cg_scalar_ok(eps2)) return PCS_EINVAL;
  const void* v[4] = {x, r, p, q};
  for (int a = 0; a < 4; ++a)
    for (int b = a + 1; b < 4; ++b)
      if (cg_overlap(v[a], v[b], nb * n * cg_esize(dt))) return PCS_EINVAL;
  const unsigned bps = cg_bps(n);
  const dim3 grid(bps, (unsigned)nb);
  const bool vec = n > 0 && (n * cg_esize(dt)) % 16 == 0 && cg_a16(x) && cg_a16(r) && cg_a16(p) && cg_a16(q);
  CgState* st = (CgState*)state;
  PCS_CG_DISPATCH(dt, vec, k_cg_update<T, VEC><<<grid, kCgThreads, 0, s>>>((T*)x, (T*)r, (const T*)p, (const T*)q, n,
                                                                            (T)eps2, st, (const Ctrl*)ctrl, partials));
  if (nb == 1) {
    k_cg_fin_update<true><<<1, kCgThreads, 0, s>>>(partials, (int)bps, st, (Ctrl*)ctrl, hist);
  } else {
    k_cg_fin_update<false><<<(unsigned)nb, kCgThreads, 0, s>>>(partials, (int)bps, st, (Ctrl*)ctrl, hist);
    k_cg_ctrl<<<1, kCgThreads, 0, s>>>(st, (int)nb, (Ctrl*)ctrl, hist, 0, 0, 0);
  }
  return launch_status();
}

}  // extern "C"
