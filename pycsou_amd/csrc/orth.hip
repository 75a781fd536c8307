// Re-orthogonalisation of one Lanczos step against a stored fp64 basis: the vector work between two applications of
// the operator in the thick-restart Lanczos behind LinearOperator.eigenvals / singularvals (pycsou/core/linop.py:
// 208-219 -> scipy.sparse.linalg.eigsh / svds -> ARPACK dsaupd, whose dsaitr re-orthogonalises on the host).
//
// V: m + 1 rows of n doubles, row stride ldv >= n.  At step s rows 0..s are orthonormal and w = A V_s.  Classical
// Gram-Schmidt, twice (CGS2):
//   pcs_orth_dots     h1[i] = <V_i, w> (i <= s), h1[s+1] = <w, w>                          reads (s + 1) n + n/group
//   pcs_orth_update   w -= sum_i h1[i] V_i;  h2[i] = <V_i, w>, h2[s+1] = <w, w>            reads (s + 1) n up to 24 rows
//                                                                                          (twice that above), writes n
//   pcs_orth_update   w -= sum_i h2[i] V_i;  h3 likewise (what is left: the orthogonality figure)
//   pcs_orth_commit   H[:, s] = H[s, :] = h1 + h2, beta_s = sqrt(h3[s+1]), omega_s = max |h3[i]| / beta_s,
//                     V_{s+1} = w / beta_s (zeros on a breakdown)
//
// k_orth_dots: blockIdx.y = a group of kOrthG rows, blockIdx.x a share of the columns (grid-stride): a thread loads
// its elements of w once and multiplies them into the kOrthG rows of the group, one fp64 accumulator per row.
// k_orth_update: blockIdx.x a share of the columns.  Phase 1 forms w_new on the thread's elements (the rows in the
// order 0..s, one fma each) and stores it; phase 2 runs the row groups over the same elements, reading back the
// thread's own w_new and the rows a second time (from whatever cache level still holds them), and reduces each group
// across the workgroup.  FUSED false is phase 1 alone (the separate axpy of the A/B in tools/bench_spectral.py).
// k_orth_update_reg serves s + 1 <= PCS_ORTH_REG_ROWS: no second read, the rows stay in registers (reads (s + 1) n).
//
// Sums: per-workgroup partials[row][blockIdx.x] (block_sum), then k_orth_fin adds a row's partials in a fixed order
// -- thread t takes partials t, t + 256, ... in order, then block_sum.  No atomics: the bits depend on n, s and the
// access path alone (16-byte loads when V, w are 16-byte aligned and ldv is even; element-wise otherwise; an odd n
// leaves one tail element to thread 0 of workgroup 0 on the 16-byte path).
#include "common.hpp"

namespace pcs {

constexpr int kOrthThreads = 256;
constexpr int kOrthG = PCS_ORTH_GROUP;
constexpr int kOrthCap = PCS_ORTH_MAX_BLOCKS;
constexpr int kOrthTile = 2 * kOrthThreads;  // columns of one workgroup and grid-stride pass on the 16-byte path

inline unsigned orth_bps(int64_t n) { return grid_for(n, kOrthTile, kOrthCap); }

struct D2 {
  double x, y;
};
__device__ __forceinline__ D2 ld2(const double* p) {
  const double2 v = *reinterpret_cast<const double2*>(p);
  return D2{v.x, v.y};
}
__device__ __forceinline__ void st2(double* p, D2 v) { *reinterpret_cast<double2*>(p) = make_double2(v.x, v.y); }

// acc[g] += <row min(g, ng - 1) of the group, w> on this thread's elements (rows past the group re-read its last
// row: no divergent loads, their sums are dropped); acc[kOrthG] += <w, w>
template <bool VEC>
__device__ __forceinline__ void orth_group_dots(const double* __restrict__ Vg, int64_t ldv, int ng,
                                                const double* w, int64_t n, double (&acc)[kOrthG + 1]) {
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  int64_t off[kOrthG];
#pragma unroll
  for (int g = 0; g < kOrthG; ++g) off[g] = (int64_t)(g < ng ? g : ng - 1) * ldv;
  if constexpr (VEC) {
    for (int64_t i = t0; i < (n >> 1); i += stride) {
      const D2 wv = ld2(w + 2 * i);
      D2 v[kOrthG];
#pragma unroll
      for (int g = 0; g < kOrthG; ++g) v[g] = ld2(Vg + off[g] + 2 * i);
#pragma unroll
      for (int g = 0; g < kOrthG; ++g) acc[g] = pcs_fma(v[g].y, wv.y, pcs_fma(v[g].x, wv.x, acc[g]));
      acc[kOrthG] = pcs_fma(wv.y, wv.y, pcs_fma(wv.x, wv.x, acc[kOrthG]));
    }
  }
  // element-wise: the whole vector, or the tail element of an odd n
  const int64_t e0 = VEC ? ((n & 1) && t0 == 0 ? n - 1 : n) : t0;
  for (int64_t i = e0; i < n; i += stride) {
    const double wv = w[i];
#pragma unroll
    for (int g = 0; g < kOrthG; ++g) acc[g] = pcs_fma(Vg[off[g] + i], wv, acc[g]);
    acc[kOrthG] = pcs_fma(wv, wv, acc[kOrthG]);
  }
}

// partials[(r0 + g) bps + blockIdx.x] for the rows of the group; the <w, w> row s + 1 from group 0
__device__ __forceinline__ void orth_group_store(double (&acc)[kOrthG + 1], double* sm, int r0, int ng, int s,
                                                 bool ww, double* __restrict__ partials) {
  block_sum<kOrthG + 1>(acc, sm);
  if (threadIdx.x != 0) return;
  const int64_t bps = gridDim.x;
#pragma unroll
  for (int g = 0; g < kOrthG; ++g)
    if (g < ng) partials[(int64_t)(r0 + g) * bps + blockIdx.x] = acc[g];
  if (ww) partials[(int64_t)(s + 1) * bps + blockIdx.x] = acc[kOrthG];
}

template <bool VEC>
__global__ __launch_bounds__(kOrthThreads) void k_orth_dots(const double* __restrict__ V, int64_t ldv, int s,
                                                            const double* __restrict__ w, int64_t n,
                                                            double* __restrict__ partials) {
  __shared__ double sm[(kOrthG + 1) * (kOrthThreads / kWave)];
  const int r0 = blockIdx.y * kOrthG;
  const int ng = s + 1 - r0 < kOrthG ? s + 1 - r0 : kOrthG;
  double acc[kOrthG + 1];
#pragma unroll
  for (int g = 0; g <= kOrthG; ++g) acc[g] = 0.0;
  orth_group_dots<VEC>(V + (int64_t)r0 * ldv, ldv, ng, w, n, acc);
  orth_group_store(acc, sm, r0, ng, s, blockIdx.y == 0, partials);
}

template <bool VEC, bool FUSED>
__global__ __launch_bounds__(kOrthThreads) void k_orth_update(const double* __restrict__ V, int64_t ldv, int s,
                                                              double* w, int64_t n, const double* __restrict__ h_in,
                                                              double* __restrict__ partials) {
  __shared__ double sh[PCS_ORTH_MAX_M];
  __shared__ double sm[(kOrthG + 1) * (kOrthThreads / kWave)];
  for (int i = threadIdx.x; i <= s; i += kOrthThreads) sh[i] = h_in[i];
  __syncthreads();
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  // phase 1: w_new = w - sum_r h[r] V_r, rows in order
  if constexpr (VEC) {
    for (int64_t i = t0; i < (n >> 1); i += stride) {
      D2 a = ld2(w + 2 * i);
      const double* p = V + 2 * i;
#pragma unroll 4
      for (int r = 0; r <= s; ++r) {
        const D2 v = ld2(p + (int64_t)r * ldv);
        const double c = -sh[r];
        a.x = pcs_fma(c, v.x, a.x);
        a.y = pcs_fma(c, v.y, a.y);
      }
      st2(w + 2 * i, a);
    }
  }
  const int64_t e0 = VEC ? ((n & 1) && t0 == 0 ? n - 1 : n) : t0;
  for (int64_t i = e0; i < n; i += stride) {
    double a = w[i];
#pragma unroll 4
    for (int r = 0; r <= s; ++r) a = pcs_fma(-sh[r], V[(int64_t)r * ldv + i], a);
    w[i] = a;
  }
  if constexpr (FUSED) {
    // phase 2: each thread reads back the elements of w it stored itself (program order, no fence needed)
    for (int r0 = 0; r0 <= s; r0 += kOrthG) {
      const int ng = s + 1 - r0 < kOrthG ? s + 1 - r0 : kOrthG;
      double acc[kOrthG + 1];
#pragma unroll
      for (int g = 0; g <= kOrthG; ++g) acc[g] = 0.0;
      orth_group_dots<VEC>(V + (int64_t)r0 * ldv, ldv, ng, w, n, acc);
      orth_group_store(acc, sm, r0, ng, s, r0 == 0, partials);
    }
  }
}

// s + 1 <= R rows: the thread's elements of every row stay in registers between the axpy and the dots, so the basis
// is read once.  Rows past s re-read row s with a zero coefficient (sh[r] = 0); their sums are dropped.
template <bool VEC, int R>
__global__ __launch_bounds__(kOrthThreads) void k_orth_update_reg(const double* __restrict__ V, int64_t ldv, int s,
                                                                  double* w, int64_t n,
                                                                  const double* __restrict__ h_in,
                                                                  double* __restrict__ partials) {
  __shared__ double sh[R];
  __shared__ double sm[(R + 1) * (kOrthThreads / kWave)];
  if (threadIdx.x < R) sh[threadIdx.x] = (int)threadIdx.x <= s ? -h_in[threadIdx.x] : 0.0;
  __syncthreads();
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  double acc[R + 1];
#pragma unroll
  for (int r = 0; r <= R; ++r) acc[r] = 0.0;
  if constexpr (VEC) {
    for (int64_t i = t0; i < (n >> 1); i += stride) {
      D2 a = ld2(w + 2 * i);
      D2 v[R];
      const double* p = V + 2 * i;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        v[r] = ld2(p);
        p += r < s ? ldv : 0;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double c = sh[r];
        a.x = pcs_fma(c, v[r].x, a.x);
        a.y = pcs_fma(c, v[r].y, a.y);
      }
      st2(w + 2 * i, a);
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = pcs_fma(v[r].y, a.y, pcs_fma(v[r].x, a.x, acc[r]));
      acc[R] = pcs_fma(a.y, a.y, pcs_fma(a.x, a.x, acc[R]));
    }
  }
  // 16-byte path, odd n: thread 0 of workgroup 0 forms the last element of w_new here (a rolled loop, no second
  // copy of the unrolled body) and adds its products after the workgroup's sums, below
  double tail = 0.0;
  bool has_tail = false;
  if constexpr (VEC) {
    has_tail = (n & 1) && t0 == 0;
    if (has_tail) {
      tail = w[n - 1];
#pragma unroll 1
      for (int r = 0; r <= s; ++r) tail = pcs_fma(sh[r], V[(int64_t)r * ldv + n - 1], tail);
      w[n - 1] = tail;
    }
  } else {
    for (int64_t i = t0; i < n; i += stride) {
      double a = w[i];
      double v[R];
      const double* p = V + i;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        v[r] = p[0];
        p += r < s ? ldv : 0;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) a = pcs_fma(sh[r], v[r], a);
      w[i] = a;
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = pcs_fma(v[r], a, acc[r]);
      acc[R] = pcs_fma(a, a, acc[R]);
    }
  }
  block_sum<R + 1>(acc, sm);
  if (threadIdx.x != 0) return;
  const int64_t bps = gridDim.x;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r > s) continue;
    const double t = has_tail ? pcs_fma(V[(int64_t)r * ldv + n - 1], tail, acc[r]) : acc[r];
    partials[(int64_t)r * bps + blockIdx.x] = t;
  }
  partials[(int64_t)(s + 1) * bps + blockIdx.x] = has_tail ? pcs_fma(tail, tail, acc[R]) : acc[R];
}

// h[j] = the sum of row j's partials in the fixed order
__global__ __launch_bounds__(kOrthThreads) void k_orth_fin(const double* __restrict__ partials, int bps,
                                                           double* __restrict__ h) {
  __shared__ double sm[kOrthThreads / kWave];
  const int j = blockIdx.x;
  double v[1] = {0.0};
  for (int i = threadIdx.x; i < bps; i += blockDim.x) v[0] += partials[(int64_t)j * bps + i];
  block_sum<1>(v, sm);
  if (threadIdx.x == 0) h[j] = v[0];
}

// state: H (m x m, row-major), beta[m], omega[m], breakdown (the first step that broke down as a double, -1: none)
__global__ __launch_bounds__(kOrthThreads) void k_orth_state_init(double* __restrict__ state, int m) {
  const int64_t len = (int64_t)m * m + 2 * m + 1;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x)
    state[i] = i == len - 1 ? -1.0 : 0.0;
}

__global__ __launch_bounds__(kOrthThreads) void k_orth_commit(int s, int m, const double* __restrict__ h1,
                                                              const double* __restrict__ h2,
                                                              const double* __restrict__ h3, double brk,
                                                              double* __restrict__ state) {
  __shared__ double smx[kOrthThreads];
  double* H = state;
  double* beta = state + (int64_t)m * m;
  double* omega = beta + m;
  double* broke_at = omega + m;
  double mx = 0.0;
  for (int i = threadIdx.x; i <= s; i += kOrthThreads) {
    const double c = h1[i] + h2[i];
    H[(int64_t)i * m + s] = c;
    H[(int64_t)s * m + i] = c;
    const double a = fabs(h3[i]);
    mx = a > mx || a != a ? a : mx;
  }
  smx[threadIdx.x] = mx;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int t = 1; t < kOrthThreads; ++t) mx = smx[t] > mx || smx[t] != smx[t] ? smx[t] : mx;
  const double b = sqrt(h3[s + 1]), before = sqrt(h1[s + 1]);
  const bool broke = b <= brk * before;  // an invariant subspace or a zero vector; 0 <= 0 on an inert step
  beta[s] = broke ? 0.0 : b;
  omega[s] = broke ? 0.0 : mx / b;
  if (broke && broke_at[0] < 0.0) broke_at[0] = (double)s;
}

// V_{s+1} = w / beta_s, zeros when beta_s == 0 (k_orth_commit's mark of a breakdown)
template <bool VEC>
__global__ __launch_bounds__(kOrthThreads) void k_orth_row(double* __restrict__ row, const double* __restrict__ w,
                                                           int64_t n, const double* __restrict__ beta_s) {
  const double b = beta_s[0];
  const bool zero = b == 0.0;
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  if constexpr (VEC) {
    for (int64_t i = t0; i < (n >> 1); i += stride) {
      D2 v = D2{0.0, 0.0};
      if (!zero) {
        v = ld2(w + 2 * i);
        v.x /= b;
        v.y /= b;
      }
      st2(row + 2 * i, v);
    }
  }
  const int64_t e0 = VEC ? ((n & 1) && t0 == 0 ? n - 1 : n) : t0;
  for (int64_t i = e0; i < n; i += stride) row[i] = zero ? 0.0 : w[i] / b;
}

inline bool orth_a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool orth_vec(const void* V, int64_t ldv, const void* w) { return orth_a16(V) && orth_a16(w) && ldv % 2 == 0; }
// w against rows 0..s+1 of V
inline bool orth_overlap(const double* V, int64_t ldv, int s, const double* w, int64_t n) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(V), b = reinterpret_cast<uintptr_t>(w);
  const uintptr_t va = ((uintptr_t)(s + 1) * (uintptr_t)ldv + (uintptr_t)n) * 8u, wb = (uintptr_t)n * 8u;
  return a < b + wb && b < a + va;
}
// PCS_OK, or the status every entry returns for these sizes
inline int orth_sizes(const double* V, int64_t ldv, int64_t s, const double* w, int64_t n) {
  if (!V || !w || n < 0 || s < 0 || ldv < n) return PCS_EINVAL;
  if (s >= PCS_ORTH_MAX_M) return PCS_EUNSUPPORTED;
  if (orth_overlap(V, ldv, (int)s, w, n)) return PCS_EINVAL;
  return PCS_OK;
}
// diagnostics (the A/B of tools/bench_spectral.py): PCS_ORTH_SPLIT=1 runs the update as axpy, then dots; read at
// every call, so one process can alternate the two forms
inline bool orth_split() { return env_override("PCS_ORTH_SPLIT", 0) == 1; }

}  // namespace pcs

using namespace pcs;

extern "C" {

int64_t pcs_orth_state_bytes(int64_t m) {
  if (m < 1) return PCS_EINVAL;
  if (m > PCS_ORTH_MAX_M) return PCS_EUNSUPPORTED;
  return (m * m + 2 * m + 1) * (int64_t)sizeof(double);
}

int64_t pcs_orth_nblocks(int64_t n, int64_t rows) {
  if (n < 0 || rows < 1) return PCS_EINVAL;
  if (rows > PCS_ORTH_MAX_M) return PCS_EUNSUPPORTED;
  return (rows + 1) * (int64_t)orth_bps(n);
}

int pcs_orth_state_init(void* state, int64_t m, hipStream_t st) {
  if (!state || m < 1) return PCS_EINVAL;
  if (m > PCS_ORTH_MAX_M) return PCS_EUNSUPPORTED;
  k_orth_state_init<<<grid_for(m * m + 2 * m + 1, kOrthThreads, 64), kOrthThreads, 0, st>>>((double*)state, (int)m);
  return launch_status();
}

int pcs_orth_dots(const double* V, int64_t ldv, int64_t s, const double* w, int64_t n, double* h, double* partials,
                  hipStream_t st) {
  const int rc = orth_sizes(V, ldv, s, w, n);
  if (rc != PCS_OK) return rc;
  if (!h || !partials) return PCS_EINVAL;
  const unsigned bps = orth_bps(n);
  const dim3 grid(bps, (unsigned)((s + kOrthG) / kOrthG));
  if (orth_vec(V, ldv, w))
    k_orth_dots<true><<<grid, kOrthThreads, 0, st>>>(V, ldv, (int)s, w, n, partials);
  else
    k_orth_dots<false><<<grid, kOrthThreads, 0, st>>>(V, ldv, (int)s, w, n, partials);
  k_orth_fin<<<(unsigned)(s + 2), kOrthThreads, 0, st>>>(partials, (int)bps, h);
  return launch_status();
}

int pcs_orth_update(const double* V, int64_t ldv, int64_t s, double* w, int64_t n, const double* h_in, double* h_out,
                    double* partials, hipStream_t st) {
  const int rc = orth_sizes(V, ldv, s, w, n);
  if (rc != PCS_OK) return rc;
  if (!h_in || !h_out || !partials || h_in == h_out) return PCS_EINVAL;
  const unsigned bps = orth_bps(n);
  const bool vec = orth_vec(V, ldv, w);
  if (orth_split()) {
    const dim3 grid(bps, (unsigned)((s + kOrthG) / kOrthG));
    if (vec) {
      k_orth_update<true, false><<<bps, kOrthThreads, 0, st>>>(V, ldv, (int)s, w, n, h_in, partials);
      k_orth_dots<true><<<grid, kOrthThreads, 0, st>>>(V, ldv, (int)s, w, n, partials);
    } else {
      k_orth_update<false, false><<<bps, kOrthThreads, 0, st>>>(V, ldv, (int)s, w, n, h_in, partials);
      k_orth_dots<false><<<grid, kOrthThreads, 0, st>>>(V, ldv, (int)s, w, n, partials);
    }
  } else if (s < PCS_ORTH_REG_ROWS) {
    const int bucket = (int)s / 8;  // the instantiation that holds s + 1 rows: 8, 16 or 24
#define PCS_ORTH_REG(R)                                                                                  \
  do {                                                                                                   \
    if (vec)                                                                                             \
      k_orth_update_reg<true, R><<<bps, kOrthThreads, 0, st>>>(V, ldv, (int)s, w, n, h_in, partials);   \
    else                                                                                                 \
      k_orth_update_reg<false, R><<<bps, kOrthThreads, 0, st>>>(V, ldv, (int)s, w, n, h_in, partials);  \
  } while (0)
    if (bucket == 0)
      PCS_ORTH_REG(8);
    else if (bucket == 1)
      PCS_ORTH_REG(16);
    else
      PCS_ORTH_REG(24);
#undef PCS_ORTH_REG
  } else if (vec) {
    k_orth_update<true, true><<<bps, kOrthThreads, 0, st>>>(V, ldv, (int)s, w, n, h_in, partials);
  } else {
    k_orth_update<false, true><<<bps, kOrthThreads, 0, st>>>(V, ldv, (int)s, w, n, h_in, partials);
  }
  k_orth_fin<<<(unsigned)(s + 2), kOrthThreads, 0, st>>>(partials, (int)bps, h_out);
  return launch_status();
}

int pcs_orth_commit(double* V, int64_t ldv, int64_t s, int64_t m, const double* w, int64_t n, const double* h1,
                    const double* h2, const double* h3, double brk, void* state, hipStream_t st) {
  if (!V || !w || !h1 || !h2 || !h3 || !state || n < 0 || m < 1 || s < 0 || s >= m || ldv < n || !(brk >= 0.0) ||
      brk == __builtin_huge_val())
    return PCS_EINVAL;
  if (m > PCS_ORTH_MAX_M) return PCS_EUNSUPPORTED;
  if (orth_overlap(V, ldv, (int)s, w, n)) return PCS_EINVAL;
  double* stt = (double*)state;
  k_orth_commit<<<1, kOrthThreads, 0, st>>>((int)s, (int)m, h1, h2, h3, brk, stt);
  double* row = V + (s + 1) * ldv;
  const double* beta_s = stt + m * m + s;
  if (orth_vec(V, ldv, w))
    k_orth_row<true><<<orth_bps(n), kOrthThreads, 0, st>>>(row, w, n, beta_s);
  else
    k_orth_row<false><<<orth_bps(n), kOrthThreads, 0, st>>>(row, w, n, beta_s);
  return launch_status();
}

}  // extern "C"
