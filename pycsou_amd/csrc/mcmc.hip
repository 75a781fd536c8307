// Proximal MYULA sampler (pycsou/opt/mcmc.py) and P-square streaming quantiles (pycsou/util/stats.py).
//
//   pcs_myula_step       one Langevin step in one launch, the noise from a buffer or generated in registers
//   pcs_mcmc_accumulate  one retained sample: running sum, running sum of squares, K P2 states, and the two
//                        fp64 sums of the reference's diagnostic, reading x once
//   pcs_p2_update        the P2 path alone (P2Algorithm)
//   pcs_mcmc_normal / pcs_mcmc_philox   the step's noise / its raw words into a buffer
//
// P2 state, structure of arrays so that lanes coalesce (n = number of pixels, K <= PCS_P2_MAX_K p-values):
//   heights[K][5][n]  in the data dtype, ascending over the middle index
//   pos[K][3][n]      int32 positions of markers 1..3; marker 0 is always at 1 and marker 4 at `count`, the
//                     number of samples seen, which the host passes by value
// The desired positions (5 doubles per p-value) are accumulated on the host by repeated addition, as
// P2Algorithm.add_sample does, and passed by value.  The element update and the noise mapping are in
// mcmc_core.hpp.  This file is built with -ffp-contract=off: the running sums add a rounded x^2 and the
// step adds rounded products, as NumPy does.
#include "common.hpp"
#include "mcmc_core.hpp"

namespace pcs {

constexpr int kMcmcBlocks = 1024;  // partials: 2 doubles per block, within pcs_reduce_ws_bytes()

struct P2Des {
  double d[PCS_P2_MAX_K][5];
};

// V elements of T (16 bytes when V > 1) between memory and registers
template <typename T, int V>
__device__ __forceinline__ void ldn(const T* p, T (&r)[V]) {
  if constexpr (V == 1) r[0] = *p;
  else __builtin_memcpy(r, __builtin_assume_aligned(p, sizeof(T) * V), sizeof(T) * V);
}
template <typename T, int V>
__device__ __forceinline__ void stn(T* p, const T (&r)[V]) {
  if constexpr (V == 1) *p = r[0];
  else __builtin_memcpy(__builtin_assume_aligned(p, sizeof(T) * V), r, sizeof(T) * V);
}

// One retained sample.  V = 16 / sizeof(T) elements per lane when n % V == 0 and every array is 16-B
// aligned (every row of the state then is), else V = 1.  ACC: with the running sums and the diagnostic.
template <typename T, int V, bool ACC>
__global__ __launch_bounds__(256) void k_mcmc_acc(const T* __restrict__ x, T* __restrict__ sum,
                                                  T* __restrict__ sumsq, T* __restrict__ hts,
                                                  int32_t* __restrict__ pos, int64_t n, int K, int64_t count,
                                                  P2Des des, double* __restrict__ part) {
  double v[2] = {0.0, 0.0};
  const int64_t ng = n / V;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < ng; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = g * V;
    T xv[V];
    ldn<T, V>(x + e, xv);
    if constexpr (ACC) {
      T s[V], s2[V];
      ldn<T, V>(sum + e, s);
      ldn<T, V>(sumsq + e, s2);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        v[0] += (double)xv[j] * (double)xv[j];
        v[1] += (double)s[j] * (double)s[j];
        s[j] += xv[j];
        s2[j] += xv[j] * xv[j];
      }
      stn<T, V>(sum + e, s);
      stn<T, V>(sumsq + e, s2);
    }
    for (int k = 0; k < K; ++k) {
      T* hk = hts + (int64_t)k * 5 * n + e;
      int32_t* pk = pos + (int64_t)k * 3 * n + e;
      T h[5][V];
      int32_t p[3][V];
#pragma unroll
      for (int m = 0; m < 5; ++m) ldn<T, V>(hk + m * n, h[m]);
#pragma unroll
      for (int m = 0; m < 3; ++m) ldn<int32_t, V>(pk + m * n, p[m]);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        T q[5] = {h[0][j], h[1][j], h[2][j], h[3][j], h[4][j]};
        int nn[5] = {1, p[0][j], p[1][j], p[2][j], (int)(count - 1)};
        p2_add_el<T>(xv[j], q, nn, count, des.d[k]);
#pragma unroll
        for (int m = 0; m < 5; ++m) h[m][j] = q[m];
#pragma unroll
        for (int m = 0; m < 3; ++m) p[m][j] = nn[m + 1];
      }
#pragma unroll
      for (int m = 0; m < 5; ++m) stn<T, V>(hk + m * n, h[m]);
#pragma unroll
      for (int m = 0; m < 3; ++m) stn<int32_t, V>(pk + m * n, p[m]);
    }
  }
  if constexpr (ACC) {
    __shared__ double sm[8];
    block_sum<2>(v, sm);
    if (threadIdx.x == 0) {
      part[2 * blockIdx.x] = v[0];
      part[2 * blockIdx.x + 1] = v[1];
    }
  }
}

// stage 2 of the diagnostic: fixed order, no atomics
__global__ __launch_bounds__(256) void k_mcmc_sums(const double* __restrict__ part, int np, double* __restrict__ out) {
  __shared__ double sm[8];
  double v[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < np; i += blockDim.x) {
    v[0] += part[2 * i];
    v[1] += part[2 * i + 1];
  }
  block_sum<2>(v, sm);
  if (threadIdx.x == 0) {
    out[0] = v[0];
    out[1] = v[1];
  }
}

// four consecutive elements, as 16-B accesses (VEC) or one by one
template <typename T, bool VEC>
__device__ __forceinline__ void ld4(const T* p, T (&r)[4]) {
  if constexpr (VEC) {
    constexpr int H = 16 / sizeof(T);
#pragma unroll
    for (int h = 0; h < 4 / H; ++h) __builtin_memcpy(r + h * H, __builtin_assume_aligned(p + h * H, 16), 16);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = p[j];
  }
}
template <typename T, bool VEC>
__device__ __forceinline__ void st4(T* p, const T (&r)[4]) {
  if constexpr (VEC) {
    constexpr int H = 16 / sizeof(T);
#pragma unroll
    for (int h = 0; h < 4 / H; ++h) __builtin_memcpy(__builtin_assume_aligned(p + h * H, 16), r + h * H, 16);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = r[j];
  }
}

struct MyulaPar {
  double a, gam, b, c;  // 1 - gamma / tau, gamma, gamma / tau, sqrt(2 gamma)
  double thr, sa, sb;   // tau * lam, segment
  int pmode, gk;
  uint64_t seed;
  uint32_t iter, stream;
};

template <typename T>
__device__ __forceinline__ T myula_el(T x, T g, T p, T z, int pmode, int gk, T a, T gam, T b, T c, T thr, T sa,
                                      T sb) {
  if (pmode == PCS_MYULA_P_NONE) return (x - gam * g) + c * z;  // mcmc.py:114
  if (pmode == PCS_MYULA_P_KIND) {                              // G.prox(x, tau)
    p = x;
    if (gk == PCS_APGD_G_L1) p = x - thr * clip1(x / thr);
    else if (gk == PCS_G_NONNEG) p = (x < T(0)) ? T(0) : x;
    else if (gk == PCS_G_SEGMENT) {
      p = (x < sa) ? sa : x;
      p = (p > sb) ? sb : p;
    }
  }
  return ((a * x - gam * g) + b * p) + c * z;  // mcmc.py:116-118, left to right
}

// One lane per block of four elements (one Philox block); the last block may be partial.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_myula_step(const T* __restrict__ x, const T* __restrict__ g,
                                                    const T* __restrict__ pb, const T* __restrict__ zb,
                                                    T* __restrict__ xn, int64_t n, MyulaPar q) {
  const T a = (T)q.a, gam = (T)q.gam, b = (T)q.b, c = (T)q.c, thr = (T)q.thr, sa = (T)q.sa, sb = (T)q.sb;
  const int64_t nb = (n + 3) / 4;
  for (int64_t blk = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; blk < nb;
       blk += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = blk * 4;
    T xv[4], gv[4], pv[4] = {T(0), T(0), T(0), T(0)}, zv[4], o[4];
    if (!zb) {
      float zf[4];
      mcmc_normal4(q.seed, q.iter, q.stream, (uint64_t)blk, zf);
#pragma unroll
      for (int j = 0; j < 4; ++j) zv[j] = (T)zf[j];
    }
    if (e + 4 <= n) {
      ld4<T, VEC>(x + e, xv);
      ld4<T, VEC>(g + e, gv);
      if (q.pmode == PCS_MYULA_P_BUF) ld4<T, VEC>(pb + e, pv);
      if (zb) ld4<T, VEC>(zb + e, zv);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = myula_el<T>(xv[j], gv[j], pv[j], zv[j], q.pmode, q.gk, a, gam, b, c, thr, sa, sb);
      st4<T, VEC>(xn + e, o);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (e + j < n) {
          const T pj = q.pmode == PCS_MYULA_P_BUF ? pb[e + j] : T(0);
          const T zj = zb ? zb[e + j] : zv[j];
          xn[e + j] = myula_el<T>(x[e + j], g[e + j], pj, zj, q.pmode, q.gk, a, gam, b, c, thr, sa, sb);
        }
      }
    }
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_mcmc_normal(T* __restrict__ out, int64_t n, uint64_t seed, uint32_t iter,
                                                     uint32_t stream) {
  const int64_t nb = (n + 3) / 4;
  for (int64_t blk = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; blk < nb;
       blk += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = blk * 4;
    float zf[4];
    mcmc_normal4(seed, iter, stream, (uint64_t)blk, zf);
    T o[4] = {(T)zf[0], (T)zf[1], (T)zf[2], (T)zf[3]};
    if (e + 4 <= n) {
      st4<T, VEC>(out + e, o);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n) out[e + j] = o[j];
    }
  }
}

__global__ __launch_bounds__(256) void k_mcmc_philox(uint32_t* __restrict__ out, int64_t nb, uint64_t seed,
                                                     uint32_t iter, uint32_t stream) {
  for (int64_t blk = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; blk < nb;
       blk += (int64_t)gridDim.x * blockDim.x) {
    uint32_t w[4];
    mcmc_words(seed, iter, stream, (uint64_t)blk, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[4 * blk + j] = w[j];
  }
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static bool p2_args_ok(int dt, const void* x, const void* hts, const void* pos, int64_t n, int K, int64_t count,
                       const double* des) {
  if (dt != PCS_F32 && dt != PCS_F64) return false;
  if (n < 0 || K < 0 || K > PCS_P2_MAX_K || count < 1 || count > 0x7fffffff) return false;
  if (!x || (K > 0 && (!hts || !pos || !des))) return false;
  return true;
}

template <typename T, bool ACC>
static int acc_launch(const void* x, void* sum, void* sumsq, void* hts, int32_t* pos, int64_t n, int K, int64_t count,
                      const double* des, double* sums_dev, void* ws, hipStream_t st) {
  constexpr int V = 16 / sizeof(T);
  P2Des d;
  for (int k = 0; k < PCS_P2_MAX_K; ++k)
    for (int m = 0; m < 5; ++m) d.d[k][m] = k < K ? des[5 * k + m] : 0.0;
  const bool vec = n % V == 0 && al16(x) && al16(sum) && al16(sumsq) && al16(hts) && al16(pos);
  if (vec) {
    const unsigned g = grid_for(n / V, 256, kMcmcBlocks);
    k_mcmc_acc<T, V, ACC><<<g, 256, 0, st>>>((const T*)x, (T*)sum, (T*)sumsq, (T*)hts, pos, n, K, count, d,
                                             (double*)ws);
    if (ACC) k_mcmc_sums<<<1, 256, 0, st>>>((const double*)ws, (int)g, sums_dev);
  } else {
    const unsigned g = grid_for(n, 256, kMcmcBlocks);
    k_mcmc_acc<T, 1, ACC><<<g, 256, 0, st>>>((const T*)x, (T*)sum, (T*)sumsq, (T*)hts, pos, n, K, count, d,
                                             (double*)ws);
    if (ACC) k_mcmc_sums<<<1, 256, 0, st>>>((const double*)ws, (int)g, sums_dev);
  }
  return launch_status();
}

template <typename T>
static void p2_host(const void* xv, void* hv, int32_t* pos, int64_t n, int K, int64_t count, const double* des) {
  const T* x = (const T*)xv;
  T* hts = (T*)hv;
  for (int k = 0; k < K; ++k)
    for (int64_t e = 0; e < n; ++e) {
      T* hk = hts + (int64_t)k * 5 * n + e;
      int32_t* pk = pos + (int64_t)k * 3 * n + e;
      T q[5];
      for (int m = 0; m < 5; ++m) q[m] = hk[m * n];
      int nn[5] = {1, pk[0], pk[n], pk[2 * n], (int)(count - 1)};
      p2_add_el<T>(x[e], q, nn, count, des + 5 * k);
      for (int m = 0; m < 5; ++m) hk[m * n] = q[m];
      for (int m = 0; m < 3; ++m) pk[m * n] = nn[m + 1];
    }
}

}  // namespace pcs

using namespace pcs;

extern "C" {

int pcs_p2_update(int dt, const void* x, void* heights, int32_t* pos, int64_t n, int K, int64_t count,
                  const double* desired, hipStream_t st) {
  if (!p2_args_ok(dt, x, heights, pos, n, K, count, desired) || K < 1) return PCS_EINVAL;
  if (n == 0) return PCS_OK;
  return dt == PCS_F64
             ? acc_launch<double, false>(x, nullptr, nullptr, heights, pos, n, K, count, desired, nullptr, nullptr, st)
             : acc_launch<float, false>(x, nullptr, nullptr, heights, pos, n, K, count, desired, nullptr, nullptr, st);
}

int pcs_mcmc_accumulate(int dt, const void* x, void* sum, void* sumsq, void* heights, int32_t* pos, int64_t n, int K,
                        int64_t count, const double* desired, double* sums_dev, void* ws, hipStream_t st) {
  if (!p2_args_ok(dt, x, heights, pos, n, K, count, desired) || !sum || !sumsq || !sums_dev || !ws) return PCS_EINVAL;
  if (x == sum || x == sumsq || sum == sumsq) return PCS_EINVAL;
  return dt == PCS_F64 ? acc_launch<double, true>(x, sum, sumsq, heights, pos, n, K, count, desired, sums_dev, ws, st)
                       : acc_launch<float, true>(x, sum, sumsq, heights, pos, n, K, count, desired, sums_dev, ws, st);
}

int pcs_myula_step(int dt, const void* x, const void* g, const void* p, const void* z, void* xn, int64_t n, double tau,
                   double gamma, int pmode, int gkind, double lam, double seg_a, double seg_b, uint64_t seed,
                   uint32_t iter, uint32_t stream_id, hipStream_t st) {
  if (dt != PCS_F32 && dt != PCS_F64) return PCS_EINVAL;
  if (!x || !g || !xn || n < 0 || !(gamma > 0.0)) return PCS_EINVAL;
  if (pmode != PCS_MYULA_P_NONE && pmode != PCS_MYULA_P_BUF && pmode != PCS_MYULA_P_KIND) return PCS_EINVAL;
  if (pmode != PCS_MYULA_P_NONE && !(tau > 0.0)) return PCS_EINVAL;
  if (pmode == PCS_MYULA_P_BUF && !p) return PCS_EINVAL;
  if (pmode == PCS_MYULA_P_KIND) {
    if (gkind != PCS_G_NULL && gkind != PCS_G_NONNEG && gkind != PCS_G_SEGMENT && gkind != PCS_APGD_G_L1)
      return PCS_EINVAL;
    if (gkind == PCS_APGD_G_L1 && !(tau * lam > 0)) return PCS_EINVAL;
  }
  if (xn == x || xn == g || xn == p || xn == z) return PCS_EINVAL;
  if (n == 0) return PCS_OK;
  MyulaPar q;
  const bool prox = pmode != PCS_MYULA_P_NONE;
  q.a = prox ? 1.0 - gamma / tau : 1.0;
  q.gam = gamma;
  q.b = prox ? gamma / tau : 0.0;
  q.c = sqrt(2.0 * gamma);
  q.thr = tau * lam;
  q.sa = seg_a;
  q.sb = seg_b;
  q.pmode = pmode;
  q.gk = gkind;
  q.seed = seed;
  q.iter = iter;
  q.stream = stream_id;
  const bool vec = al16(x) && al16(g) && al16(xn) && (pmode != PCS_MYULA_P_BUF || al16(p)) && (!z || al16(z));
  const unsigned gr = grid_for((n + 3) / 4, 256);
#define PCS_MYULA_GO(T)                                                                                             \
  do {                                                                                                              \
    if (vec) k_myula_step<T, true><<<gr, 256, 0, st>>>((const T*)x, (const T*)g, (const T*)p, (const T*)z, (T*)xn, n, q); \
    else k_myula_step<T, false><<<gr, 256, 0, st>>>((const T*)x, (const T*)g, (const T*)p, (const T*)z, (T*)xn, n, q);    \
  } while (0)
  if (dt == PCS_F64) PCS_MYULA_GO(double);
  else PCS_MYULA_GO(float);
#undef PCS_MYULA_GO
  return launch_status();
}

int pcs_mcmc_normal(int dt, void* out, int64_t n, uint64_t seed, uint32_t iter, uint32_t stream_id, hipStream_t st) {
  if ((dt != PCS_F32 && dt != PCS_F64) || !out || n < 0) return PCS_EINVAL;
  if (n == 0) return PCS_OK;
  const unsigned gr = grid_for((n + 3) / 4, 256);
  if (dt == PCS_F64) {
    if (al16(out)) k_mcmc_normal<double, true><<<gr, 256, 0, st>>>((double*)out, n, seed, iter, stream_id);
    else k_mcmc_normal<double, false><<<gr, 256, 0, st>>>((double*)out, n, seed, iter, stream_id);
  } else {
    if (al16(out)) k_mcmc_normal<float, true><<<gr, 256, 0, st>>>((float*)out, n, seed, iter, stream_id);
    else k_mcmc_normal<float, false><<<gr, 256, 0, st>>>((float*)out, n, seed, iter, stream_id);
  }
  return launch_status();
}

int pcs_mcmc_philox(uint32_t* out, int64_t nblocks, uint64_t seed, uint32_t iter, uint32_t stream_id,
                    hipStream_t st) {
  if (!out || nblocks < 0) return PCS_EINVAL;
  if (nblocks == 0) return PCS_OK;
  k_mcmc_philox<<<grid_for(nblocks, 256), 256, 0, st>>>(out, nblocks, seed, iter, stream_id);
  return launch_status();
}

int pcs_mcmc_philox_host(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
  if (!ctr || !key || !out) return PCS_EINVAL;
  const uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]}, k[2] = {key[0], key[1]};
  uint32_t o[4];
  philox4x32_10(c, k, o);
  for (int j = 0; j < 4; ++j) out[j] = o[j];
  return PCS_OK;
}

int pcs_mcmc_normal_host(uint64_t seed, uint32_t iter, uint32_t stream_id, int64_t n, float* out) {
  if (!out || n < 0) return PCS_EINVAL;
  for (int64_t b = 0; 4 * b < n; ++b) {
    float z[4];
    mcmc_normal4(seed, iter, stream_id, (uint64_t)b, z);
    for (int j = 0; j < 4 && 4 * b + j < n; ++j) out[4 * b + j] = z[j];
  }
  return PCS_OK;
}

int pcs_p2_update_host(int dt, const void* x, void* heights, int32_t* pos, int64_t n, int K, int64_t count,
                       const double* desired) {
  if (!p2_args_ok(dt, x, heights, pos, n, K, count, desired) || K < 1) return PCS_EINVAL;
  if (dt == PCS_F64) p2_host<double>(x, heights, pos, n, K, count, desired);
  else p2_host<float>(x, heights, pos, n, K, count, desired);
  return PCS_OK;
}

}  // extern "C"
