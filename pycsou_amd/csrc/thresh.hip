// One global threshold: the prox of L1Ball, LInftyNorm and SquaredL1Norm.
//
// Replaces the host root searches of pycsou/math/prox.py:158-164 (proj_l1_ball: brentq on
// sum max(|x| - mu, 0) = radius), pycsou/func/base.py:239-240 with proj_l1_ball (LInftyNorm.prox)
// and pycsou/func/penalty.py:296-316 (SquaredL1Norm.prox: brentq or a full sort).  All three are
//   t = 0                                          if sum |x_i| <= a
//   t > 0 with sum max(|x_i| - t, 0) = a + b t     otherwise,
// followed by a soft threshold or a clip at t.  psi(p) = sum max(|x_i| - p, 0) - a - b p is piecewise
// linear and decreasing, so t = (S_k - a) / (k + b) with S_k, k the sum and count of the |x_i| above
// the crossing.  The crossing is found in the ordered bit patterns of |x| (non-negative IEEE values
// order like their unsigned bits): a bracket [lo, hi] of keys with psi(lo) > 0 >= psi(hi) is cut into
// 32 by 31 pivots per pass until it holds two adjacent representable values; no datum then lies
// strictly inside, and {|x_i| > value(lo)} is the active set.  The first bracket is
// [(S - a) / (n + b), max |x|] (S = sum |x|), a pass evaluates the pivots only on the elements inside its
// bracket (those above it enter through their sum and count), and a pass that finds the bracket closed
// returns at once.  Every pass is a plain launch pair (per-block fp64 partials, then one block that sums
// them in a fixed order and moves the bracket in a small device state): no host read-back, no atomics, the
// same result on every run.
#include "common.hpp"

namespace pcs {

#define PCS_GRID_LOOP(p, n) \
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < (n); p += (int64_t)gridDim.x * blockDim.x)

constexpr int kThrJ = PCS_THRESH_PIVOTS;  // pivots per pass: the bracket shrinks 32-fold
constexpr int kThrRow = kThrJ + 2;        // doubles per block of a descent pass
constexpr int kThrBlocks = 1024;          // stage-1 blocks at most
constexpr int kThrStage2 = 1024;          // threads of a descent pass's stage 2 (one block)
constexpr int kThrStateDoubles = 8;       // ThreshState, padded
// passes until a bracket of width <= 2^31 (fp32 keys) / 2^63 (fp64 keys) has width <= 1
constexpr int kThrPasses32 = 7, kThrPasses64 = 13;

struct ThreshState {
  uint64_t lo, hi;  // keys: psi(value(lo)) > 0 >= psi(value(hi))
  double t;
  int32_t inside;  // sum |x| <= a: t = 0
  int32_t pad;
};
static_assert(sizeof(ThreshState) <= sizeof(double) * kThrStateDoubles, "state");

template <typename T>
struct Key;
template <>
struct Key<float> {
  static __host__ __device__ __forceinline__ uint64_t of(float v) {
    union { float f; uint32_t u; } c;
    c.f = v;
    return c.u & 0x7fffffffu;
  }
  static __host__ __device__ __forceinline__ double value(uint64_t k) {
    union { float f; uint32_t u; } c;
    c.u = (uint32_t)k;
    return (double)c.f;
  }
};
template <>
struct Key<double> {
  static __host__ __device__ __forceinline__ uint64_t of(double v) {
    union { double f; uint64_t u; } c;
    c.f = v;
    return c.u & 0x7fffffffffffffffull;
  }
  static __host__ __device__ __forceinline__ double value(uint64_t k) {
    union { double f; uint64_t u; } c;
    c.u = k;
    return c.f;
  }
};

__host__ __device__ __forceinline__ double key_value(int dt, uint64_t k) {
  return dt == PCS_F32 ? Key<float>::value(k) : Key<double>::value(k);
}

// pivot j = 0 .. J+1 of the bracket [lo, hi]: lo + j * ceil((hi - lo) / (J + 1)), at most hi
__host__ __device__ __forceinline__ uint64_t thresh_pivot(uint64_t lo, uint64_t hi, int j) {
  const uint64_t s = (hi - lo + (uint64_t)kThrJ) / (uint64_t)(kThrJ + 1);
  const uint64_t p = lo + (uint64_t)j * s;
  return (j > kThrJ || p > hi) ? hi : p;
}

__host__ __device__ __forceinline__ bool thresh_inside(double sum_abs, double a) { return sum_abs <= a; }

// Stage-2 bracket selection.  sums[j - 1] = sum max(|x| - value(pivot j), 0) for j = 1 .. J.  The new
// bracket is [pivot k - 1, pivot k] with k the first pivot at which psi <= 0 (J + 1, i.e. hi, if none).
__host__ __device__ inline void thresh_pick(int dt, uint64_t lo, uint64_t hi, const double* sums, double a, double b,
                                            uint64_t* nlo, uint64_t* nhi) {
  int k = 1;
#pragma unroll
  for (; k <= kThrJ; ++k) {
    const double psi = sums[k - 1] - a - b * key_value(dt, thresh_pivot(lo, hi, k));
    if (!(psi > 0.0)) break;
  }
  *nlo = thresh_pivot(lo, hi, k - 1);
  *nhi = thresh_pivot(lo, hi, k);
}

// f(|x[p]|) over the grid's share of x, four independent loads in flight per thread; the elements past n read
// as 0, which adds nothing to any of the sums below.  A thread's order of visits is fixed.
template <typename T, typename F>
__device__ __forceinline__ void for_each_abs(const T* __restrict__ x, int64_t n, F f) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += 4 * stride) {
    T e[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t q = p + u * stride;
      e[u] = q < n ? x[q] : T(0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) f(fabs((double)e[u]));
  }
}

__device__ __forceinline__ bool thresh_idle(const ThreshState* st) { return st->inside || st->hi - st->lo <= 1; }

// pass 0: part[2b] = sum |x|, part[2b + 1] = max |x| of block b
template <typename T>
__global__ __launch_bounds__(256) void k_thr_stats1(const T* __restrict__ x, int64_t n, double* __restrict__ part) {
  __shared__ double sm[4];
  __shared__ double smx[4];
  double v[1] = {0.0};
  double mx = 0.0;
  for_each_abs(x, n, [&](double a) {
    v[0] += a;
    mx = fmax(mx, a);
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, kWave));
  if ((threadIdx.x & 63) == 0) smx[threadIdx.x >> 6] = mx;
  block_sum<1>(v, sm);  // its barriers also publish smx
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = v[0];
    part[2 * blockIdx.x + 1] = fmax(fmax(smx[0], smx[1]), fmax(smx[2], smx[3]));
  }
}

// The first bracket.  hi = max |x| (psi <= 0 there).  lo: psi(p) >= S - a - (n + b) p, so the root is at least
// (S - a) / (n + b); the largest key below that (less a 1e-9 margin for the rounding of S), or 0.
template <typename T>
__device__ __forceinline__ uint64_t thresh_first_lo(double sum_abs, double a, double b, int64_t n, uint64_t hi) {
  const double l = (sum_abs - a) / ((double)n + b) * (1.0 - 1e-9);
  if (!(l > 0.0)) return 0;
  uint64_t k = Key<T>::of((T)l);
  if (Key<T>::value(k) > l && k > 0) --k;
  return k < hi ? k : hi;
}

template <typename T>
__global__ __launch_bounds__(256) void k_thr_stats2(const double* __restrict__ part, int np, double a, double b,
                                                    int64_t n, ThreshState* __restrict__ st) {
  __shared__ double sm[4];
  __shared__ double smx[4];
  double v[1] = {0.0};
  double mx = 0.0;
  for (int i = threadIdx.x; i < np; i += blockDim.x) {
    v[0] += part[2 * i];
    mx = fmax(mx, part[2 * i + 1]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, kWave));
  if ((threadIdx.x & 63) == 0) smx[threadIdx.x >> 6] = mx;
  block_sum<1>(v, sm);
  if (threadIdx.x == 0) {
    mx = fmax(fmax(smx[0], smx[1]), fmax(smx[2], smx[3]));
    const bool inside = thresh_inside(v[0], a);
    st->hi = Key<T>::of((T)mx);
    st->lo = inside ? 0 : thresh_first_lo<T>(v[0], a, b, n, st->hi);
    st->t = 0.0;
    st->inside = inside ? 1 : 0;
    st->pad = 0;
  }
}

// One descent pass over the bracket [lo, hi].  An element at or below value(lo) adds nothing to any pivot's
// sum; one above value(hi) adds |x| - pivot to every pivot's, which needs only the sum and the count of those
// elements; only the elements inside the bracket (1/32 of the previous pass's) take the loop over the pivots,
// which a wave skips when none of its lanes holds one.  Per block b, kThrRow doubles (row-major by quantity,
// so that stage 2 reads each row contiguously):
//   part[j - 1][b] = sum over the inside elements of max(|x| - value(pivot j), 0),  j = 1 .. J
//   part[J][b], part[J + 1][b] = sum and count of the elements above value(hi)
template <typename T>
__global__ __launch_bounds__(256) void k_thr_psi1(const T* __restrict__ x, int64_t n,
                                                  const ThreshState* __restrict__ st, double* __restrict__ part) {
  __shared__ double sm[4 * kThrRow];
  if (thresh_idle(st)) return;  // uniform: the whole grid leaves
  const uint64_t lo = st->lo, hi = st->hi;
  const double lv = Key<T>::value(lo), hv = Key<T>::value(hi);
  double pv[kThrJ], v[kThrRow];
#pragma unroll
  for (int j = 0; j < kThrJ; ++j) pv[j] = Key<T>::value(thresh_pivot(lo, hi, j + 1));
#pragma unroll
  for (int j = 0; j < kThrRow; ++j) v[j] = 0.0;
  for_each_abs(x, n, [&](double a) {
    if (a > hv) {
      v[kThrJ] += a;
      v[kThrJ + 1] += 1.0;
    } else if (a > lv) {
#pragma unroll
      for (int j = 0; j < kThrJ; ++j) {
        const double d = a - pv[j];
        v[j] += d > 0.0 ? d : 0.0;
      }
    }
  });
  block_sum<kThrRow>(v, sm);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < kThrRow; ++j) part[(int64_t)j * gridDim.x + blockIdx.x] = v[j];
  }
}

// stage 2 of a descent pass: wave w sums rows w, w + 16, ... of the partials over the blocks (lane-strided,
// then a fixed butterfly); thread 0 moves the bracket
__global__ __launch_bounds__(kThrStage2) void k_thr_psi2(int dt, const double* __restrict__ part, int np, double a,
                                                         double b, ThreshState* __restrict__ st) {
  __shared__ double sums[kThrRow];
  if (thresh_idle(st)) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int j = w; j < kThrRow; j += kThrStage2 / kWave) {
    double e[kThrBlocks / kWave];  // the row's loads all in flight, then summed in index order
#pragma unroll
    for (int u = 0; u < kThrBlocks / kWave; ++u) {
      const int i = lane + u * kWave;
      e[u] = i < np ? part[(int64_t)j * np + i] : 0.0;
    }
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < kThrBlocks / kWave; ++u) s += e[u];
    s = wave_sum(s);
    if (lane == 0) sums[j] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t nlo, nhi;
    const uint64_t lo = st->lo, hi = st->hi;
    // the elements above the bracket: sum (|x| - pivot) = S - count * pivot
    const double sa = sums[kThrJ], ca = sums[kThrJ + 1];
    double tot[kThrJ];
#pragma unroll
    for (int j = 1; j <= kThrJ; ++j) tot[j - 1] = sums[j - 1] + (sa - ca * key_value(dt, thresh_pivot(lo, hi, j)));
    thresh_pick(dt, lo, hi, tot, a, b, &nlo, &nhi);
    st->lo = nlo;
    st->hi = nhi;
  }
}

// the active set {|x| > value(lo)}: part[2b] = its sum, part[2b + 1] = its count in block b
template <typename T>
__global__ __launch_bounds__(256) void k_thr_active1(const T* __restrict__ x, int64_t n,
                                                     const ThreshState* __restrict__ st, double* __restrict__ part) {
  __shared__ double sm[8];
  if (st->inside) return;
  const double lv = Key<T>::value(st->lo);
  double v[2] = {0.0, 0.0};
  for_each_abs(x, n, [&](double a) {
    if (a > lv) {
      v[0] += a;
      v[1] += 1.0;
    }
  });
  block_sum<2>(v, sm);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = v[0];
    part[2 * blockIdx.x + 1] = v[1];
  }
}

__global__ __launch_bounds__(256) void k_thr_active2(int dt, const double* __restrict__ part, int np, double a,
                                                     double b, ThreshState* __restrict__ st,
                                                     double* __restrict__ t_dev) {
  __shared__ double sm[8];
  double v[2] = {0.0, 0.0};
  const bool inside = st->inside != 0;
  if (!inside) {
    for (int i = threadIdx.x; i < np; i += blockDim.x) {
      v[0] += part[2 * i];
      v[1] += part[2 * i + 1];
    }
  }
  block_sum<2>(v, sm);
  if (threadIdx.x == 0) {
    double t = 0.0;
    if (!inside) t = v[1] > 0.0 ? (v[0] - a) / (v[1] + b) : key_value(dt, st->hi);
    st->t = t;
    if (t_dev) *t_dev = t;
  }
}

// x and out may be the same buffer
template <typename T>
__global__ void k_thr_apply(const T* x, T* out, int64_t n, int mode, const ThreshState* __restrict__ st) {
  const double t = st->t;
  const bool inside = st->inside != 0;
  PCS_GRID_LOOP(p, n) {
    const T xv = x[p];
    T r;
    if (mode == PCS_THRESH_SOFT) {
      // sign(x) max(|x| - t, 0), formed in fp64 and rounded once (math/prox.py:114)
      r = inside ? xv : (T)copysign(fmax(fabs((double)xv) - t, 0.0), (double)xv);
    } else {
      r = inside ? T(0) : (T)fmin(fmax((double)xv, -t), t);
    }
    out[p] = r;
  }
}

template <typename T>
static int thresh_l1(const void* x, void* out, int64_t n, double a, double b, int mode, double* t_dev, void* ws,
                     hipStream_t st) {
  ThreshState* state = (ThreshState*)ws;
  double* part = (double*)ws + kThrStateDoubles;
  const int dt = sizeof(T) == 4 ? PCS_F32 : PCS_F64;
  const unsigned g = grid_for(n, 256, kThrBlocks);
  k_thr_stats1<T><<<g, 256, 0, st>>>((const T*)x, n, part);
  k_thr_stats2<T><<<1, 256, 0, st>>>(part, (int)g, a, b, n, state);
  const int passes = sizeof(T) == 4 ? kThrPasses32 : kThrPasses64;
  for (int i = 0; i < passes; ++i) {
    k_thr_psi1<T><<<g, 256, 0, st>>>((const T*)x, n, state, part);
    k_thr_psi2<<<1, kThrStage2, 0, st>>>(dt, part, (int)g, a, b, state);
  }
  k_thr_active1<T><<<g, 256, 0, st>>>((const T*)x, n, state, part);
  k_thr_active2<<<1, 256, 0, st>>>(dt, part, (int)g, a, b, state, t_dev);
  k_thr_apply<T><<<grid_for(n, 256), 256, 0, st>>>((const T*)x, (T*)out, n, mode, state);
  return launch_status();
}

}  // namespace pcs

using namespace pcs;

extern "C" {

int64_t pcs_thresh_ws_bytes(int64_t n) {
  if (n < 0) return PCS_EINVAL;
  return (int64_t)sizeof(double) * (kThrStateDoubles + (int64_t)kThrRow * grid_for(n, 256, kThrBlocks));
}

int pcs_thresh_l1(int dt, const void* x, void* out, int64_t n, double a, double b, int mode, double* t_dev, void* ws,
                  hipStream_t st) {
  if (dt != PCS_F32 && dt != PCS_F64) return PCS_EINVAL;
  if (!x || !out || !ws || n < 0 || ((uintptr_t)ws & 7)) return PCS_EINVAL;
  if (!(a >= 0.0) || !(b >= 0.0) || (a == 0.0 && b == 0.0)) return PCS_EINVAL;
  if (mode != PCS_THRESH_SOFT && mode != PCS_THRESH_CLIP) return PCS_EINVAL;
  if (n == 0) return PCS_OK;
  return dt == PCS_F32 ? thresh_l1<float>(x, out, n, a, b, mode, t_dev, ws, st)
                       : thresh_l1<double>(x, out, n, a, b, mode, t_dev, ws, st);
}

int pcs_thresh_pick_host(int dt, uint64_t lo, uint64_t hi, double sum_abs, const double* sums, double a, double b,
                         double* pivots_out, uint64_t* bracket_out) {
  if (dt != PCS_F32 && dt != PCS_F64) return PCS_EINVAL;
  if (lo > hi || hi > (dt == PCS_F32 ? 0x7fffffffull : 0x7fffffffffffffffull)) return PCS_EINVAL;
  if (!(a >= 0.0) || !(b >= 0.0) || (a == 0.0 && b == 0.0)) return PCS_EINVAL;
  if (pivots_out)
    for (int j = 1; j <= kThrJ; ++j) pivots_out[j - 1] = key_value(dt, thresh_pivot(lo, hi, j));
  if (!sums) return kThrJ;
  if (!bracket_out) return PCS_EINVAL;
  if (thresh_inside(sum_abs, a)) {
    bracket_out[0] = bracket_out[1] = 0;
    return 0;
  }
  thresh_pick(dt, lo, hi, sums, a, b, &bracket_out[0], &bracket_out[1]);
  return kThrJ;
}

}  // extern "C"
