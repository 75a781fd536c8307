// The five Green functions of pycsou/math/green.py as closed forms, and the distances of MappedDistanceMatrix
// (pycsou/linop/sampling.py:772-1058), for the kernels of mdm.hip.  Everything is evaluated in T (fp32 with the
// standard sqrtf / expf / powf, fp64 with sqrt / exp / pow; no fast-math intrinsic), in the order of operations
// the NumPy expressions imply.  (kind, k, p0, p1) is what the Python classes' _device_spec() returns:
//   PCS_GREEN_MATERN       k in 0..3, p0 = epsilon > 0
//   PCS_GREEN_WENDLAND     k in 0..3, p0 = epsilon > 0
//   PCS_GREEN_SUBGAUSSIAN  p0 = alpha in (0, 2), p1 = epsilon > 0
//   PCS_GREEN_CAUSAL_ITER  k >= 1
//   PCS_GREEN_CAUSAL_EXP   k >= 1, p0 = alpha > 0
// Negative arguments do what NumPy does: the causal functions multiply by (x >= 0), SubGaussian is NaN (pow of a
// negative base), Matern and Wendland evaluate their formulas; 0^0 = 1.
#pragma once

#include <math.h>

#include "common.hpp"

namespace pcs {

constexpr int kGreenMaxCausalK = 1 << 20;

inline bool green_params_ok(int kind, int k, double p0, double p1) {
  switch (kind) {
    case PCS_GREEN_MATERN:
    case PCS_GREEN_WENDLAND:
      return k >= 0 && k <= 3 && p0 > 0.0 && p0 < INFINITY;
    case PCS_GREEN_SUBGAUSSIAN:
      return p0 > 0.0 && p0 < 2.0 && p1 > 0.0 && p1 < INFINITY;
    case PCS_GREEN_CAUSAL_ITER:
      return k >= 1 && k <= kGreenMaxCausalK;
    case PCS_GREEN_CAUSAL_EXP:
      return k >= 1 && k <= kGreenMaxCausalK && p0 > 0.0 && p0 < INFINITY;
    default:
      return false;
  }
}

// The parameters of one function, converted to T once per thread.
template <typename T>
struct GreenSpec {
  int kind, k;
  T p0, p1;
};

__device__ __forceinline__ float g_exp(float v) { return expf(v); }
__device__ __forceinline__ double g_exp(double v) { return exp(v); }
__device__ __forceinline__ float g_pow(float a, float b) { return powf(a, b); }
__device__ __forceinline__ double g_pow(double a, double b) { return pow(a, b); }
__device__ __forceinline__ float g_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double g_sqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float g_abs(float v) { return fabsf(v); }
__device__ __forceinline__ double g_abs(double v) { return fabs(v); }

// x^m for an integer m >= 0: products up to the cube, pow beyond (0^0 = 1)
template <typename T>
__device__ __forceinline__ T g_powi(T x, int m) {
  return m == 0 ? T(1) : m == 1 ? x : m == 2 ? x * x : m == 3 ? x * x * x : g_pow(x, (T)m);
}

template <typename T>
__device__ __forceinline__ T green_phi(const GreenSpec<T>& g, T r) {
  switch (g.kind) {
    case PCS_GREEN_MATERN: {
      const T eps = g.p0;
      if (g.k == 0) return g_exp(-r / eps);
      const T s = g.k == 1 ? T(1.7320508075688772) : g.k == 2 ? T(2.23606797749979) : T(2.6457513110645907);
      const T decay = g_exp(-s * r / eps);
      T poly = T(1) + s * r / eps;
      if (g.k == 2) poly += (T(5) * (r * r)) / (T(3) * (eps * eps));
      if (g.k == 3)
        poly = poly + (T(42) * (r * r)) / (T(15) * (eps * eps)) + (T(7) * s * (r * r * r)) / (T(15) * (eps * eps * eps));
      return poly * decay;
    }
    case PCS_GREEN_WENDLAND: {
      const T eps = g.p0;
      T t = T(1) - r / eps;
      t = t < T(0) ? T(0) : t;   // np.clip(., 0, None): a NaN stays a NaN
      const T t2 = t * t;
      if (g.k == 0) return t2;
      const T t4 = t2 * t2;
      if (g.k == 1) return t4 * (T(1) + T(4) * r / eps);
      if (g.k == 2) return (t4 * t2) * (T(1) + T(6) * r / eps + T(35) * (r * r) / (T(3) * (eps * eps)));
      return (t4 * t4) *
             (T(1) + T(8) * r / eps + T(25) * (r * r) / (eps * eps) + T(32) * (r * r * r) / (eps * eps * eps));
    }
    case PCS_GREEN_SUBGAUSSIAN:
      return g_exp(-g_pow(r, g.p0) / g.p1);
    case PCS_GREEN_CAUSAL_ITER:
      return g_powi(r, g.k - 1) * (r >= T(0) ? T(1) : T(0));
    default:  // PCS_GREEN_CAUSAL_EXP
      return g_powi(r, g.k - 1) * g_exp(-g.p0 * r) * (r >= T(0) ? T(1) : T(0));
  }
}

// How d(p, q) is formed: the three fast paths of the radial mode, the general ord > 0, the zonal mode.
enum { kDistL1 = 0, kDistL2 = 1, kDistLinf = 2, kDistLp = 3, kDistZonal = 4 };

inline int dist_kind(int mode, double ord) {
  if (mode == PCS_MDM_ZONAL) return kDistZonal;
  return ord == 1.0 ? kDistL1 : ord == 2.0 ? kDistL2 : ord == INFINITY ? kDistLinf : kDistLp;
}

// d(p, q) of two points of DIM coordinates: ||p - q||_ord, or clip(<p, q>, -1, 1).  `ord` and `inv_ord` (1 / ord,
// rounded once from the fp64 quotient) are read by kDistLp alone.
template <typename T, int DIM>
__device__ __forceinline__ T mdm_dist(int dk, T ord, T inv_ord, const T (&p)[DIM], const T (&q)[DIM]) {
  T s = T(0);
  switch (dk) {
    case kDistL2:
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        const T v = p[d] - q[d];
        s += v * v;
      }
      return g_sqrt(s);
    case kDistL1:
#pragma unroll
      for (int d = 0; d < DIM; ++d) s += g_abs(p[d] - q[d]);
      return s;
    case kDistLinf:
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        const T v = g_abs(p[d] - q[d]);
        s = v > s ? v : s;
      }
      return s;
    case kDistLp:
#pragma unroll
      for (int d = 0; d < DIM; ++d) s += g_pow(g_abs(p[d] - q[d]), ord);
      return g_pow(s, inv_ord);
    default:
#pragma unroll
      for (int d = 0; d < DIM; ++d) s += p[d] * q[d];
      return clip1(s);
  }
}

}  // namespace pcs
