// The per-element PDS update rule, stated once for every fused step kernel (pds*.hpp / pds*.hip, pds3d.hip):
//   x~ = prox_G((x - tau gradF) - tau K^T z)                 primal_prox
//   u  = 2 x~ - x                                            reflect
//   x' = rho x~ + (1 - rho) x                                relax
//   z' = rho prox_{sigma H*}(z + sigma K u) + (1 - rho) z    fenchel, relax
// The kernels keep what differs between them: gradF, K^T z and K u, the `own` / `in` masks, the stores and
// the per-launch sums.  Every helper is generic over the parameter struct (Params<T>, GenP<T>, P3<T>: kernel
// arguments whose layouts stay their own) and is a pure expression of its arguments.
//
// The helpers' shapes are chosen so that every step kernel compiles to the machine code of the hand-written
// lines they replaced (tools/asm_ab.py; profiles/update_rule_asm_ab.txt).  The compiler inlines them only
// after its first simplification of the caller, and its schedule follows the order of the statements, so:
//  * a site evaluates in the order it always did: grad_step before the K^T z passed to primal_prox; dual_arg
//    per component where K u is an expression; w0, w1, v0, v1 (fenchel_w) or w0, v0, w1, v1 (fenchel);
//  * the kernels whose H kind is a run-time argument keep their if / else and scalar temporaries and call the
//    scalar pieces (l21_shrink, fenchel_l21, fenchel_l1); the others hand arrays to fenchel_w / fenchel;
//  * `in ? reflect(xt, xv) : 0` stays as the site had it; the tile kernel and pds3d.hip's backward / centred
//    step take reflect() before the conditional, which is what reproduces their code.
//
// The kernels do not round alike; the template parameters name the spelling, DESIGN.md section 4 lists which
// kernel uses which:
//   Fenchel::Literal  w - sigma prox_{H/sigma}(w / sigma), the reference's op sequence
//   Fenchel::Direct   clip(w, -lam, lam) / w min(1, lam / ||w||): the same map, fewer roundings (fp32 only)
//   FMA = false       a * b + c as written, contracted by the compiler where it sees fit
//   FMA = true        an explicit fma: the same bits in every instantiation of a kernel (stencil.hpp)
#pragma once

#include <type_traits>

#include "common.hpp"

namespace pcs {

template <typename T>
struct G4 {
  T v[4];
};

template <typename T>
struct Params {
  T tau, sigma, inv_sigma, rho, omr, t_h, inv_t_h, inv_step0, inv_step1, seg_a, seg_b;
  T lam;  // H = lam * L1 / L21 (the normal-operator kernel's fenchel step: clip / scale by lam)
  int unit0, unit1;  // step == 1: skip the scaling (exact)
};

template <typename T>
__device__ __forceinline__ T prox_g(T v, int gk, T a, T b) {
  if (gk == PCS_G_NONNEG) return (v < T(0)) ? T(0) : v;  // math/prox.py:295-297
  if (gk == PCS_G_SEGMENT) {                             // math/prox.py:340-343
    v = (v < a) ? a : v;
    return (v > b) ? b : v;
  }
  return v;
}

__device__ __forceinline__ float fast_rsqrt(float v) { return __builtin_amdgcn_rsqf(v); }
// fp64: v_rsq_f64 and two Newton steps (each squares the relative error: ~1 ulp) instead of 1.0 / sqrt(v),
// an IEEE square root and an IEEE division (~25 fp64 instructions on the fenchel prox's path).  v = 0 and
// v = +inf keep the hardware's exact +inf / 0 (a Newton step would turn them into NaN)
__device__ __forceinline__ double fast_rsqrt(double v) {
  const double y0 = __builtin_amdgcn_rsq(v);
  const double h = 0.5 * v;
  double y = y0 * __builtin_fma(-h * y0, y0, 1.5);
  y = y * __builtin_fma(-h * y, y, 1.5);
  return (v == 0.0 || v == __builtin_huge_val()) ? y0 : y;
}

// x - tau gradF, and x~ from it and K^T z (kt: already scaled by 1 / step).  Two calls, so that a site
// evaluates x - tau gradF before the K^T z it passes: primal_prox(grad_step(xv, gf, P), kt, gk, P)
template <typename T, typename PT>
__device__ __forceinline__ T grad_step(T xv, T gf, const PT& P) {
  return xv - P.tau * gf;
}
template <typename T, typename PT>
__device__ __forceinline__ T primal_prox(T xg, T kt, int gk, const PT& P) {
  return prox_g(xg - P.tau * kt, gk, P.seg_a, P.seg_b);
}

template <typename T>
__device__ __forceinline__ T reflect(T xt, T xv) {
  return T(2) * xt - xv;
}

// rho t + (1 - rho) old
template <bool FMA, typename T, typename PT>
__device__ __forceinline__ T relax(T t, T old, const PT& P) {
  if constexpr (FMA) return pcs_fma(P.rho, t, P.omr * old);
  else return P.rho * t + P.omr * old;
}

enum class Fenchel { Literal, Direct };

// w = z + sigma K u for one component (ku: K u, already scaled by 1 / step)
template <typename T, typename PT>
__device__ __forceinline__ T dual_arg(T zv, T ku, const PT& P) {
  return zv + P.sigma * ku;
}

// The literal form piece by piece, scalars in and out, for the kernels that take the H kind as a run-time
// argument (pds_tile.hpp, pds_gen.hip, pds3d.hip): they keep the if / else on hk and their own temporaries,
// since results handed back through an array reach the optimiser as memory and come out scheduled otherwise.
//   v = w / sigma;  L21: f = max(1 - t / ||v||, 0), zt = w - sigma (f v);  L1: zt = w - sigma (v - t clip(v / t))
template <typename T, typename PT>
__device__ __forceinline__ T dual_scaled(T w, const PT& P) {
  return w * P.inv_sigma;
}
template <bool FMA, typename T>
__device__ __forceinline__ T norm2(T a, T b) {
  if constexpr (FMA) return pcs_fma(a, a, b * b);
  else return a * a + b * b;
}
template <bool FMA, typename T>
__device__ __forceinline__ T norm2(T a, T b, T c) {
  if constexpr (FMA) return pcs_fma(a, a, pcs_fma(b, b, c * c));
  else return (a * a + b * b) + c * c;
}
template <typename T, typename PT>
__device__ __forceinline__ T l21_shrink(T n2, const PT& P) {  // penalty.py:551-557
  const T f = T(1) - P.t_h * fast_rsqrt(n2);
  return f > T(0) ? f : T(0);
}
template <typename T, typename PT>
__device__ __forceinline__ T fenchel_l21(T w, T v, T f, const PT& P) {
  return w - P.sigma * (f * v);
}
template <typename T, typename PT>
__device__ __forceinline__ T fenchel_l1(T w, T v, const PT& P) {  // func/base.py:239-240
  return w - P.sigma * (v - P.t_h * clip1(v * P.inv_t_h));
}

// zt = prox_{sigma H*}(w) for one element's D components w, v = w / sigma; H = t_h sigma L21 over the D
// components if hk == PCS_H_L21 and D >= 2, else t_h sigma L1.  FMA spells the group norm; the direct form
// does not read v.
template <int D, Fenchel FORM, bool FMA, typename T, typename PT>
__device__ __forceinline__ void fenchel_wv(int hk, const T (&w)[D], const T (&v)[D], const PT& P, T (&zt)[D]) {
  static_assert(D == 1 || D == 2, "one group is the two components of a 2-D gradient");
  if constexpr (FORM == Fenchel::Direct) {
    static_assert(std::is_same<T, float>::value, "the direct form is fp32 only");
    if (D >= 2 && hk == PCS_H_L21) {
      // w - sigma prox_{L21, t}(w / sigma) (penalty.py:551-557, t = lam / sigma) = w min(1, lam / ||w||)
      const T sc = fminf(T(1), P.lam * fast_rsqrt(norm2<FMA>(w[0], w[D - 1])));
#pragma unroll
      for (int d = 0; d < D; ++d) zt[d] = w[d] * sc;
    } else {  // w - sigma (v - t clip(v / t)), v = w / sigma (func/base.py:239-240) = clip(w, -lam, lam)
#pragma unroll
      for (int d = 0; d < D; ++d) zt[d] = fminf(fmaxf(w[d], -P.lam), P.lam);
    }
  } else {
    if (D >= 2 && hk == PCS_H_L21) {
      const T f = l21_shrink(norm2<FMA>(v[0], v[D - 1]), P);
#pragma unroll
      for (int d = 0; d < D; ++d) zt[d] = fenchel_l21(w[d], v[d], f, P);
    } else {
#pragma unroll
      for (int d = 0; d < D; ++d) zt[d] = fenchel_l1(w[d], v[d], P);
    }
  }
}
// The same from w alone: every w is formed by the caller (dual_arg), then every v here -- w0, w1, v0, v1
template <int D, Fenchel FORM, bool FMA, typename T, typename PT>
__device__ __forceinline__ void fenchel_w(int hk, const T (&w)[D], const PT& P, T (&zt)[D]) {
  T v[D];
  if constexpr (FORM == Fenchel::Literal) {
#pragma unroll
    for (int d = 0; d < D; ++d) v[d] = dual_scaled(w[d], P);
  }
  fenchel_wv<D, FORM, FMA>(hk, w, v, P, zt);
}
// The same from z and K u, component by component -- w0, v0, w1, v1; z is element m of D four-groups, read in
// place (the general-stencil march: with the elements copied out first its centred kernels schedule otherwise)
template <int D, Fenchel FORM, bool FMA, typename T, typename PT>
__device__ __forceinline__ void fenchel(int hk, const G4<T> (&zv)[D], int m, const T (&ku)[D], const PT& P,
                                        T (&zt)[D]) {
  T w[D], v[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    w[d] = dual_arg(zv[d].v[m], ku[d], P);
    v[d] = dual_scaled(w[d], P);
  }
  fenchel_wv<D, FORM, FMA>(hk, w, v, P, zt);
}

// The masked data term's dual block, H = |. - y|_1 and K = the mask (K u = u at a sampled pixel):
// prox_{sigma H*}(z + sigma u) through ProxFuncPreComp's shift by -y
template <typename T, typename PT>
__device__ __forceinline__ T fenchel_l1_shifted(T zv, T u, T yv, const PT& P) {
  const T w = zv + P.sigma * u;
  const T a = w * P.inv_sigma + (-yv);                // ProxFuncPreComp: v + (-y)
  const T pl = a - P.inv_sigma * clip1(a * P.sigma);  // prox_l1(a, 1 / sigma)
  return w - P.sigma * (pl - (-yv));
}

}  // namespace pcs
