// The two-pass normal-operator kernels of a separable blur (N = C^T C as two 29-tap passes), shared by
// sep_ata.hip (out = N in [- sub]) and apgd2d.hip (the same march with the APGD update as its epilogue).
#pragma once

#include <type_traits>

#include "pds_ctrl.hpp"
#include "vecio.hpp"

namespace pcs {

// ---------------------------------------------------------------------------------------------
// The same operator as TWO 29-tap passes (the default when the taps reach <= 7 samples either
// side and the plane is >= 16 x 16): per axis C^T C is the autocorrelation of the taps,
//   (C^T C)[j, k] = a[j - k] - E[j][k],  a[e] = sum_m c(m) c(m + e),  c(d) = h[d + off],
// E the terms of the samples outside the plane (rows i < 0 / i >= n), nonzero only for j, k in
// the 7 samples nearest each edge (the zero boundary of the reference's Convolve1D, PyLops 1.x
// `Convolve1D` truncation between C and C^T).  A 128-column (fp32) / 64-column (fp64) strip
// marches down a row segment 32 rows per step:
//   PH  horizontal 29-tap pass of the 32 staged input rows (+ the left / right edge terms)
//       -> a ring of RS + 28 rows (each input row filtered once: no vertical halo recomputed)
//   PV  vertical 29-tap pass, RB rows x 4 columns per thread (RB + 28 ring reads per 4 RB
//       outputs) + the top / bottom edge terms -> HBM
// Two barriers per step; the next step's input rows are in flight (registers) during PH and PV.
// The tables (a for both axes, the four 7x7 edge blocks) are built per workgroup from the taps
// in fp64.  2 words of HBM traffic per voxel, like one k_sep2d_march pass, for the work of two.
// fp32 geometry (fp64 takes k_sep2d_nrmm below): 128-column strips, 32-row steps, PV items of 4 rows x
// 4 columns, PH items of 16 outputs (0.433-0.449 against 0.469 ms for 8 at 512^3, C4 642-645 against
// 633-635 it/s, profiles/r4_nrm_cfg6_ab.txt).  Measured without gain and removed in round 5: loads two
// steps ahead, packed-FMA PV, PH unroll, PV chunks of 2 / 8 rows, lane-rotated LDS writes
// (profiles/r4_nrm_var_ab*.txt, r4_nrm_swz_ab.txt)
struct NrmF {
  static constexpr int PQ = 4;  // PH item: 4 PQ outputs of one row
  static constexpr int TX = 128, RS = 32, RB = 4, RING = RS + 28, GX = TX / 4, GI = GX + 8;
  // the lanes of a b128 group read every fourth 16-B slot of rows r .. r + 3, so the staged rows take an
  // odd slot pitch (22.4 M bank-conflict cycles per 512^3 launch without it at 8 outputs,
  // profiles/r4_prof_nrm32_pmc_summary.txt)
  static constexpr int SPAD = 4, WI = 4 * GI + SPAD, TP = TX;
  static constexpr int NT = (RS / RB) * GX, NIN = RS * GI, NL = (NIN + NT - 1) / NT, NPH = RS * GX / PQ;
  static constexpr int NST = RB;  // 16-B stores per thread per step
  static constexpr int NTAB = 288;  // a_v[0..29), a_h[32..61), E_v lo / hi, E_h lo / hi (7 x 8 each)
  static_assert(NPH % NT == 0, "whole PH items per thread");
  static constexpr size_t lds_bytes() { return 4 * ((size_t)RS * WI + (size_t)RING * TP + NTAB); }
};

// compiler fences of the PV chunks: no LDS read or FMA moves across (bounds the registers held
// by hoisted window reads) ...
__device__ __forceinline__ void nrm_fence() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
// ... and the chunk's FMAs stay before the fence (not sunk below the later reads)
template <typename T>
__device__ __forceinline__ void nrm_pin(Q4<T>& a) {
  asm volatile("" : "+v"(a.v[0]), "+v"(a.v[1]), "+v"(a.v[2]), "+v"(a.v[3]));
}

// 4 elements through a descriptor (16-B stores; an offset carrying kOOB is dropped)
template <typename T>
__device__ __forceinline__ void nrm_bstore(Rsrc r, uint32_t off, const Q4<T>& a) {
  typedef unsigned int u4 __attribute__((ext_vector_type(4)));
  constexpr int VN = V16<T>::N;
#pragma unroll
  for (int h = 0; h < 4 / VN; ++h) {
    u4 d;
    __builtin_memcpy(&d, a.v + h * VN, 16);
    __builtin_amdgcn_raw_buffer_store_b128(d, r, (int)(off + 16 * h), 0, 0);
  }
}

// a += h w on 4 columns
template <typename T>
__device__ __forceinline__ void nrm_fma4(Q4<T>& a, T h, const Q4<T>& w) {
#pragma unroll
  for (int m = 0; m < 4; ++m) a.v[m] += h * w.v[m];
}

// tap d of a filter stored as h[0..k) with offset off (zero outside)
__device__ __forceinline__ double nrm_tap(const double* h, int k, int off, int d) {
  const int t = d + off;
  return (t >= 0 && t < k) ? h[t] : 0.0;
}

// 4 elements through a descriptor (16-B loads; an offset carrying kOOB reads 0)
template <typename T>
__device__ __forceinline__ Q4<T> nrm_bload(Rsrc r, uint32_t off) {
  constexpr int VN = V16<T>::N;
  Q4<T> a;
#pragma unroll
  for (int h = 0; h < 4 / VN; ++h) {
    const auto d = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(off + 16 * h), 0, 0);
    __builtin_memcpy(a.v + h * VN, &d, 16);
  }
  return a;
}

// ---- output policies of the PV phase.  NrmStore: out = acc (SUB: acc - sub), the operator alone.
struct NrmStore {
  static constexpr bool kApgd = false;
};

// lam*L1Norm.prox: x - t * proj_linfty_ball(x / t, 1), as prox_l1_el of prox.hip
template <typename T>
__device__ __forceinline__ T nrm_prox_l1(T v, T t) {
  return v - t * clip1(v / t);
}

// NrmApgd: one AcceleratedProximalGradientDescent.update_iterand (pycsou/opt/proxalgs.py:586-601) on the value
// the march is about to store, element by element in the expression order of k_apgd_step (prox.hip):
//   g = acc - cty (the SUB subtraction) ; w = prox_G(x - tau g) ; x' = w + a (w - aux) ; aux' = w
// x' goes to the march's `out`, aux' to aux_n; d2 / n2 collect this thread's (x - x')^2 and x^2 in fp64.
// x, aux and cty of the output rows are loaded AFTER PV: the march holds 165 of the 168 VGPRs of its
// 3-workgroup (fp32) occupancy through PH and PV, and the rows' x was staged 14-28 rows ago (a cache hit)
template <typename T>
struct NrmApgd {
  static constexpr bool kApgd = true;
  const T* aux;
  T* aux_n;
  T tau, a, thr, sa, sb;
  int gk;
  double d2, n2;  // 0 at launch
  // loop control, as the PDS step kernels (pds_ctrl.hpp): a launch after the stop stores nothing; at its end
  // every workgroup publishes its two sums (the dual pair 0) and the last one records the metric, advances
  // Ctrl::it and sets the stop flag
  double* partials;
  void* ws;
  Ctrl* ctrl;
  double* hist;
  __device__ __forceinline__ bool stopped() const { return ctrl->stopped != 0; }
  __device__ __forceinline__ void finish() {
    __shared__ double red[2 * 4];
    __shared__ int flag[2];
    double v[2] = {d2, n2};
    block_sum<2>(v, red);
    const double part[4] = {v[0], v[1], 0.0, 0.0};
    publish_partials(part, partials, gridDim.x, ws, ctrl, hist, flag, RedOut{nullptr, nullptr, 0, nullptr});
  }
  // one 16-B chunk of VW elements: g (in) -> x' (out), w (out) = aux'
  template <int VW>
  __device__ __forceinline__ void apply(T (&g)[VW], T (&w)[VW], const T (&xv)[VW], const T (&av)[VW], bool live) {
#pragma unroll
    for (int m = 0; m < VW; ++m) {
      T u = xv[m] - tau * g[m];
      if (gk == PCS_APGD_G_L1) {
        u = nrm_prox_l1(u, thr);
      } else if (gk == PCS_G_NONNEG) {
        u = (u < T(0)) ? T(0) : u;
      } else if (gk == PCS_G_SEGMENT) {
        u = (u < sa) ? sa : u;
        u = (u > sb) ? sb : u;
      }
      const T xnew = u + a * (u - av[m]);
      w[m] = u;
      g[m] = xnew;
      if (live) {
        const double d = (double)xv[m] - (double)xnew;
        d2 += d * d;
        n2 += (double)xv[m] * (double)xv[m];
      }
    }
  }
};

// the kernel's policy object: its trailing argument, or a stateless one
template <class EP>
__device__ __forceinline__ EP nrm_policy() {
  return EP{};
}
template <class EP>
__device__ __forceinline__ EP nrm_policy(const EP& e) {
  return e;
}

// one 16-B chunk through a descriptor, either way
template <typename T>
__device__ __forceinline__ void nrm_bload16(Rsrc r, uint32_t off, T (&a)[16 / sizeof(T)]) {
  const auto d = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
  __builtin_memcpy(a, &d, 16);
}
template <typename T>
__device__ __forceinline__ void nrm_bstore16(Rsrc r, uint32_t off, const T (&a)[16 / sizeof(T)]) {
  typedef unsigned int u4 __attribute__((ext_vector_type(4)));
  u4 d;
  __builtin_memcpy(&d, a, 16);
  __builtin_amdgcn_raw_buffer_store_b128(d, r, (int)off, 0, 0);
}

// The APGD epilogue of one PV item: RB rows x one 16-B chunk.  acc[rr] holds N x of row rr; offs[rr] is the
// chunk's byte offset in every image-shaped array (kOOB when the row is not the task's: loads read 0, stores
// are dropped).  All 3 RB loads are issued before the first is used; 2 RB stores per item
template <typename T, int RB, typename ACC>
__device__ __forceinline__ void nrm_apgd_rows(NrmApgd<T>& ep, ACC (&acc)[RB], const uint32_t (&offs)[RB], Rsrc rx,
                                              Rsrc rcty, Rsrc raux, Rsrc rxn, Rsrc rauxn) {
  constexpr int VW = 16 / sizeof(T);
  T xv[RB][VW], av[RB][VW], cv[RB][VW];
#pragma unroll
  for (int rr = 0; rr < RB; ++rr) {
    nrm_bload16<T>(rcty, offs[rr], cv[rr]);
    nrm_bload16<T>(rx, offs[rr], xv[rr]);
    nrm_bload16<T>(raux, offs[rr], av[rr]);
  }
#pragma unroll
  for (int rr = 0; rr < RB; ++rr) {
    T g[VW], w[VW];
#pragma unroll
    for (int m = 0; m < VW; ++m) g[m] = acc[rr].v[m] - cv[rr][m];
    ep.template apply<VW>(g, w, xv[rr], av[rr], offs[rr] != kOOB);
    nrm_bstore16<T>(rxn, offs[rr], g);
    nrm_bstore16<T>(rauxn, offs[rr], w);
  }
}

// SUB: out = C^T C in - sub (sub laid out as in / out; a 2-D step's grad F = N x - Conv^T y formed here, so
// the step reads one buffer instead of two -- the same subtraction, bit for bit).  fp32 (T = float): 53 KB of
// LDS, 3 workgroups / CU.  EP: the output policy; a policy with state (NrmApgd) is the trailing kernel
// argument, NrmStore adds none
template <typename T, bool SUB, class EP = NrmStore, class... EA>
__global__ __launch_bounds__(NrmF::NT, 3) void k_sep2d_nrm(const T* __restrict__ in, T* __restrict__ out, int n1,
                                                           int n2, int nstrips, int nseg, int seg_len, int64_t ntasks,
                                                           const T* __restrict__ ha_, int ka, int offa,
                                                           const T* __restrict__ hb_, int kb, int offb,
                                                           const T* __restrict__ sub, EA... ea) {
  static_assert(sizeof(T) == 4, "fp32 (fp64: k_sep2d_nrmm)");
  static_assert(SUB || !EP::kApgd, "the APGD epilogue subtracts Conv^T y");
  EP ep = nrm_policy<EP>(ea...);
  if constexpr (EP::kApgd) {
    if (ep.stopped()) return;
  }
  using G = NrmF;
  constexpr int TX = G::TX, RS = G::RS, RB = G::RB, RING = G::RING, GX = G::GX, GI = G::GI, WI = G::WI, NT = G::NT,
                NL = G::NL, TP = G::TP;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* stg = reinterpret_cast<T*>(smem_raw);  // RS x WI staged input rows
  T* ring = stg + RS * WI;                  // RING rows (pitch TP) of the horizontal pass
  T* tab = ring + RING * TP;                // NTAB
  const int tid = threadIdx.x;
  {
    __shared__ double hs[32];  // the two filters in fp64
    if (tid < 16) hs[tid] = tid < ka ? (double)ha_[tid] : 0.0;
    else if (tid < 32) hs[tid] = tid - 16 < kb ? (double)hb_[tid - 16] : 0.0;
    __syncthreads();
    for (int e = tid; e < G::NTAB; e += NT) {
      double v = 0.0;
      if (e < 64) {
        const int q = e & 31;
        const double* h = e < 32 ? hs : hs + 16;
        const int k = e < 32 ? ka : kb, off = e < 32 ? offa : offb;
        if (q < 29)
          for (int m = -7; m <= 7; ++m) v += nrm_tap(h, k, off, m) * nrm_tap(h, k, off, m + q - 14);
      } else {
        const int idx = e - 64, tb = idx / 56, r = idx - 56 * tb, j = r >> 3, c = r & 7;
        const double* h = tb < 2 ? hs : hs + 16;
        const int k = tb < 2 ? ka : kb, off = tb < 2 ? offa : offb;
        if (c < 7) {
          if ((tb & 1) == 0)  // rows / columns i = -7..-1 before the plane: E[j][c], j, c < 7
            for (int i = -7; i < 0; ++i) v += nrm_tap(h, k, off, i - j) * nrm_tap(h, k, off, i - c);
          else  // after it: j = n - 7 + jj, c = n - 7 + cc, i = n + ii
            for (int ii = 0; ii < 7; ++ii) v += nrm_tap(h, k, off, 7 + ii - j) * nrm_tap(h, k, off, 7 + ii - c);
        }
      }
      tab[e] = (T)v;
    }
    __syncthreads();
  }
  // the autocorrelation is symmetric: window tap q is a[|q - 14|], 15 registers per axis
  T av[15], ah[15];
#pragma unroll
  for (int e = 0; e < 15; ++e) {
    av[e] = tab[14 + e];
    ah[e] = tab[32 + 14 + e];
  }
  const T* evl = tab + 64;
  const T* evh = tab + 120;
  const T* ehl = tab + 176;
  const T* ehh = tab + 232;
  const XcdShare own = xcd_share(ntasks);  // XCD x owns a contiguous share of the task list (common.hpp)
  const int64_t t0 = own.t0, t_end = own.end, t_stride = own.stride;
  if (t0 >= t_end) {
    if constexpr (EP::kApgd) ep.finish();
    return;
  }
  struct Cur {
    int64_t t, plane;
    int strip, a, b, s, ns;
  };
  auto task_at = [&](int64_t t) {
    Cur c;
    c.t = t;
    const int64_t per_plane = (int64_t)nseg * nstrips;
    c.plane = t / per_plane;
    const int rem = (int)(t - c.plane * per_plane), seg = rem / nstrips;
    c.strip = rem - seg * nstrips;
    c.a = seg * seg_len;
    c.b = min(n1, c.a + seg_len);
    c.s = 0;
    c.ns = (c.b - c.a + 28 + RS - 1) / RS;
    return c;
  };
  // staged rows of step s: input rows a - 14 + s RS + rr, columns c0 - 16 + 4 gg (0 outside)
  auto prefetch = [&](const Cur& c, Q4<T>(&q)[NL]) {
    const T* src = in + c.plane * (int64_t)n1 * n2;
    const int kmax = c.b - c.a + 27;  // last staged row any output of [a, b) reads
    const int gc0 = c.strip * TX - 16;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const int e = min(l * NT + tid, G::NIN - 1);
      const int rr = e / GI, gg = e - rr * GI;
      const int k = c.s * RS + rr, gi = c.a - 14 + k, gc = gc0 + 4 * gg;
      const bool ok = gi >= 0 && gi < n1 && k <= kmax && gc >= 0 && gc + 4 <= n2;
      const Q4<T> v = ldq(src + (ok ? (int64_t)gi * n2 + gc : 0));
#pragma unroll
      for (int m = 0; m < 4; ++m) q[l].v[m] = ok ? v.v[m] : T(0);
    }
  };
  // the staged rows have landed (WAITN: the memory ops issued after them that may stay in flight --
  // vector memory ops retire in order); rows -> LDS
  auto stage = [&](const Q4<T>(&q)[NL], auto waitn) {
    constexpr int WN = decltype(waitn)::value;
    __builtin_amdgcn_s_waitcnt((WN & 15) | ((WN >> 4) << 14) | (7 << 4) | (15 << 8));
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const int e = l * NT + tid, rr = e / GI, gg = e - rr * GI;
      if (e < G::NIN) stq(stg + rr * WI + 4 * gg, q[l]);
    }
  };
  // one step on the staged rows of cur: PH into the ring, PV from it -> HBM
  auto body = [&](const Cur cur) {
    const int vi = tid / GX, vg = tid - vi * GX;  // PV item: rows RB vi .. + RB - 1 of the step, group vg
    const int c0 = cur.strip * TX;
    Q4<T> bsub[SUB && !EP::kApgd ? RB : 1];  // SUB: the PV outputs' sub values, loaded before PH (a phase to land)
    if constexpr (SUB && !EP::kApgd) {
      const Rsrc rs = rsrc_of(sub + cur.plane * (int64_t)n1 * n2, (uint32_t)((int64_t)n1 * n2 * sizeof(T)));
      const int gc = c0 + 4 * vg;
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) {
        const int i = cur.a - 28 + cur.s * RS + RB * vi + rr;
        const bool live = i >= cur.a && i < cur.b && gc < n2;
        bsub[rr] = nrm_bload<T>(rs, live ? (uint32_t)(((int64_t)i * n2 + gc) * sizeof(T)) : kOOB);
      }
    }
    const int sb = (cur.s * RS) % RING;  // ring slot of the step's first staged row
    lds_barrier();
    // ---- PH: t[row][c0 + j] = sum_q a_h[q] x[row][c0 + j - 14 + q] (staged column j + 2 + q);
    // an item is 4 PQ consecutive outputs of one row (PQ + 8 window reads)
#pragma unroll 1
    for (int l = 0; l < G::NPH / NT; ++l) {
      constexpr int PQ = G::PQ, GQ = GX / PQ;
      const int e = l * NT + tid, r = e / GQ, g = PQ * (e - r * GQ);
      const T* srow = stg + r * WI;
      T acc[4 * PQ];
#pragma unroll
      for (int o = 0; o < 4 * PQ; ++o) acc[o] = T(0);
#pragma unroll
      for (int u = 0; u < PQ + 8; ++u) {
        const Q4<T> v = ldsq(srow + 4 * (g + u));
#pragma unroll
        for (int ee = 0; ee < 4; ++ee)
#pragma unroll
          for (int o = 0; o < 4 * PQ; ++o) {
            const int qq = 4 * u + ee - o - 2;
            if (qq >= 0 && qq < 29) acc[o] += ah[qq < 14 ? 14 - qq : qq - 14] * v.v[ee];
          }
      }
      const int col = c0 + 4 * g;
      if (col < 7 || col + 4 * PQ - 1 >= n2 - 7) {  // the edge terms of the first / last 7 columns
#pragma unroll
        for (int o = 0; o < 4 * PQ; ++o) {
          const int j = col + o;
          if (j < 7) {
            for (int c = 0; c < 7; ++c) acc[o] -= ehl[8 * j + c] * srow[16 + c];
          } else if (j >= n2 - 7 && j < n2) {
            const int jj = j - (n2 - 7), s0 = n2 - 7 - c0 + 16;
            for (int c = 0; c < 7; ++c) acc[o] -= ehh[8 * jj + c] * srow[s0 + c];
          }
        }
      }
      int slot = sb + r;
      slot = slot >= RING ? slot - RING : slot;
#pragma unroll
      for (int k = 0; k < PQ; ++k) {
        Q4<T> c;
#pragma unroll
        for (int m = 0; m < 4; ++m) c.v[m] = acc[4 * k + m];
        stq(ring + slot * TP + 4 * (g + k), c);
      }
    }
    lds_barrier();
    // ---- PV: out row i = a - 28 + s RS + r reads t rows i - 14 .. i + 14 (staged s RS + r - 28 ..)
    {
      const int r0 = RB * vi;
      const int base = (cur.s * RS + r0 - 28 + RING) % RING;
      Q4<T> acc[RB];
#pragma unroll
      for (int rr = 0; rr < RB; ++rr)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[rr].v[m] = T(0);
      // RB + 28 window rows in chunks of CH, the next chunk's reads in flight during this one's FMAs
      // 4-row chunks: 0.543 against 0.565-0.573 ms for 8 (512^3 fp32, profiles/r2_nrm_ablation.txt)
      constexpr int NV = RB + 28, CH = 4, NCH = (NV + CH - 1) / CH;
      const T* rcol = ring + 4 * vg;
      // window row v sits at ring slot base + v, wrapped once at most: two bases (the second one ring
      // length back) and a per-row select, the row offset an immediate of the LDS read -- instead of
      // recomputing the wrapped slot and its address for every row (round 6)
      const T* rb0 = rcol + base * TP;
      const T* rb1 = rb0 - RING * TP;
      const int wrap = RING - base;  // the first window row past the ring's end
      Q4<T> w[2][CH];  // chunk c in w[c & 1] (static after unrolling: no register copies)
      auto rd = [&](int c, Q4<T>(&wc)[CH]) {
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int v = c * CH + j;
          if (v < NV) wc[j] = ldsq((v < wrap ? rb0 : rb1) + v * TP);
        }
      };
      rd(0, w[0]);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if (c + 1 < NCH) rd(c + 1, w[(c + 1) & 1]);
        nrm_fence();
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int v = c * CH + j;
          if (v < NV) {
#pragma unroll
            for (int rr = 0; rr < RB; ++rr) {
              const int qq = v - rr;
              if (qq >= 0 && qq < 29) nrm_fma4(acc[rr], av[qq < 14 ? 14 - qq : qq - 14], w[c & 1][j]);
            }
          }
        }
#pragma unroll
        for (int rr = 0; rr < RB; ++rr) nrm_pin(acc[rr]);
        nrm_fence();
      }
      const int gc = c0 + 4 * vg;
      // every thread issues RB stores per step (rows outside [a, b) dropped by the range check),
      // so the next step's wait for its staged rows leaves these stores in flight
      const Rsrc dst = rsrc_of(out + cur.plane * (int64_t)n1 * n2, (uint32_t)((int64_t)n1 * n2 * sizeof(T)));
      uint32_t offs[EP::kApgd ? RB : 1];
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) {
        const int i = cur.a - 28 + cur.s * RS + r0 + rr;
        const bool live = i >= cur.a && i < cur.b && gc < n2;
        if (live) {
          if (i < 7 || i >= n1 - 7) {  // the edge terms of the first / last 7 rows
            const bool top = i < 7;
            const int jr = top ? i : i - (n1 - 7), row0 = top ? 0 : n1 - 7;
            const T* e = top ? evl : evh;
            for (int c = 0; c < 7; ++c) {
              const Q4<T> w = ldsq(ring + ((row0 + c - cur.a + 14) % RING) * TP + 4 * vg);
              const T ec = e[8 * jr + c];
#pragma unroll
              for (int m = 0; m < 4; ++m) acc[rr].v[m] -= ec * w.v[m];
            }
          }
        }
        if constexpr (EP::kApgd) {
          offs[rr] = live ? (uint32_t)(((int64_t)i * n2 + gc) * sizeof(T)) : kOOB;
        } else {
          if constexpr (SUB) {
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[rr].v[m] = acc[rr].v[m] - bsub[rr].v[m];
          }
          nrm_bstore(dst, live ? (uint32_t)(((int64_t)i * n2 + gc) * sizeof(T)) : kOOB, acc[rr]);
        }
      }
      if constexpr (EP::kApgd) {
        const int64_t po = cur.plane * (int64_t)n1 * n2;
        const uint32_t nb = (uint32_t)((int64_t)n1 * n2 * sizeof(T));
        nrm_apgd_rows<T, RB>(ep, acc, offs, rsrc_of(in + po, nb), rsrc_of(sub + po, nb), rsrc_of(ep.aux + po, nb),
                             dst, rsrc_of(ep.aux_n + po, nb));
      }
    }
  };
  Q4<T> q[NL];
  Cur cur = task_at(t0);
  prefetch(cur, q);
  for (;;) {
    // the previous step's RB row stores may still be in flight (the APGD epilogue: its 2 RB stores, x' and aux',
    // issued after its 3 RB loads)
    stage(q, std::integral_constant<int, (EP::kApgd ? 2 : 1) * G::NST>{});
    Cur nxt = cur;
    bool more = true;
    if (cur.s + 1 < cur.ns) {
      nxt.s = cur.s + 1;
    } else {
      more = cur.t + t_stride < t_end;
      if (more) nxt = task_at(cur.t + t_stride);
    }
    prefetch(nxt, q);  // unconditional (the last step re-reads its own rows): the wait for these
                    // loads at the next step then leaves this step's stores in flight
    body(cur);
    if (!more) break;
    cur = nxt;
  }
  if constexpr (EP::kApgd) ep.finish();
}

// ---------------------------------------------------------------------------------------------
// k_sep2d_nrmm: the same two 29-tap passes on a MIRRORED ring (round 5).  The vertical window of a PV
// item spans RB + 28 ring rows; with the ring's first RB + 27 rows duplicated past its end (PH writes
// those rows twice) every window is contiguous, so its reads are one base address plus immediate
// offsets -- the old kernel recomputed a wrapped slot and its row offset for each of the 30 window rows
// (about 7 VALU per row pair, 227 VALU beside 232 FMAs in the fp64 PV block).  PV items are RB = 4 rows x
// one 16-B chunk (4 floats / 2 doubles): RB + 28 = 32 b128 reads per 4 x VN outputs (fp64: 4 reads per
// output instead of 7.5).  LDS layouts, all conflict-free in the lane-group model of MI355X_MICROARCH.md
// (ds_read_b128: 16-lane groups, 64 banks; ds_write_b128: 8-lane groups, 32 banks):
//   staged rows  pitch WI = the row's 4-column groups + 4 16-B slots, row r shifted by (r & 3) slots;
//                staging items in row-major order (fp32) / 8-lane groups of 4 groups x 2 rows (fp64)
//   PH items     lane l of wave w: row 8 w + (l & 7), item (l >> 3) & 7 of the row's 8 (4 PQ outputs, 4
//                chunks each): the 8 lanes of a write group hold 8 rows of one item column
//   ring         pitch TP = TX + one 16-B slot (an odd number of slots: those 8 rows hit 8 banks)
//   PV items     the 32 lanes of a half-wave read 32 consecutive chunks of one ring row
// one 16-B chunk from LDS as a single ds_read_b128 (volatile LDS access, as ldsq)
template <typename T>
__device__ __forceinline__ V16<T> nrm_ldsv(const T* p) {
  typedef unsigned int u4 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) const volatile u4* lds_u4;
  V16<T> r;
  const u4 v = *((lds_u4)(p));
  __builtin_memcpy(r.v, &v, 16);
  return r;
}

template <typename T>
struct NrmM {
  static constexpr int ES = sizeof(T), VN = 16 / ES;
  static constexpr int TX = ES == 4 ? 128 : 64, PQ = ES == 4 ? 4 : 2;  // 8 PH items of 4 chunks per row
  static constexpr int RS = 32, RB = 4, RING = RS + 28, MIR = RB + 27;
  static constexpr int GX = TX / 4, GI = GX + 8, GQ = GX / PQ, GV = TX / VN;
  static constexpr int NT = (RS / RB) * GV;
  static constexpr int WI = 4 * GI + 4 * VN;  // staged pitch (elements): the groups + 4 slots of shift room
  static constexpr int TP = TX + VN;          // ring pitch
  static constexpr int NIN = RS * GI, NL = (NIN + NT - 1) / NT;
  static constexpr int NTAB = 288;
  static_assert(GQ == 8 && NT == 256 && RS * GQ == NT && GI % 4 == 0, "one PH item per thread");
  static constexpr size_t lds_bytes() { return ES * ((size_t)RS * WI + (size_t)(RING + MIR) * TP + NTAB); }
  // staging item e -> staged row / 4-column group
  static __device__ __forceinline__ void stage_item(int e, int& rr, int& gg) {
    if constexpr (ES == 4) {
      rr = e / GI;
      gg = e - rr * GI;
    } else {
      const int e8 = e & 7, eh = e >> 3, q = eh / (GI / 4);
      rr = 2 * q + (e8 >> 2);
      gg = 4 * (eh - q * (GI / 4)) + (e8 & 3);
    }
  }
  static __device__ __forceinline__ int srow(int r) { return r * WI + (r & 3) * VN; }
};

template <typename T, bool SUB, class EP = NrmStore, class... EA>
__global__ __launch_bounds__(256, 2) void k_sep2d_nrmm(const T* __restrict__ in, T* __restrict__ out, int n1, int n2,
                                                       int nstrips, int nseg, int seg_len, int64_t ntasks,
                                                       const T* __restrict__ ha_, int ka, int offa,
                                                       const T* __restrict__ hb_, int kb, int offb,
                                                       const T* __restrict__ sub, EA... ea) {
  static_assert(SUB || !EP::kApgd, "the APGD epilogue subtracts Conv^T y");
  EP ep = nrm_policy<EP>(ea...);
  if constexpr (EP::kApgd) {
    if (ep.stopped()) return;
  }
  using G = NrmM<T>;
  constexpr int TX = G::TX, RS = G::RS, RB = G::RB, RING = G::RING, GV = G::GV, VN = G::VN, NT = G::NT,
                NL = G::NL, TP = G::TP, PQ = G::PQ;
  typedef unsigned int u4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* stg = reinterpret_cast<T*>(smem_raw);  // RS staged input rows (pitch WI, shifted)
  T* ring = stg + RS * G::WI;               // RING + MIR rows of the horizontal pass (pitch TP)
  T* tab = ring + (RING + G::MIR) * TP;     // NTAB
  const int tid = threadIdx.x;
  {
    __shared__ double hs[32];  // the two filters in fp64
    if (tid < 16) hs[tid] = tid < ka ? (double)ha_[tid] : 0.0;
    else if (tid < 32) hs[tid] = tid - 16 < kb ? (double)hb_[tid - 16] : 0.0;
    __syncthreads();
    for (int e = tid; e < G::NTAB; e += NT) {
      double v = 0.0;
      if (e < 64) {
        const int q = e & 31;
        const double* h = e < 32 ? hs : hs + 16;
        const int k = e < 32 ? ka : kb, off = e < 32 ? offa : offb;
        if (q < 29)
          for (int m = -7; m <= 7; ++m) v += nrm_tap(h, k, off, m) * nrm_tap(h, k, off, m + q - 14);
      } else {
        const int idx = e - 64, tb = idx / 56, r = idx - 56 * tb, j = r >> 3, c = r & 7;
        const double* h = tb < 2 ? hs : hs + 16;
        const int k = tb < 2 ? ka : kb, off = tb < 2 ? offa : offb;
        if (c < 7) {
          if ((tb & 1) == 0)  // rows / columns i = -7..-1 before the plane: E[j][c], j, c < 7
            for (int i = -7; i < 0; ++i) v += nrm_tap(h, k, off, i - j) * nrm_tap(h, k, off, i - c);
          else  // after it: j = n - 7 + jj, c = n - 7 + cc, i = n + ii
            for (int ii = 0; ii < 7; ++ii) v += nrm_tap(h, k, off, 7 + ii - j) * nrm_tap(h, k, off, 7 + ii - c);
        }
      }
      tab[e] = (T)v;
    }
    __syncthreads();
  }
  // the autocorrelation is symmetric: window tap q is a[|q - 14|], 15 registers per axis
  T av[15], ah[15];
#pragma unroll
  for (int e = 0; e < 15; ++e) {
    av[e] = tab[14 + e];
    ah[e] = tab[32 + 14 + e];
  }
  const T* evl = tab + 64;
  const T* evh = tab + 120;
  const T* ehl = tab + 176;
  const T* ehh = tab + 232;
  const XcdShare own = xcd_share(ntasks);  // XCD x owns a contiguous share of the task list (common.hpp)
  const int64_t t0 = own.t0, t_end = own.end, t_stride = own.stride;
  if (t0 >= t_end) {
    if constexpr (EP::kApgd) ep.finish();
    return;
  }
  struct Cur {
    int64_t t, plane;
    int strip, a, b, s, ns;
  };
  auto task_at = [&](int64_t t) {
    Cur c;
    c.t = t;
    const int64_t per_plane = (int64_t)nseg * nstrips;
    c.plane = t / per_plane;
    const int rem = (int)(t - c.plane * per_plane), seg = rem / nstrips;
    c.strip = rem - seg * nstrips;
    c.a = seg * seg_len;
    c.b = min(n1, c.a + seg_len);
    c.s = 0;
    c.ns = (c.b - c.a + 28 + RS - 1) / RS;
    return c;
  };
  // this thread's staging items (fixed): staged row / group and their LDS offsets
  int st_rr[NL], st_gg[NL], st_off[NL];
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    G::stage_item(min(l * NT + tid, G::NIN - 1), st_rr[l], st_gg[l]);
    st_off[l] = G::srow(st_rr[l]) + 4 * st_gg[l];
  }
  // staged rows of step s: input rows a - 14 + s RS + rr, columns c0 - 16 + 4 gg (0 outside)
  auto prefetch = [&](const Cur& c, Q4<T>(&q)[NL]) {
    const T* src = in + c.plane * (int64_t)n1 * n2;
    const int kmax = c.b - c.a + 27;  // last staged row any output of [a, b) reads
    const int gc0 = c.strip * TX - 16;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const int k = c.s * RS + st_rr[l], gi = c.a - 14 + k, gc = gc0 + 4 * st_gg[l];
      const bool ok = gi >= 0 && gi < n1 && k <= kmax && gc >= 0 && gc + 4 <= n2;
      const Q4<T> v = ldq(src + (ok ? (int64_t)gi * n2 + gc : 0));
#pragma unroll
      for (int m = 0; m < 4; ++m) q[l].v[m] = ok ? v.v[m] : T(0);
    }
  };
  // the staged rows have landed (WN: the memory ops issued after them that may stay in flight --
  // vector memory ops retire in order); rows -> LDS
  auto stage = [&](const Q4<T>(&q)[NL], auto waitn) {
    constexpr int WN = decltype(waitn)::value;
    __builtin_amdgcn_s_waitcnt((WN & 15) | ((WN >> 4) << 14) | (7 << 4) | (15 << 8));
#pragma unroll
    for (int l = 0; l < NL; ++l)
      if (l * NT + tid < G::NIN) stq(stg + st_off[l], q[l]);
  };
  // PH item: row pr, outputs 4 PQ pg .. + 4 PQ - 1 of the strip
  const int pr = ((tid >> 6) << 3) | (tid & 7), pg = PQ * ((tid >> 3) & 7);
  const T* psrow = stg + G::srow(pr);
  // PV item: rows RB vi .. + RB - 1 of the step, chunk vg (columns VN vg .. VN vg + VN - 1)
  const int vi = tid / GV, vg = tid - vi * GV, r0 = RB * vi;
  auto body = [&](const Cur cur) {
    const int c0 = cur.strip * TX;
    const int gc = c0 + VN * vg;
    V16<T> bsub[SUB && !EP::kApgd ? RB : 1];  // SUB: the PV outputs' sub values, loaded before PH (a phase to land)
    if constexpr (SUB && !EP::kApgd) {
      const Rsrc rs = rsrc_of(sub + cur.plane * (int64_t)n1 * n2, (uint32_t)((int64_t)n1 * n2 * sizeof(T)));
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) {
        const int i = cur.a - 28 + cur.s * RS + r0 + rr;
        const bool live = i >= cur.a && i < cur.b && gc < n2;
        const u4 d = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(live ? (uint32_t)(((int64_t)i * n2 + gc) * sizeof(T)) : kOOB), 0, 0);
        __builtin_memcpy(bsub[rr].v, &d, 16);
      }
    }
    lds_barrier();
    // ---- PH: t[row][c0 + j] = sum_q a_h[q] x[row][c0 + j - 14 + q] (staged column j + 2 + q)
    {
      T acc[4 * PQ];
#pragma unroll
      for (int o = 0; o < 4 * PQ; ++o) acc[o] = T(0);
#pragma unroll
      for (int u = 0; u < PQ + 8; ++u) {
        const Q4<T> v = ldsq(psrow + 4 * (pg + u));
#pragma unroll
        for (int ee = 0; ee < 4; ++ee)
#pragma unroll
          for (int o = 0; o < 4 * PQ; ++o) {
            const int qq = 4 * u + ee - o - 2;
            if (qq >= 0 && qq < 29) acc[o] += ah[qq < 14 ? 14 - qq : qq - 14] * v.v[ee];
          }
      }
      const int col = c0 + 4 * pg;
      if (col < 7 || col + 4 * PQ - 1 >= n2 - 7) {  // the edge terms of the first / last 7 columns
#pragma unroll
        for (int o = 0; o < 4 * PQ; ++o) {
          const int j = col + o;
          if (j < 7) {
            for (int c = 0; c < 7; ++c) acc[o] -= ehl[8 * j + c] * psrow[16 + c];
          } else if (j >= n2 - 7 && j < n2) {
            const int jj = j - (n2 - 7), s0 = n2 - 7 - c0 + 16;
            for (int c = 0; c < 7; ++c) acc[o] -= ehh[8 * jj + c] * psrow[s0 + c];
          }
        }
      }
      int slot = (cur.s * RS) % RING + pr;
      slot = slot >= RING ? slot - RING : slot;
      T* dst = ring + slot * TP + 4 * pg;
#pragma unroll
      for (int k = 0; k < 4 * PQ / VN; ++k) {
        V16<T> c;
#pragma unroll
        for (int e = 0; e < VN; ++e) c.v[e] = acc[k * VN + e];
        stv(dst + k * VN, c);
      }
      if (slot < G::MIR) {  // the ring's first RB + 27 rows again past its end
#pragma unroll
        for (int k = 0; k < 4 * PQ / VN; ++k) {
          V16<T> c;
#pragma unroll
          for (int e = 0; e < VN; ++e) c.v[e] = acc[k * VN + e];
          stv(dst + RING * TP + k * VN, c);
        }
      }
    }
    lds_barrier();
    // ---- PV: out row i = a - 28 + s RS + r0 + rr reads t rows i - 14 .. i + 14 (staged s RS + r0 + rr - 28 ..)
    {
      const int base = (cur.s * RS + r0 - 28 + RING) % RING;
      const T* rcol = ring + base * TP + VN * vg;  // window row j at rcol + j TP (contiguous: the mirror)
      V16<T> acc[RB];
#pragma unroll
      for (int rr = 0; rr < RB; ++rr)
#pragma unroll
        for (int m = 0; m < VN; ++m) acc[rr].v[m] = T(0);
      constexpr int NV = RB + 28, CH = 4, NCH = NV / CH;
      static_assert(NV % CH == 0, "whole chunks");
      V16<T> w[2][CH];  // chunk c in w[c & 1]; the next chunk's reads in flight during this one's FMAs
      auto rd = [&](int c, V16<T>(&wc)[CH]) {
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          wc[j] = nrm_ldsv(rcol + (c * CH + j) * TP);
        }
      };
      rd(0, w[0]);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if (c + 1 < NCH) rd(c + 1, w[(c + 1) & 1]);
        nrm_fence();
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int v = c * CH + j;
#pragma unroll
          for (int rr = 0; rr < RB; ++rr) {
            const int qq = v - rr;
            if (qq >= 0 && qq < 29) {
              const T h = av[qq < 14 ? 14 - qq : qq - 14];
#pragma unroll
              for (int m = 0; m < VN; ++m) acc[rr].v[m] += h * w[c & 1][j].v[m];
            }
          }
        }
#pragma unroll
        for (int rr = 0; rr < RB; ++rr)
#pragma unroll
          for (int m = 0; m < VN; ++m) asm volatile("" : "+v"(acc[rr].v[m]));
        nrm_fence();
      }
      // every thread issues RB stores per step (rows outside [a, b) dropped by the range check),
      // so the next step's wait for its staged rows leaves these stores in flight
      const Rsrc dst = rsrc_of(out + cur.plane * (int64_t)n1 * n2, (uint32_t)((int64_t)n1 * n2 * sizeof(T)));
      uint32_t offs[EP::kApgd ? RB : 1];
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) {
        const int i = cur.a - 28 + cur.s * RS + r0 + rr;
        const bool live = i >= cur.a && i < cur.b && gc < n2;
        if (live && (i < 7 || i >= n1 - 7)) {  // the edge terms of the first / last 7 rows
          const bool top = i < 7;
          const int jr = top ? i : i - (n1 - 7), row0 = top ? 0 : n1 - 7;
          const T* e = top ? evl : evh;
          for (int c = 0; c < 7; ++c) {
            const V16<T> wv = ldv(ring + ((row0 + c - cur.a + 14) % RING) * TP + VN * vg);
            const T ec = e[8 * jr + c];
#pragma unroll
            for (int m = 0; m < VN; ++m) acc[rr].v[m] -= ec * wv.v[m];
          }
        }
        if constexpr (EP::kApgd) {
          offs[rr] = live ? (uint32_t)(((int64_t)i * n2 + gc) * sizeof(T)) : kOOB;
        } else {
          if constexpr (SUB) {
#pragma unroll
            for (int m = 0; m < VN; ++m) acc[rr].v[m] = acc[rr].v[m] - bsub[rr].v[m];
          }
          u4 d;
          __builtin_memcpy(&d, acc[rr].v, 16);
          __builtin_amdgcn_raw_buffer_store_b128(d, dst, (int)(live ? (uint32_t)(((int64_t)i * n2 + gc) * sizeof(T)) : kOOB), 0, 0);
        }
      }
      if constexpr (EP::kApgd) {
        const int64_t po = cur.plane * (int64_t)n1 * n2;
        const uint32_t nb = (uint32_t)((int64_t)n1 * n2 * sizeof(T));
        nrm_apgd_rows<T, RB>(ep, acc, offs, rsrc_of(in + po, nb), rsrc_of(sub + po, nb), rsrc_of(ep.aux + po, nb),
                             dst, rsrc_of(ep.aux_n + po, nb));
      }
    }
  };
  auto advance = [&](const Cur& c, bool& more) {  // the step after c (more = false: none)
    Cur n = c;
    more = true;
    if (c.s + 1 < c.ns) {
      n.s = c.s + 1;
    } else {
      more = c.t + t_stride < t_end;
      if (more) n = task_at(c.t + t_stride);
    }
    return n;
  };
  Q4<T> q[NL];
  Cur cur = task_at(t0);
  prefetch(cur, q);
  for (;;) {
    // the previous step's RB row stores may still be in flight (with SUB the wait also covers its RB
    // sub loads, issued before the stores; the APGD epilogue: its 2 RB stores, after its 3 RB loads)
    stage(q, std::integral_constant<int, (EP::kApgd ? 2 : 1) * RB>{});
    bool more;
    const Cur nxt = advance(cur, more);
    prefetch(nxt, q);  // unconditional (the last step re-reads its own rows): the wait for these
                       // loads at the next step then leaves this step's stores in flight
    body(cur);
    if (!more) break;
    cur = nxt;
  }
  if constexpr (EP::kApgd) ep.finish();
}

// ---- host side, shared by the launchers
template <typename T>
inline size_t nrm_lds() {
  if constexpr (sizeof(T) == 8) return NrmM<T>::lds_bytes();
  else return NrmF::lds_bytes();
}

// the two-pass kernels take taps reaching <= 7 samples either side (any centred filter of <= 15 taps) on
// planes of >= 16 x 16 whose rows are whole 16-B groups
inline bool nrm_takes(int64_t n1, int64_t n2, int ka, int offa, int kb, int offb) {
  return n1 >= 16 && n2 >= 16 && n2 % 4 == 0 && offa <= 7 && ka - 1 - offa <= 7 && offb <= 7 && kb - 1 - offb <= 7;
}

// Tasks of a launch over np planes of n1 x n2: (plane, row segment, strip).  Row segments: the fewest (each
// task re-reads a 28-row prologue) whose tasks fill the resident workgroup slots once, segments of >= 64
// rows; then one task per workgroup, later workgroups starting as earlier ones finish.  Against the
// resident grid (a contiguous run of tasks per workgroup, segments by a waves x rows cost): 512^3 fp32 0.49
// against 0.57-0.58 ms, 1024^3 fp64 5.96 (4 tasks per workgroup) against 7.33-7.44 ms, 4096^2 fp64 0.113
// either way (profiles/r4_nrm_slots_sweep*.txt)
struct NrmGrid {
  int64_t nstrips, nseg, seg_len, ntasks;
};
template <typename T>
inline NrmGrid nrm_grid(int64_t np, int64_t n1, int64_t n2, int64_t slots) {
  constexpr int TX = sizeof(T) == 8 ? NrmM<T>::TX : NrmF::TX;
  NrmGrid g;
  g.nstrips = (n2 + TX - 1) / TX;
  const int64_t pieces = np * g.nstrips;
  const int64_t max_seg = n1 / 64 > 1 ? n1 / 64 : 1;
  int64_t nseg = 1;
  while (nseg < max_seg && pieces * nseg < slots) ++nseg;
  g.seg_len = (n1 + nseg - 1) / nseg;
  g.nseg = (n1 + g.seg_len - 1) / g.seg_len;
  g.ntasks = pieces * g.nseg;
  return g;
}

}  // namespace pcs
