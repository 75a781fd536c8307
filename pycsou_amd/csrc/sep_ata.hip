// In-plane normal operator of a separable 3-D blur, every plane in one pass:
//
//   out = C_a^T C_b^T C_b C_a in        (C_a: Convolve1D along axis 1, C_b: along axis 2)
//
// i.e. the in-plane half of grad F = C^T (C x - y) for the reference's 3-D deconvolution
// (pycsou/linop/conv.py:20-164 per axis; residual and adjoint of core/map.py:609-610).  The
// axis-0 pass commutes with the in-plane ones, so the 3-D engine computes
//   g = C_0^T (C_0 (C_12^T C_12 x) - C_12^T y)
// with C_12^T y formed once at setup: two sub-volume passes per iteration (this kernel, then
// pcs_conv0_residual_adjoint) instead of three, 5 words per voxel of traffic instead of 7.
//
// Four 15-tap passes per plane, marched down a 128-column strip 32 rows per step:
//   P1  horizontal conv  (staging  -> ring A, 144 columns: the strip + the reach of P4)
//   P2  vertical conv    (ring A   -> ring B, rows outside the image forced to 0)
//   P3  vertical corr    (ring B   -> P3 rows, aliasing the staging buffer)
//   P4  horizontal corr  (P3 rows  -> HBM, the strip's 128 columns)
// Rings hold 48 rows (the 14-row reach of the vertical passes above a step), so no row is
// filtered twice; a strip's horizontal halo (16 columns) is recomputed by P1-P3 (1.125x).
// Zero boundary: input outside the plane reads 0, and P1 / P2 outputs outside the plane
// are 0 (the truncation between C and C^T).  Taps are zero-padded to 15 (out[j] =
// sum_t h'[t] in[j + o - t], h'[t] = h[t - pad], o = off + pad); the adjoint passes use
// h'[14 - t] with offset 14 - o.  Persistent grid, tasks (plane, row segment, strip) with the
// strip fastest and an XCD-aware task map, as k_sep2d_march.
#include <cstring>
#include <type_traits>

#include "sep_nrm.hpp"
#include "vecio.hpp"

namespace pcs {

struct AtaG {
  static constexpr int KT = 15, TX = 128, GX = TX / 4, GE = GX + 4, WE = 4 * GE, GI = GE + 4, WI = 4 * GI;
  static constexpr int RS = 32, RING = 48, NT = 576;
  static constexpr int NIN = RS * GI, NL = (NIN + NT - 1) / NT;  // staging loads per thread
  static constexpr int NP1 = RS * GE, NP4 = RS * GX;             // P1 / P4 items
  static_assert((RS / 2) * GE == NT, "at most one vertical item (2 or 4 rows x 4 columns) per thread");
  static_assert(RING >= RS + KT - 1, "ring holds the 14 rows above a step");
};

// rows per vertical item
#ifndef PCS_ATA_RB
#define PCS_ATA_RB 2
#endif

// one vertical 15-tap pass over a ring of rows: acc[r] = sum_t h(t) ring[(base + r0 + r - t) mod RING]
// at 4-column group q, h(t) = hv[t] (conv) or hv[14 - t] (FLIP: correlation); each of the RB + 14
// ring rows is read once
template <typename T, int RB, bool FLIP>
__device__ __forceinline__ void vert_pass(const T* ring, int base, int r0, int q, const T* hv, Q4<T> (&acc)[RB]) {
  using A = AtaG;
  constexpr int KT = A::KT, RING = A::RING, WE = A::WE;
#pragma unroll
  for (int r = 0; r < RB; ++r)
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[r].v[m] = T(0);
#pragma unroll 2
  for (int j = 0; j < KT - 1 + RB; ++j) {  // ring rows base + r0 - 14 + j
    int slot = base + r0 - (KT - 1) + j;
    slot = slot < 0 ? slot + RING : (slot >= RING ? slot - RING : slot);
    const Q4<T> v = ldsq(ring + slot * WE + 4 * q);
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int t = r + KT - 1 - j;
      if (t >= 0 && t < KT) {
        const T h = FLIP ? hv[KT - 1 - t] : hv[t];
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[r].v[m] += h * v.v[m];
      }
    }
  }
}

template <typename T, int SH4>
__global__ __launch_bounds__(AtaG::NT) void k_sep2d_ata(const T* __restrict__ in, T* __restrict__ out, int n1, int n2,
                                                         int nstrips, int nseg, int seg_len, int64_t ntasks,
                                                         const T* __restrict__ ha_, int ka, const T* __restrict__ hb_,
                                                         int kb, int o1, int padb, int o2) {
  using A = AtaG;
  constexpr int KT = A::KT, TX = A::TX, GE = A::GE, WE = A::WE, WI = A::WI, GI = A::GI, RS = A::RS, RING = A::RING,
                NT = A::NT, NL = A::NL;
  constexpr int SH1 = 2 - SH4;  // P1's window shift: the staged input starts 16 columns left of the strip
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* stg = reinterpret_cast<T*>(smem_raw);  // RS x WI input rows; P3 rows (RS x WE) after P1
  T* ringA = stg + RS * WI;                 // RING x WE
  T* ringB = ringA + RING * WE;             // RING x WE
  // taps in LDS (broadcast reads, re-read per phase): 30 fp64 taps in registers spill at the
  // 168-VGPR budget of 9 waves per workgroup.  hv: [0, 15), hh: [16, 31)
  T* hv = ringB + RING * WE;
  T* hh = hv + 16;
  if (threadIdx.x < 16) {
    const int t = threadIdx.x;
    hv[t] = t < ka ? ha_[t] : T(0);
    hh[t] = (t >= padb && t - padb < kb) ? hb_[t - padb] : T(0);
  }
  const XcdShare own = xcd_share(ntasks);  // XCD x owns a contiguous share of the task list (common.hpp)
  const int64_t t0 = own.t0, t_end = own.end, t_stride = own.stride;
  if (t0 >= t_end) return;
  const int tid = threadIdx.x;
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
    c.ns = (c.b - c.a + 2 * (KT - 1) + RS - 1) / RS;
    return c;
  };
  Q4<T> q[NL];
  // staging rows of step c: input rows L1 + s RS + r (L1 = a - 14), columns c0 - 16 + 4 g
  auto prefetch = [&](const Cur& c) {
    const T* src = in + c.plane * (int64_t)n1 * n2;
    const int kmax = c.b - c.a + 2 * (KT - 1) - 1;  // last staged row any output of [a, b) needs
    const int gc0 = c.strip * TX - 16;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const int e = min(l * NT + tid, A::NIN - 1);
      const int rr = e / GI, g = e - rr * GI;
      const int k = c.s * RS + rr, gi = c.a - (KT - 1) + k, gc = gc0 + 4 * g;
      const bool ok = gi >= 0 && gi < n1 && k <= kmax && gc >= 0 && gc + 4 <= n2;
      const Q4<T> v = ldq(src + (ok ? (int64_t)gi * n2 + gc : 0));
#pragma unroll
      for (int m = 0; m < 4; ++m) q[l].v[m] = ok ? v.v[m] : T(0);
    }
  };
  Cur cur = task_at(t0);
  prefetch(cur);
  constexpr int RB = PCS_ATA_RB, NV = (RS / RB) * GE;  // vertical items: RB rows x one 4-column group
  const int vrb = tid / GE, vq = tid - (tid / GE) * GE;  // vertical item: rows RB vrb .. + RB - 1; group vq
  for (;;) {
    lds_barrier();  // the previous step's P4 is done with the P3 rows (staging)
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const int e = l * NT + tid;
      if (e < A::NIN) stq(stg + 4 * e, q[l]);
    }
    Cur nxt = cur;
    bool more = true;
    if (cur.s + 1 < cur.ns) {
      nxt.s = cur.s + 1;
    } else {
      more = cur.t + t_stride < t_end;
      if (more) nxt = task_at(cur.t + t_stride);
    }
    if (more) prefetch(nxt);
    const int c0 = cur.strip * TX;
    const int e0 = c0 - o2 - SH4;  // first P1 column (E0, a multiple of 4); E0 + WE covers P4's reach
    const int base = (cur.s * RS) % RING;  // ring slot of the step's first row
    lds_barrier();
    // ---- P1: horizontal conv of the RS staged rows, columns [E0, E0 + WE) -> ring A
#pragma unroll 1
    for (int l = 0; l < (A::NP1 + NT - 1) / NT; ++l) {
      const int e = l * NT + tid;
      if (e < A::NP1) {
        const int r = e / GE, g = e - r * GE;
        T w[20];
#pragma unroll
        for (int u = 0; u < 5; ++u) {
          const Q4<T> v = ldsq(stg + r * WI + 4 * (g + u));
#pragma unroll
          for (int m = 0; m < 4; ++m) w[4 * u + m] = v.v[m];
        }
        Q4<T> o;
        const int col = e0 + 4 * g;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          T acc = T(0);
#pragma unroll
          for (int t = 0; t < KT; ++t) acc += hh[t] * w[SH1 + m + (KT - 1 - t)];
          o.v[m] = (unsigned)(col + m) < (unsigned)n2 ? acc : T(0);
        }
        int slot = base + r;
        slot = slot >= RING ? slot - RING : slot;
        stq(ringA + slot * WE + 4 * g, o);
      }
    }
    lds_barrier();
    // ---- P2: vertical conv, P2 row (rel. L1 - o1) s RS + r reads ring A rows s RS + r - t
    if (tid < NV) {
      Q4<T> acc[RB];
      vert_pass<T, RB, false>(ringA, base, RB * vrb, vq, hv, acc);
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int row = cur.a - (KT - 1) - o1 + cur.s * RS + RB * vrb + r;  // image row of this P2 output
        if ((unsigned)row >= (unsigned)n1) {
#pragma unroll
          for (int m = 0; m < 4; ++m) acc[r].v[m] = T(0);
        }
        int slot = base + RB * vrb + r;
        slot = slot >= RING ? slot - RING : slot;
        stq(ringB + slot * WE + 4 * vq, acc[r]);
      }
    }
    lds_barrier();
    // ---- P3: vertical correlation (taps hv[14 - t], offset 14 - o1): P3 row s RS + r (rel.
    // a - 28) reads ring B rows s RS + r - t -> P3 rows in the staging buffer (pitch WE)
    if (tid < NV) {
      Q4<T> acc[RB];
      vert_pass<T, RB, true>(ringB, base, RB * vrb, vq, hv, acc);
#pragma unroll
      for (int r = 0; r < RB; ++r) stq(stg + (RB * vrb + r) * WE + 4 * vq, acc[r]);
    }
    lds_barrier();
    // ---- P4: horizontal correlation (taps hh[14 - t], offset 14 - o2) -> output row
    // a - 28 + s RS + r, columns c0 + 4 g .. + 3
    {
      T* dst = out + cur.plane * (int64_t)n1 * n2;
#pragma unroll 1
      for (int l = 0; l < (A::NP4 + NT - 1) / NT; ++l) {
        const int e = l * NT + tid;
        if (e < A::NP4) {
          const int r = e / A::GX, g = e - r * A::GX;
          const int row = cur.a - 2 * (KT - 1) + cur.s * RS + r, gc = c0 + 4 * g;
          T w[20];
#pragma unroll
          for (int u = 0; u < 5; ++u) {
            const Q4<T> v = ldsq(stg + r * WE + 4 * (g + u));
#pragma unroll
            for (int m = 0; m < 4; ++m) w[4 * u + m] = v.v[m];
          }
          Q4<T> o;
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            T acc = T(0);
#pragma unroll
            for (int s = 0; s < KT; ++s) acc += hh[s] * w[SH4 + m + s];
            o.v[m] = acc;
          }
          if (row >= cur.a && row < cur.b && gc < n2) stq(dst + (int64_t)row * n2 + gc, o);
        }
      }
    }
    if (!more) break;
    cur = nxt;
  }
}

template <typename T>
static size_t ata_lds_bytes() {
  using A = AtaG;
  return sizeof(T) * (size_t)(A::RS * A::WI + 2 * A::RING * A::WE + 32);
}

// the kernel's LDS (> 64 KB) is dynamic: raise the function's limit once per instantiation
template <typename T, int SH4>
static void ata_attr() {
  static bool done = false;
  if (!done) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sep2d_ata<T, SH4>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)ata_lds_bytes<T>());
    (void)hipGetLastError();
    done = true;
  }
}

// resident workgroups of k_sep2d_ata<T> on the device (queried once per type)
template <typename T>
static int ata_slots() {
  static const int slots = [] {
    ata_attr<T, 1>();
    const Occupancy o = occupancy(k_sep2d_ata<T, 1>, AtaG::NT, ata_lds_bytes<T>(), 1);
    return env_override("PCS_ATA_SLOTS", o.cus * o.per_cu);
  }();
  return slots;
}

// horizontal tap padding that makes both horizontal windows fit the strip layout: the padded
// offset o2 = offb + pad must satisfy o2 % 4 != 1 (SH4 = (-o2) mod 4 <= 2); -1 if none exists
static int ata_padb(int kb, int offb) {
  for (int pad = 0; pad <= AtaG::KT - kb; ++pad)
    if ((offb + pad) % 4 != 1) return pad;
  return -1;
}

// ---------------------------------------------------------------------------------------------
// The same operator as TWO 29-tap passes (the default when the taps reach <= 7 samples either side and the
// plane is >= 16 x 16): the kernels k_sep2d_nrm / k_sep2d_nrmm live in sep_nrm.hpp, shared with apgd2d.hip.
// fp32: k_sep2d_nrm (53 KB of LDS, 3 workgroups / CU); fp64: k_sep2d_nrmm (77 KB, 2 / CU).  The mirrored ring
// in fp32 needs 72 KB (2 / CU) and measured slower there: 512^3 0.41-0.48 against 0.36-0.43 ms, 4096^2 equal;
// in fp64 it took 1024^3 from 5.19-5.22 to 4.59-4.67 ms, 4096^2 from 0.108-0.111 to 0.098-0.100 ms (bitwise the
// same output; loading two steps ahead: no further change, profiles/r5_nrm_ab.txt)
template <typename T, bool SUB>
static const void* nrm_fn() {
  if constexpr (sizeof(T) == 8) return reinterpret_cast<const void*>(&k_sep2d_nrmm<T, SUB>);
  else return reinterpret_cast<const void*>(&k_sep2d_nrm<T, SUB>);
}
template <typename T, bool SUB>
static void nrm_attr() {
  static bool done = false;
  if (!done) {
    (void)hipFuncSetAttribute(nrm_fn<T, SUB>(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)nrm_lds<T>());
    (void)hipGetLastError();
    done = true;
  }
}

template <typename T>
static int nrm_slots() {
  static const int slots = [] {
    nrm_attr<T, false>();
    const Occupancy o = occupancy(nrm_fn<T, false>(), 256, nrm_lds<T>(), 1);
    return env_override("PCS_ATA_SLOTS", o.cus * o.per_cu);
  }();
  return slots;
}

// the two-pass kernel takes taps reaching <= 7 samples either side (any centred filter of
// <= 15 taps) on planes of >= 16 x 16; PCS_ATA_KERNEL=4pass pins the four-pass kernel (diagnostics)
static bool nrm_fits(int64_t n1, int64_t n2, int ka, int offa, int kb, int offb) {
  const char* e = getenv("PCS_ATA_KERNEL");
  if (e && strcmp(e, "4pass") == 0) return false;
  return nrm_takes(n1, n2, ka, offa, kb, offb);
}

template <typename T>
static int sep_nrm(const void* in, void* out, int64_t np, int64_t n1, int64_t n2, const void* ha, int ka, int offa,
                   const void* hb, int kb, int offb, hipStream_t st, const void* sub = nullptr) {
  if (np == 0) return PCS_OK;
  const int64_t slots = nrm_slots<T>();
  const NrmGrid gr = nrm_grid<T>(np, n1, n2, slots);
  const int64_t nstrips = gr.nstrips, nseg = gr.nseg, seg_len = gr.seg_len, ntasks = gr.ntasks;
  // PCS_NRM_GRIDX=k (diagnostics): k x the resident slots, each workgroup a contiguous run of tasks
  static int gridx = -1;
  if (gridx < 0) {
    const char* e = getenv("PCS_NRM_GRIDX");
    gridx = e && atoi(e) > 0 ? atoi(e) : 0;
  }
  const int64_t gslots = gridx > 0 ? slots * gridx : ntasks;
  const int64_t grid = ntasks < gslots ? ntasks : gslots;
  const size_t lds = nrm_lds<T>();
  auto go = [&](auto kern) {
    kern<<<(unsigned)grid, 256, lds, st>>>((const T*)in, (T*)out, (int)n1, (int)n2, (int)nstrips, (int)nseg,
                                           (int)seg_len, ntasks, (const T*)ha, ka, offa, (const T*)hb, kb, offb,
                                           (const T*)sub);
  };
  if (sub != nullptr) {
    nrm_attr<T, true>();
    if constexpr (sizeof(T) == 8) go(k_sep2d_nrmm<T, true>);
    else go(k_sep2d_nrm<T, true>);
  } else {
    nrm_attr<T, false>();
    if constexpr (sizeof(T) == 8) go(k_sep2d_nrmm<T, false>);
    else go(k_sep2d_nrm<T, false>);
  }
  return launch_status();
}

template <typename T>
static int sep_ata(const void* in, void* out, int64_t np, int64_t n1, int64_t n2, const void* ha, int ka, int offa,
                   const void* hb, int kb, int offb, hipStream_t st) {
  using A = AtaG;
  if (!in || !out || !ha || !hb || np < 0 || n1 < 1 || n2 < 1 || ka < 1 || ka > A::KT || kb < 1 || kb > A::KT ||
      offa < 0 || offa >= ka || offb < 0 || offb >= kb || in == out)
    return PCS_EINVAL;
  if ((uintptr_t)in % 16 || (uintptr_t)out % 16) return PCS_EINVAL;
  if (nrm_fits(n1, n2, ka, offa, kb, offb) && n1 * n2 * (int64_t)sizeof(T) < (1LL << 30))
    return sep_nrm<T>(in, out, np, n1, n2, ha, ka, offa, hb, kb, offb, st);
  const int padb = ata_padb(kb, offb);
  if (padb < 0 || n2 % 4 != 0 || n1 >= (1LL << 30) || n2 >= (1LL << 30)) return PCS_EUNSUPPORTED;
  if (np == 0) return PCS_OK;
  const int o2 = offb + padb, sh4 = (4 - o2 % 4) % 4;
  const int64_t nstrips = (n2 + A::TX - 1) / A::TX, pieces = np * nstrips;
  const int64_t slots = ata_slots<T>();
  // row segments: the count minimising (waves of resident workgroups) x (rows per task + the
  // 28-row prologue of the two vertical passes), segments of >= 64 rows
  const int64_t max_seg = n1 / 64 > 1 ? n1 / 64 : 1;
  int64_t nseg = 1, best = -1;
  for (int64_t c = 1; c <= max_seg; ++c) {
    const int64_t len = (n1 + c - 1) / c, waves = (pieces * c + slots - 1) / slots;
    const int64_t cost = waves * (len + 2 * (A::KT - 1));
    if (best < 0 || cost < best) {
      best = cost;
      nseg = c;
    }
  }
  const int64_t seg_len = (n1 + nseg - 1) / nseg;
  nseg = (n1 + seg_len - 1) / seg_len;
  const int64_t ntasks = pieces * nseg;
  const int64_t grid = ntasks < slots ? ntasks : slots;
  const size_t lds = ata_lds_bytes<T>();
  auto go = [&](auto kern) {
    kern<<<(unsigned)grid, A::NT, lds, st>>>((const T*)in, (T*)out, (int)n1, (int)n2, (int)nstrips, (int)nseg,
                                             (int)seg_len, ntasks, (const T*)ha, ka, (const T*)hb, kb, offa, padb, o2);
  };
  switch (sh4) {
    case 0: ata_attr<T, 0>(); go(k_sep2d_ata<T, 0>); break;
    case 1: ata_attr<T, 1>(); go(k_sep2d_ata<T, 1>); break;
    default: ata_attr<T, 2>(); go(k_sep2d_ata<T, 2>); break;
  }
  return launch_status();
}

}  // namespace pcs

using namespace pcs;

namespace pcs {
// N x - sub by the two-pass kernel (the fp64 2-D march's gradient buffer, pds.hip); PCS_EUNSUPPORTED when
// the two-pass kernel does not take the taps / layout (the caller then forms N x and subtracts in the step)
int sep_normal_minus(int dt, const void* in, void* out, const void* sub, int64_t np, int64_t n1, int64_t n2,
                     const void* ha, int ka, int offa, const void* hb, int kb, int offb, hipStream_t st) {
  if (!in || !out || !sub || !ha || !hb || np < 0 || n1 < 1 || n2 < 1 || in == out || sub == out) return PCS_EINVAL;
  // a buffer off the 16-B grid is a layout this kernel does not take: the caller's fallback (N x, then the
  // subtraction inside the step) runs it
  if ((uintptr_t)in % 16 || (uintptr_t)out % 16 || (uintptr_t)sub % 16) return PCS_EUNSUPPORTED;
  const int64_t esz = dt == PCS_F64 ? 8 : 4;
  if (!nrm_fits(n1, n2, ka, offa, kb, offb) || n1 * n2 * esz >= (1LL << 30)) return PCS_EUNSUPPORTED;
  if (np == 0) return PCS_OK;
  if (dt == PCS_F32) return sep_nrm<float>(in, out, np, n1, n2, ha, ka, offa, hb, kb, offb, st, sub);
  if (dt == PCS_F64) return sep_nrm<double>(in, out, np, n1, n2, ha, ka, offa, hb, kb, offb, st, sub);
  return PCS_EINVAL;
}
}  // namespace pcs

extern "C" {

int pcs_conv2d_sep_ata_planes(int dt, const void* in, void* out, int64_t nplanes, int64_t n1, int64_t n2,
                              const void* ha, int ka, int offa, const void* hb, int kb, int offb, hipStream_t st) {
  if (dt == PCS_F32) return sep_ata<float>(in, out, nplanes, n1, n2, ha, ka, offa, hb, kb, offb, st);
  if (dt == PCS_F64) return sep_ata<double>(in, out, nplanes, n1, n2, ha, ka, offa, hb, kb, offb, st);
  return PCS_EINVAL;
}

}  // extern "C"
