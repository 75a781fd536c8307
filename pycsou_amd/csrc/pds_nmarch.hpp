// Row-marching fused 2-D PDS iteration through the NORMAL operator of the separable blur
// (fp32, tiers H = 3 / 7): grad F = Conv^T (Conv x - y) = N x - b with
//   N = Conv^T Conv = N_v (x) N_h        (the column and row passes commute, so N factors)
//   b = Conv^T y                          (formed once per problem by the host: pcs_pds2d_args.cty)
// so an iteration applies two (4H+1)-tap passes instead of four (2H+1)-tap passes, with no
// residual ring and one LDS round trip per pass.  Away from the image edges N_v / N_h are the
// autocorrelation of the taps; on the H rows (columns) nearest an edge the zero-boundary
// truncation between Conv and Conv^T changes the window taps -- the host tables
// (pcs_pds2d_args.ntaps, below) hold the exact rows of N there.  Same update as the 4-pass
// march kernel (pds_march.hpp); the iterates differ from it only by fp32 rounding.
//
// One workgroup (256 threads: 4 rows x 16 column groups per wave) owns a 64-column strip of a row
// segment [s0, s1) (strips on 256-B boundaries) and marches down it 16 rows per step; each item
// also computes the column after its 4 (t, g, u): the strip's 65th column, whose u K u of the 64th
// needs, comes from the last group's fifth column:
//   top   land z of this step (loaded during the previous one); issue the next step's loads:
//         x rows [a+2H+17, a+2H+33), b rows [a+17, a+33), z rows [a+16, a+33)
//   PH    t = N_h x on rows [a+2H+1, a+2H+17)           x ring (32 rows) -> t ring (64 rows)
//   PV    g = N_v t - b on rows [a+1, a+17); x_t = prox_G(x - tau g - tau K^T z),
//         u = 2 x_t - x -> u ring, x' = rho x_t + (1 - rho) x
//   P6    z' = rho fenchel(z + sigma K u) + (1 - rho) z on rows [a, a+16)
//         park the next step's x rows in the x ring
// Three barriers per step (the 4-pass kernel has five).
//
// ntaps (fp32, 64 + 32 H values): [0, 32) N_v window taps tv[q] (q = 0..4H: row r - 2H + q) =
// the autocorrelation of the axis-0 taps, [32, 64) the same along axis 1, then the truncation
// corrections E (H x 8 each, N = window - E on the edge band): E_v for rows 0..H-1 against rows
// 0..H-1, E_v for rows n0-H+j against rows n0-H+k, E_h for columns 0..H-1, E_h for the last H.
// Reference: PrimalDualSplitting.update_iterand, pycsou/opt/proxalgs.py:343-355, with
// grad F = Conv^T((2 (Conv x - y)) 0.5) (core/map.py:609-610), Conv from
// pycsou/linop/conv.py:167-295.
#pragma once
// waves per SIMD the register budget targets (diagnostics builds override)
#ifndef PCS_NM_WPE
#define PCS_NM_WPE 3
#endif
// window rows per PV read chunk (2 chunks in flight)
#ifndef PCS_NM_PF
#define PCS_NM_PF 2
#endif
// cache-policy bits of the x' / z' stores (16 = sc1: written through, not left dirty in L2)
// C2 2048^2: 31.4 against 32.3 us per iteration, C3 4096^2: 112.7 against 113.9 us (two alternating
// reps each, profiles/r3_store_policy_ab.txt)
#ifndef PCS_NM_SAUX
#define PCS_NM_SAUX 16
#endif

#include <type_traits>

#include "pds_march.hpp"
#include "stencil.hpp"

namespace pcs {

// compiler-only fence: no memory access (LDS reads included) moves across it, at IR or MIR level
// (bounds the reads in flight, hence the registers they occupy); emits no instruction
__device__ __forceinline__ void pcs_fence() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// the value is live (computed) at this point: arithmetic is not sunk past it
__device__ __forceinline__ void pin4(G4<float>& g) {
  asm volatile("" : "+v"(g.v[0]), "+v"(g.v[1]), "+v"(g.v[2]), "+v"(g.v[3]));
}

__device__ __forceinline__ void pin1(float& v) { asm volatile("" : "+v"(v)); }

// one LDS float (a volatile read: never widened or merged with its neighbours)
__device__ __forceinline__ float lds1(const float* p) {
  typedef __attribute__((address_space(3))) const volatile float* lds_f1;
  return *(lds_f1)(p);
}

// s_waitcnt vmcnt(N) alone (expcnt / lgkmcnt left at their maxima)
template <int N>
__device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N < 64, "vmcnt");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

// cache-policy bits of the march's steady-state x / z / b loads (0: default; 2 = nt, streaming: measured
// 113.6-115.9 against 109.9-112.2 us on C3, no change on the centred-K C3, profiles/r3_ck38_nt_*ab.txt)
#ifndef PCS_NM_LAUX
#define PCS_NM_LAUX 0
#endif
template <int AUX>
__device__ __forceinline__ G4<float> bload4a(Rsrc r, uint32_t off) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, AUX);
  return {{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])}};
}

// sum over the 16-lane DPP row holding the lane (every lane of the row gets the sum; the lanes of a
// row add in different orders, so only one lane's value is used): row_ror 8, 4, 2, 1
__device__ __forceinline__ float row_sum16(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xf, 0xf, false));
  return v;
}

// sum over the 8-lane group holding the lane (lanes 8 g .. 8 g + 7) by DPP (quad_perm xor 1, xor 2,
// row_half_mirror: VALU latency); every lane gets the same value, the sums of __shfl_xor by 1, 2, 4 bit for bit
// (fp addition commutes, and after the quad steps a quad holds one value)
__device__ __forceinline__ float oct_sum8(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));   // [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false));   // [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false));  // half mirror
  return v;
}

// GEN: backward / centred K (KK != PCS_FORWARD) -- K^T z reads z rows lr - 1 .. lr + 1 and columns
// c - 1 .. c + 1, K u reads u rows r - 1 .. r + 1 and columns c - 1 .. c + 1: z tiles of 18 rows (the
// z0 tile from column c0 - 4 too), an 18-row u ring, and a sixth u / t / g column c0 - 1 (group 0,
// slot SLM1 of the t and u rows) beside the 65th
template <int H, bool GEN = false>
struct NMarch {
  static constexpr int TW = 64, TS = 16, NQ = 4 * H + 1;
  static constexpr int XL = RU4<2 * H>::value, SHX = XL - 2 * H;  // x region [c0 - XL, c0 + TW + XL)
  static constexpr int GXL = (TW + 2 * XL) / 4;                    // loaded x groups per row (24 / 20)
  static constexpr int WX = TW + 2 * XL + 4;                       // x ring pitch (odd slot count)
  // t ring: 48 rows (a step's window + new rows: 4H + 2 TS <= 48 + TS) + a mirror of its first 4H
  // (rows 48..48+4H-1 repeat rows 0..4H-1), so any (4H+1)-row window starting in the ring is contiguous
  static constexpr int XRING = 32, TRING = 48, TMIR = 4 * H;
  static constexpr int WT = TW + 4, WU = TW + 4;  // t / u rows: 65 columns used (272 B; GEN: 66)
  static constexpr int SLM1 = TW + 1;             // GEN: slot of column c0 - 1 in a t / u row
  // z tiles (own __shared__ arrays, filled by LDS-DMA, lane-linear): z0 rows of 17 groups (from
  // column c0; GEN: 18 from c0 - 4), z1 rows of 18 groups (from column c0 - 4); ZR rows from row a;
  // 5 (GEN: 6) wave-instructions of 64 x 16 B each
  static constexpr int ZR = GEN ? TS + 2 : TS + 1, Z0C = GEN ? 4 : 0, Z0G = GEN ? 18 : 17;
  static constexpr int WZ0 = 4 * Z0G, WZ1 = TW + 8, ZSLOTS = (GEN ? 6 : 5) * 64;
  static constexpr int UR = GEN ? TS + 2 : TS + 1;  // u ring rows: [a, a+16] (GEN: [a-1, a+16])
  static constexpr int NVH = (SHX + 3 + 4 * H) / 4 + 1;  // b128 groups a PH item reads
  static constexpr int NXN = TS * GXL;                   // x items per step
  static constexpr int NXP = (4 * H + 1 + (GEN ? 1 : 0)) * GXL;  // prologue x items
  static constexpr int O_XR = 0, O_T = O_XR + XRING * WX, O_U = O_T + (TRING + TMIR) * WT, O_W = O_U + UR * WU,
                       NW = 64 + 32 * H, SZ = O_W + NW;  // W: the ntaps table
  static_assert(ZR * (WZ0 / 4) <= ZSLOTS && ZR * (WZ1 / 4) <= ZSLOTS, "z tiles");
  static_assert(H == 3 || H == 7, "tiers 3 and 7");
  static_assert(TS + 2 * H + 1 + TS <= XRING + 1 + 2 * H, "x ring holds rows [a+1, a+2H+17)");
  static_assert(4 * H + TS <= TRING, "t ring holds a step's PV window (the rows PH writes are its newest)");
  static __device__ __forceinline__ int tslot(int r) { return (int)((unsigned)(r + TRING * (1 << 20)) % TRING); }
  static_assert(4 * (NVH - 1) + 3 >= SHX + 4 + 4 * H, "PH window (5 outputs)");
  static_assert((WX / 4) % 2 == 1, "odd x slot pitch");
};

template <typename T, int H, int HK, int NT, int KK>
__device__ __forceinline__ void nmarch_task(const T* __restrict__ x, T* __restrict__ xn, const T* __restrict__ z,
                                            T* __restrict__ zn, const T* __restrict__ b,
                                            const T* __restrict__ tq, const Slab32& s, const Params<T>& P, int gk,
                                            int edge, int s0, int s1, int c0, T* sm, T* Z0, T* Z1,
                                            double (&part)[4], int stop_raw) {
  static_assert(sizeof(T) == 4 && NT == 256, "fp32, 256 threads (4 rows x 16 column groups per wave)");
  constexpr bool GEN = KK != PCS_FORWARD;
  using M = NMarch<H, GEN>;
  constexpr int TS = M::TS, TW = M::TW, NQ = M::NQ, XL = M::XL, SHX = M::SHX, NVH = M::NVH;
  constexpr int WX = M::WX, WT = M::WT, WU = M::WU, WZ0 = M::WZ0, WZ1 = M::WZ1, GXL = M::GXL;
  constexpr int UR = M::UR, ZR = M::ZR, SLM1 = M::SLM1;
  constexpr int KXN = cdiv(M::NXN, NT), KXP = cdiv(M::NXP, NT);
  constexpr int GG = TW / 4;
  T* XR = sm + M::O_XR;
  T* TR = sm + M::O_T;
  T* U = sm + M::O_U;
  T* W = sm + M::O_W;  // taps (broadcast reads, re-read per phase: none live across the loop)
  int wz = 0;          // 0, laundered every step: taps read at W + wz are not loop-invariant
  const T* Wq = W;     // (so no tap read is hoisted out of the loop into registers)
  for (int i = threadIdx.x; i < M::NW; i += NT) W[i] = tq[i];  // visible after the first barrier
  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hb = tid >> 5, l5 = tid & 31;
  const int ui = 2 * hb + lane_grp(l5), ug = lane_idx(l5);  // every phase: row ui, column group ug
  const int n0 = s.n0, n1 = s.n1;
  const int zstride = (s.rows + 2 * s.hz) * n1;
  const int xc0 = c0 - XL;
  const View vx = make_view(x, s, s.hx), vb = make_view(b, s, s.hy), vz0 = make_view(z, s, s.hz),
             vz1 = make_view(z + zstride, s, s.hz);
  const uint32_t pitch = (uint32_t)n1 * 4u;
  const Rsrc rxn = rsrc_of(xn, (uint32_t)(s.rows + 2 * s.hx) * pitch);
  const Rsrc rzn0 = rsrc_of(zn, (uint32_t)zstride * 4u), rzn1 = rsrc_of(zn + zstride, (uint32_t)zstride * 4u);
#define PCS_WAVE_ON(k, N) ((k) * NT + wv * 64 < (N))
#define PCS_ITEM(k, N) min((k) * NT + tid, (N) - 1)

  // ---- per-thread geometry
  const int ucg = c0 + 4 * ug;
  const uint32_t co_u = col_off(ucg, n1);
  const bool cin = ucg < n1;                        // group in the image (4-groups wholly in / out)
  const bool clast = ucg == n1 - 4;                 // holds the image's last column
  const bool cown = cin;                            // stored by this workgroup
  // GEN: the strip's columns c0 - 1 .. c0 + 64 >= 2 samples inside the image (no column edge rules)
  const bool cint = c0 >= 4 && c0 + TW + 3 <= n1 - 3;
  // GEN extra columns: lane l of wave wv works on output (row 4 wv + (eo & 3), column c0 - 1 (eo < 4) or
  // c0 + 64), eo = l / 8, window taps l % 8 + 8 j; its b value is loaded with the step's b (bm1)
  const int elane = tid & 63, eo = elane >> 3, esub = elane & 7, eur = 4 * wv + (eo & 3);
  const bool eright = eo >= 4;
  const int ecol = eright ? c0 + TW : c0 - 1, ets = eright ? TW : SLM1, eti = eright ? TW + 4 : 3;
  const uint32_t co_bx = GEN ? col_off(ecol, n1) : kOOB;
  // forward: lane l of wave wv works on the 65th column of row 4 wv + l / 16, window taps l % 16 + 16 j
  const int fur = 4 * wv + (elane >> 4), fsub = elane & 15;
  uint32_t co_xn[KXN];
  int rr_xn[KXN];
#pragma unroll
  for (int k = 0; k < KXN; ++k) {
    const int e = PCS_ITEM(k, M::NXN);
    rr_xn[k] = e / GXL;
    co_xn[k] = col_off(xc0 + 4 * (e - (e / GXL) * GXL), n1);
  }

  auto load_xn = [&](G4<T>(&xv)[KXN], int r0) {  // x rows [r0, r0 + TS) of the x region
#pragma unroll
    for (int k = 0; k < KXN; ++k) xv[k] = bload4a<PCS_NM_LAUX>(vx.r, vx.row_off(r0 + rr_xn[k]) + co_xn[k]);
  };
  auto store_xn = [&](const G4<T>(&xv)[KXN], int r0) {
#pragma unroll
    for (int k = 0; k < KXN; ++k) {
      if (!PCS_WAVE_ON(k, M::NXN)) continue;
      const int e = PCS_ITEM(k, M::NXN);
      const int r = e / GXL, g = e - (e / GXL) * GXL;
      st4(XR + ((r0 + r) & 31) * WX + 4 * g, xv[k]);
    }
  };
  // z0 rows [a, a + ZR), cols [c0 - Z0C, c0 + TW + 4) -> Z0; z1 rows [a, a + ZR), cols [c0 - 4, c0 + TW + 4) -> Z1,
  // straight into LDS (buffer_load ... lds: no VGPRs, no ds_write).  Wave w issues tile
  // instructions w and w + 4 of each tile (5 / 6 each): lane l of instruction j fills slot 64 j + l (rows
  // past the tile and rows below `rmin` read as 0).  The issuing waves wait for them (vmcnt) before the
  // barrier that precedes the first read.
  const int lane = tid & 63;
  auto load_z = [&](int a, int rmin) {
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = wv + 4 * jj;
      if (j < M::ZSLOTS / 64) {
        const int e = 64 * j + lane;
        constexpr int G0 = M::Z0G;
        const int r0 = e / G0, g0 = e - G0 * (e / G0);  // z0: 17 (GEN: 18) groups per row
        const int r1 = e / 18, g1 = e - 18 * (e / 18);  // z1: 18 groups per row (cols c0 - 4 .. c0 + 67)
        const uint32_t o0 = (r0 >= ZR || r0 < rmin ? kOOB : vz0.row_off(a + r0)) + col_off(c0 - M::Z0C + 4 * g0, n1);
        const uint32_t o1 = (r1 >= ZR || r1 < rmin ? kOOB : vz1.row_off(a + r1)) + col_off(c0 - 4 + 4 * g1, n1);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(vz0.r, (__attribute__((address_space(3))) void*)(Z0 + 256 * j), 16,
                                                 o0, 0, 0, PCS_NM_LAUX);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(vz1.r, (__attribute__((address_space(3))) void*)(Z1 + 256 * j), 16,
                                                 o1, 0, 0, PCS_NM_LAUX);
      }
    }
  };
  // ---- PH: t row lr = N_h x row lr on columns [c0 + 4 ug, + 5) -> t ring (the fifth column is
  // kept by the last group only: the strip's 65th column)
  auto ph = [&](int lr) {
    const T* xrow = XR + (lr & 31) * WX;
    T v[4 * NVH];
#pragma unroll
    for (int q = 0; q < NVH; ++q) {
      const G4<T> t4 = lds4(xrow + 4 * ug + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * q + e] = t4.v[e];
    }
    G4<T> o;
    T o4 = T(0), om1 = T(0);  // om1 (GEN): column c0 - 1 (kept by group 0)
#pragma unroll
    for (int m = 0; m < 4; ++m) o.v[m] = T(0);
    // taps 4 at a time (broadcast LDS reads), the next 4 read while the current ones are used
    constexpr int NQ4 = (NQ + 3) / 4;
    G4<T> wc = lds4(Wq + 32), wn;
#pragma unroll
    for (int q4 = 0; q4 < NQ4; ++q4) {
      if (q4 + 1 < NQ4) wn = lds4(Wq + 32 + 4 * (q4 + 1));
      pcs_fence();
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int q = 4 * q4 + e;
        if (q < NQ) {
#pragma unroll
          for (int m = 0; m < 4; ++m) o.v[m] += wc.v[e] * v[SHX + m + q];
          o4 += wc.v[e] * v[SHX + 4 + q];
          if constexpr (GEN) om1 += wc.v[e] * v[SHX - 1 + q];
        }
      }
      pin4(o);
      pin1(o4);
      if constexpr (GEN) pin1(om1);
      pcs_fence();
      wc = wn;
    }
    if (c0 < H) {  // exact rows of N_h on the H columns nearest the left image edge
      const G4<T> x0 = lds4(xrow + XL), x1 = lds4(xrow + XL + 4);  // image columns 0..7
      const T xe[8] = {x0.v[0], x0.v[1], x0.v[2], x0.v[3], x1.v[0], x1.v[1], x1.v[2], x1.v[3]};
      const bool on = ug < 2;
      const T* et = Wq + 64 + 16 * H + 4 * (on ? ug : 0);
#pragma unroll
      for (int k = 0; k < H; ++k) {
        const G4<T> e4 = lds4(et + 8 * k);
#pragma unroll
        for (int m = 0; m < 4; ++m) o.v[m] -= (on ? e4.v[m] : T(0)) * xe[k];
      }
    }
    if (c0 + TW + 1 > n1 - H) {  // ... and the right one (image columns n1 - 8 .. n1 - 1)
      const T* xr8 = xrow + (n1 - 8 - xc0);
      const G4<T> x0 = lds4(xr8), x1 = lds4(xr8 + 4);
      const T xf[8] = {x0.v[0], x0.v[1], x0.v[2], x0.v[3], x1.v[0], x1.v[1], x1.v[2], x1.v[3]};
      const int j = ucg - (n1 - 8);
      const bool on = j == 0 || j == 4;
      const bool on5 = ug == GG - 1 && ucg + 4 == n1 - 4;  // the 65th column is column n1 - 4
      const T* et = Wq + 64 + 24 * H + (on ? j : 0);
#pragma unroll
      for (int k = 0; k < H; ++k) {
        const G4<T> e4 = lds4(et + 8 * k);
#pragma unroll
        for (int m = 0; m < 4; ++m) o.v[m] -= (on ? e4.v[m] : T(0)) * xf[8 - H + k];
        o4 -= (on5 ? et[8 * k + 4 - j] : T(0)) * xf[8 - H + k];
      }
    }
    const int sl = M::tslot(lr);
    T* trow = TR + sl * WT + 4 * ug;
    st4(trow, o);
    if (ug == GG - 1) trow[4] = o4;
    if constexpr (GEN) {  // column c0 - 1 (>= H columns inside the image, or outside it: no edge rows of N_h)
      if (ug == 0) trow[SLM1] = om1;
    }
    if (sl < M::TMIR) {  // the mirror copy
      st4(trow + M::TRING * WT, o);
      if (ug == GG - 1) trow[M::TRING * WT + 4] = o4;
      if constexpr (GEN) {
        if (ug == 0) trow[M::TRING * WT + SLM1] = om1;
      }
    }
  };
  // ---- PV + update: row lr = a + 1 + ui, columns [c, c + 4), in the row layout of PH; then the strip's 65th
  // column.  (A column layout of PV / update / P6 -- a thread owning one column of the wave's four rows -- lost:
  // 123.8-125.0 against 107.1-111.0 us, profiles/r3_ck35_cols_ab.txt)
  auto pv = [&](int a, const G4<T>& bv, T b5, T bm1, int ub) {
    const int lr = a + 1 + ui, gr = s.row0 + lr;
    // GEN: the step's update rows [a+1, a+16] and z' rows [a, a+16) >= 2 samples inside the image
    const bool rint = s.row0 + a >= 2 && s.row0 + a + TS <= n0 - 3;
    int slot = ui + 1 + ub;
    slot = slot >= UR ? slot - UR : slot;
    // g = N_v t - b: rows lr - 2H .. lr + 2H of the t ring, window row q at p0 + q rows (no
    // address arithmetic: immediate offsets); reads are issued in chunks of PF behind a compiler
    // fence (at most 2 PF in flight)
    G4<T> g;
#pragma unroll
    for (int m = 0; m < 4; ++m) g.v[m] = T(0);
    const T* p0 = TR + M::tslot(lr - 2 * H) * WT + 4 * ug;  // the window is contiguous (mirror rows)
    constexpr int PF = PCS_NM_PF, NCH = (NQ + PF - 1) / PF;  // window rows per chunk
    G4<T> buf[2][PF];
#pragma unroll
    for (int j = 0; j < PF; ++j)
      if (j < NQ) buf[0][j] = lds4(p0 + j * WT);
    // taps 4 at a time, the next 4 read one chunk ahead of their use (as the window rows)
    static_assert(4 % PF == 0, "a tap group spans whole chunks");
    G4<T> w4 = lds4(Wq), w4n;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c + 1 < NCH) {
#pragma unroll
        for (int j = 0; j < PF; ++j)
          if ((c + 1) * PF + j < NQ) buf[(c + 1) & 1][j] = lds4(p0 + ((c + 1) * PF + j) * WT);
        if (((c + 1) * PF) % 4 == 0) w4n = lds4(Wq + (c + 1) * PF);
      }
      pcs_fence();
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        if (c * PF + j < NQ) {
#pragma unroll
          for (int m = 0; m < 4; ++m) g.v[m] += w4.v[(c * PF + j) & 3] * buf[c & 1][j].v[m];
        }
      }
      pin4(g);  // the chunk's FMAs stay here (not sunk below the later reads)
      pcs_fence();
      if (c + 1 < NCH && ((c + 1) * PF) % 4 == 0) w4 = w4n;
    }
    const int wrow0 = s.row0 + a + 1 + 4 * wv;  // the wave's first global row
    const bool vedge = wrow0 < H || wrow0 + 3 >= n0 - H;  // rows of N_v near an image edge
    const bool top = gr >= 0 && gr < H, bot = gr >= n0 - H && gr < n0;
    const T* d = Wq + 64 + (top ? 8 * gr : 8 * H + 8 * (gr - (n0 - H)));
    const int kr0 = (wrow0 < H ? 0 : n0 - H) - s.row0;  // local row of the band's first image row
    if (vedge) {
#pragma unroll
      for (int k = 0; k < H; ++k) {
        const G4<T> t4 = lds4(TR + (M::tslot(kr0) + k) * WT + 4 * ug);  // contiguous through the mirror
        const T w = (top || bot) ? d[k] : T(0);
#pragma unroll
        for (int m = 0; m < 4; ++m) g.v[m] -= w * t4.v[m];
      }
    }
    if constexpr (!GEN) {
      const G4<T> xv4 = lds4(XR + (lr & 31) * WX + XL + 4 * ug);
      const G4<T> za = lds4(Z0 + ui * WZ0 + 4 * ug);               // z0[lr - 1]
      const G4<T> zb = lds4(Z0 + (ui + 1) * WZ0 + 4 * ug);         // z0[lr]
      const G4<T> z1a = lds4(Z1 + (ui + 1) * WZ1 + 4 * ug);        // z1[lr][c - 4 .. c - 1]
      const G4<T> z1b = lds4(Z1 + (ui + 1) * WZ1 + 4 * ug + 4);    // z1[lr][c .. c + 3]
      const bool r_last = gr >= n0 - 1, r_first = gr <= 0;
      const bool rrow = gr < n0 && lr <= s.rows;
      const bool own = lr >= s0 && lr < s1 && gr < n0 && cown;
      // x_t = prox_G((x - tau g) - tau K^T z); K^T z for forward differences, VStack order:
      // (0 + D0^T z0) + D1^T z1
      auto xt_of = [&](T gd, T xv, T za_, T zb_, T zl, T zr, bool last_col) {
        T d0 = r_first ? T(0) : za_;
        if (!r_last) d0 -= zb_;
        const T d1 = zl - (last_col ? T(0) : zr);
        return primal_prox(grad_step(xv, gd, P), d0 * P.inv_step0 + d1 * P.inv_step1, gk, P);
      };
      G4<T> uo, xo;
      T sdx = T(0), sx = T(0);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const T xv = xv4.v[m];
        const T xt = xt_of(g.v[m] - bv.v[m], xv, za.v[m], zb.v[m], (m == 0) ? z1a.v[3] : z1b.v[m - 1], z1b.v[m],
                           m == 3 && clast);
        uo.v[m] = (rrow && cin) ? reflect(xt, xv) : T(0);
        const T xnew = relax<false>(xt, xv, P);
        xo.v[m] = xnew;
        const T dx = xv - xnew;
        sdx += dx * dx;
        sx += xv * xv;
      }
      if (own) {
        part[0] += (double)sdx;
        part[1] += (double)sx;
      }
      T* urow = U + slot * WU + 4 * ug;
      st4(urow, uo);
      bstore4<PCS_NM_SAUX>(rxn, (own ? (uint32_t)(lr + s.hx) * pitch : kOOB) + co_u, xo);
      // the strip's 65th column c0 + 64 (never the image's last: n1 % 4 == 0), cooperatively: the wave's 4
      // outputs (its rows 4 wv + f, f = lane / 16) take 16 lanes each, lane fsub summing window taps
      // fsub and fsub + 16 (and edge term fsub), a row_ror DPP reduction inside the 16-lane row, then
      // every lane evaluates the update and lane fsub == 0 stores u (b65: the step's b at the column,
      // loaded per lane with bv).  The last group's 4 lanes per wave in a serial 29-read branch lost to it.
      {
        const int flr = a + 1 + fur, fgr = s.row0 + flr;
        const T* q0 = TR + M::tslot(flr - 2 * H) * WT + TW;  // the window is contiguous (mirror rows)
        T pg = T(0);
#pragma unroll
        for (int j = 0; j < (NQ + 15) / 16; ++j) {
          const int q = fsub + 16 * j;
          if (q < NQ) pg += Wq[q] * q0[q * WT];
        }
        if (vedge) {  // the exact rows of N_v near an image edge: term k = fsub
          const bool ftop = fgr >= 0 && fgr < H, fbot = fgr >= n0 - H && fgr < n0;
          const T* fd = Wq + 64 + (ftop ? 8 * fgr : 8 * H + 8 * (fgr - (n0 - H)));
          if (fsub < H && (ftop || fbot)) pg -= fd[fsub] * TR[(M::tslot(kr0) + fsub) * WT + TW];
        }
        pg = row_sum16(pg);
        const T xe = XR[(flr & 31) * WX + XL + TW];
        const bool f_last = fgr >= n0 - 1, f_first = fgr <= 0;
        T d0 = f_first ? T(0) : Z0[fur * WZ0 + TW];
        if (!f_last) d0 -= Z0[(fur + 1) * WZ0 + TW];
        const T d1 = Z1[(fur + 1) * WZ1 + TW + 3] - Z1[(fur + 1) * WZ1 + TW + 4];
        const T xt = primal_prox(grad_step(xe, pg - b5, P), d0 * P.inv_step0 + d1 * P.inv_step1, gk, P);
        int fslot = fur + 1 + ub;
        fslot = fslot >= UR ? fslot - UR : fslot;
        const bool frow = fgr < n0 && flr <= s.rows;
        if (fsub == 0) U[fslot * WU + TW] = (frow && c0 + TW < n1) ? reflect(xt, xe) : T(0);
      }
    } else {  // backward / centred K: K^T z from z rows lr - 1 .. lr + 1, columns c - 1 .. c + 1
      const G4<T> xv4 = lds4(XR + (lr & 31) * WX + XL + 4 * ug);
      const T* z0p = Z0 + ui * WZ0 + 4 * ug + 4;  // tile row ui = row lr - 1, column c
      const G4<T> za = lds4(z0p), zb = lds4(z0p + WZ0), zc = lds4(z0p + 2 * WZ0);
      const T* z1p = Z1 + (ui + 1) * WZ1 + 4 * ug;  // row lr, columns c - 4 ..
      const G4<T> z1a = lds4(z1p), z1b = lds4(z1p + 4);
      const T z1r = lds4(z1p + 8).v[0];
      const T zh[6] = {z1a.v[3], z1b.v[0], z1b.v[1], z1b.v[2], z1b.v[3], z1r};
      const bool rrow = (unsigned)gr < (unsigned)n0 && lr <= s.rows;
      const bool own = lr >= s0 && lr < s1 && gr < n0 && cown;
      // x_t = prox_G((x - tau (g - b)) - tau K^T z), K^T z = D0^T z0 + D1^T z1 (stencil.hpp windows;
      // I: rows and columns >= 2 samples inside the image, no edge rules -- the same bits)
      // (intr: the row axis interior; intc: the column axis)
      auto xt_of = [&](auto intr, auto intc, T gd, T xv, const T (&w0)[5], const T (&w1)[5], int i1) {
        constexpr bool I0 = decltype(intr)::value;
        constexpr bool I1 = decltype(intc)::value;
        const T kt = pcs_fma(sw_d1_adj<KK, I0>(w0, gr, n0, edge), P.inv_step0,
                             sw_d1_adj<KK, I1>(w1, i1, n1, edge) * P.inv_step1);
        return primal_prox(grad_step(xv, gd, P), kt, gk, P);
      };
      G4<T> uo, xo;
      T sdx = T(0), sx = T(0);
      auto items = [&](auto intr, auto intc) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const T xv = xv4.v[m];
          const T w0[5] = {T(0), za.v[m], zb.v[m], zc.v[m], T(0)};
          const T w1[5] = {T(0), zh[m], zh[m + 1], zh[m + 2], T(0)};
          const T xt = xt_of(intr, intc, g.v[m] - bv.v[m], xv, w0, w1, ucg + m);
          uo.v[m] = (rrow && cin) ? reflect(xt, xv) : T(0);
          const T xnew = relax<true>(xt, xv, P);
          xo.v[m] = xnew;
          const T dx = xv - xnew;
          sdx += dx * dx;
          sx += xv * xv;
        }
      };
      if (rint && cint) items(std::true_type{}, std::true_type{});
      else if (rint) items(std::true_type{}, std::false_type{});
      else items(std::false_type{}, std::false_type{});
      if (own) {
        part[0] += (double)sdx;
        part[1] += (double)sx;
      }
      T* urow = U + slot * WU + 4 * ug;
      st4(urow, uo);
      bstore4<PCS_NM_SAUX>(rxn, (own ? (uint32_t)(lr + s.hx) * pitch : kOOB) + co_u, xo);
      // the two extra columns, cooperatively: the wave's 8 outputs (its 4 rows x columns c0 - 1 and
      // c0 + 64) take 8 lanes each, lane `esub` summing window taps esub, esub + 8, .. (and edge term
      // esub), a 3-step xor reduction, then all 8 lanes evaluate the update and lane 0 of the group
      // stores u.  Column c0 - 1 is >= H inside the image or outside it, c0 + 64 is < n1 - H or the
      // image's last group (no edge rows of N_h); every lane of the wave does useful work instead of
      // 8 lanes issuing a 29-read serial pass
      {
        const int elr = a + 1 + eur, egr = s.row0 + elr;
        const T* q0 = TR + M::tslot(elr - 2 * H) * WT + ets;  // the window is contiguous (mirror rows)
        T part_g = T(0);
#pragma unroll
        for (int j = 0; j < (NQ + 7) / 8; ++j) {
          const int q = esub + 8 * j;
          if (q < NQ) part_g += Wq[q] * q0[q * WT];
        }
        if (vedge) {  // the exact rows of N_v near an image edge: term k = esub
          const bool etop = egr >= 0 && egr < H, ebot = egr >= n0 - H && egr < n0;
          const T* ed = Wq + 64 + (etop ? 8 * egr : 8 * H + 8 * (egr - (n0 - H)));
          if (esub < H && (etop || ebot)) part_g -= ed[esub] * TR[(M::tslot(kr0) + esub) * WT + ets];
        }
        part_g = oct_sum8(part_g);
        const T xe = XR[(elr & 31) * WX + XL + (ecol - c0)];
        const T w0[5] = {T(0), Z0[eur * WZ0 + eti], Z0[(eur + 1) * WZ0 + eti], Z0[(eur + 2) * WZ0 + eti], T(0)};
        const T* z1e = Z1 + (eur + 1) * WZ1 + eti;
        const T w1[5] = {T(0), z1e[-1], z1e[0], z1e[1], T(0)};
        // K^T z on the extra column's row (egr) through xt_of's row index: recompute with egr
        const T kt = pcs_fma(sw_d1_adj<KK, false>(w0, egr, n0, edge), P.inv_step0,
                             sw_d1_adj<KK, false>(w1, ecol, n1, edge) * P.inv_step1);
        const T xt = primal_prox(grad_step(xe, part_g - bm1, P), kt, gk, P);
        int eslot = eur + 1 + ub;
        eslot = eslot >= UR ? eslot - UR : eslot;
        const bool erow = (unsigned)egr < (unsigned)n0 && elr <= s.rows;
        if (esub == 0) U[eslot * WU + ets] = (erow && (unsigned)ecol < (unsigned)n1) ? reflect(xt, xe) : T(0);
      }
    }
  };
  // ---- P6: z' on row lr = a + ui
  auto p6f = [&](int a, int ub) {
    const int lr = a + ui, gr = s.row0 + lr;
    int sl0 = ui + ub, sl1 = ui + 1 + ub;
    sl0 = sl0 >= 17 ? sl0 - 17 : sl0;
    sl1 = sl1 >= 17 ? sl1 - 17 : sl1;
    const G4<T> uc = lds4(U + sl0 * WU + 4 * ug);
    const G4<T> ud = lds4(U + sl1 * WU + 4 * ug);
    const G4<T> zv0 = lds4(Z0 + ui * WZ0 + 4 * ug);
    const G4<T> zv1 = lds4(Z1 + ui * WZ1 + 4 * ug + 4);
    const T une = lds4(U + sl0 * WU + 4 * ug + 4).v[0];  // u[c + 4] (a b128 read: conflict-free)
    const bool r_last = gr >= n0 - 1;
    const bool own = lr >= s0 && lr < s1 && gr < n0 && cown;
    G4<T> o0, o1;
    T sdz = T(0), sz = T(0);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const T uright = (m < 3) ? uc.v[m + 1] : une;
      const T d0 = r_last ? T(0) : (ud.v[m] - uc.v[m]);
      const T d1 = (m == 3 && clast) ? T(0) : (uright - uc.v[m]);
      const T zv[2] = {zv0.v[m], zv1.v[m]};
      const T w[2] = {dual_arg(zv[0], d0 * P.inv_step0, P), dual_arg(zv[1], d1 * P.inv_step1, P)};
      T zt[2];
      fenchel_w<2, Fenchel::Direct, false>(HK, w, P, zt);
      o0.v[m] = relax<false>(zt[0], zv[0], P);
      o1.v[m] = relax<false>(zt[1], zv[1], P);
      const T e0 = zv0.v[m] - o0.v[m], e1 = zv1.v[m] - o1.v[m];
      sdz += e0 * e0 + e1 * e1;
      sz += zv0.v[m] * zv0.v[m] + zv1.v[m] * zv1.v[m];
    }
    if (own) {
      part[2] += (double)sdz;
      part[3] += (double)sz;
    }
    const uint32_t off = (own ? (uint32_t)(lr + s.hz) * pitch : kOOB) + co_u;
    bstore4<PCS_NM_SAUX>(rzn0, off, o0);
    bstore4<PCS_NM_SAUX>(rzn1, off, o1);
  };
  // ---- P6 (GEN): z' on row lr = a + ui; K u from u rows lr - 1 .. lr + 1 (ring rows [a - 1, a + 16]) and
  // columns c - 1 .. c + 4 (c0 - 1 at SLM1, c0 + 64 at slot TW)
  auto p6g = [&](int a, int ub) {
    const int lr = a + ui, gr = s.row0 + lr;
    int slm = ui - 1 + ub, sl0 = ui + ub, sl1 = ui + 1 + ub;
    slm = slm < 0 ? slm + UR : (slm >= UR ? slm - UR : slm);
    sl0 = sl0 >= UR ? sl0 - UR : sl0;
    sl1 = sl1 >= UR ? sl1 - UR : sl1;
    const T* u0 = U + sl0 * WU;
    const G4<T> uc = lds4(u0 + 4 * ug), ud = lds4(U + sl1 * WU + 4 * ug), uu = lds4(U + slm * WU + 4 * ug);
    const T ur4 = lds4(u0 + 4 * ug + 4).v[0];               // u[c + 4] (a b128 read: conflict-free)
    const T ul = lds1(u0 + (ug == 0 ? SLM1 : 4 * ug - 1));  // u[c - 1]
    const T uh[6] = {ul, uc.v[0], uc.v[1], uc.v[2], uc.v[3], ur4};
    const G4<T> zv0 = lds4(Z0 + ui * WZ0 + 4 * ug + 4);
    const G4<T> zv1 = lds4(Z1 + ui * WZ1 + 4 * ug + 4);
    const bool own = lr >= s0 && lr < s1 && gr < n0 && cown;
    const bool rint = s.row0 + a >= 2 && s.row0 + a + TS <= n0 - 3;
    G4<T> o0, o1;
    T sdz = T(0), sz = T(0);
    auto items = [&](auto intr, auto intc) {
      constexpr bool I0 = decltype(intr)::value;
      constexpr bool I1 = decltype(intc)::value;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const T w0[5] = {T(0), uu.v[m], uc.v[m], ud.v[m], T(0)};
        const T w1[5] = {T(0), uh[m], uh[m + 1], uh[m + 2], T(0)};
        const T k0 = sw_d1_fwd<KK, I0>(w0, gr, n0, P.inv_step0, edge);
        const T k1 = sw_d1_fwd<KK, I1>(w1, ucg + m, n1, P.inv_step1, edge);
        const T zv[2] = {zv0.v[m], zv1.v[m]};
        const T w[2] = {dual_arg(zv[0], k0, P), dual_arg(zv[1], k1, P)};
        T zt[2];
        fenchel_w<2, Fenchel::Direct, true>(HK, w, P, zt);
        o0.v[m] = relax<true>(zt[0], zv[0], P);
        o1.v[m] = relax<true>(zt[1], zv[1], P);
        const T e0 = zv0.v[m] - o0.v[m], e1 = zv1.v[m] - o1.v[m];
        sdz += pcs_fma(e0, e0, e1 * e1);
        sz += pcs_fma(zv0.v[m], zv0.v[m], zv1.v[m] * zv1.v[m]);
      }
    };
    if (rint && cint) items(std::true_type{}, std::true_type{});
    else if (rint) items(std::true_type{}, std::false_type{});
    else items(std::false_type{}, std::false_type{});
    if (own) {
      part[2] += (double)sdz;
      part[3] += (double)sz;
    }
    const uint32_t off = (own ? (uint32_t)(lr + s.hz) * pitch : kOOB) + co_u;
    bstore4<PCS_NM_SAUX>(rzn0, off, o0);
    bstore4<PCS_NM_SAUX>(rzn1, off, o1);
  };
  auto p6 = [&](int a, int ub) {
    if constexpr (GEN) p6g(a, ub);
    else p6f(a, ub);
  };

  // ================= prologue: t rows [s0 - 2H, s0 + 2H], u / x' on row s0 (GEN: t rows from s0 - 2H - 1,
  // u on rows s0 - 1 and s0)
  // b of a group = its 4 columns (bv) and, for the last group, the strip's 65th column (b5; GEN: the
  // lane's extra-column output, bm1)
  const uint32_t co_b5 = ug == GG - 1 ? col_off(c0 + TW, n1) : kOOB;
  // forward: every lane loads b of its 65th-column output (row r0 + fur); GEN: the last group's lanes b of
  // their own row's 65th column
  const uint32_t co_f65 = col_off(c0 + TW, n1);
  auto load_b5 = [&](int r0) -> T {
    if constexpr (!GEN)
      return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vb.r, (int)(vb.row_off(r0 + fur) + co_f65), 0, 0));
    else
      return bload4(vb.r, vb.row_off(r0 + ui) + co_b5).v[0];
  };
  constexpr int PR = GEN ? 1 : 0;  // extra prologue rows
  G4<T> xnx[KXN], bv;
  T b5, bm1 = T(0);
  {
    G4<T> xv[KXP];
#pragma unroll
    for (int k = 0; k < KXP; ++k) {
      const int e = PCS_ITEM(k, M::NXP);
      const int r = e / GXL, g = e - (e / GXL) * GXL;
      xv[k] = bload4(vx.r, vx.row_off(s0 - 2 * H - PR + r) + col_off(xc0 + 4 * g, n1));
    }
    // z rows s0 - 1, s0 only (GEN: s0 - 3 .. s0 + 1) for the prologue's update rows; b on those rows
    load_z(s0 - TS, GEN ? TS - 3 : TS - 1);
    if constexpr (GEN) {  // rows s0 - 1 (ui 14) and s0 (ui 15)
      const uint32_t rbp = ui >= TS - 2 ? vb.row_off(s0 - TS + 1 + ui) : kOOB;
      bv = bload4(vb.r, rbp + co_u);
      b5 = bload4(vb.r, rbp + co_b5).v[0];
      bm1 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vb.r, (int)(vb.row_off(s0 - TS + 1 + eur) + co_bx), 0, 0));
    } else {
      bv = bload4(vb.r, (ui == TS - 1 ? vb.row_off(s0) : kOOB) + co_u);
      b5 = load_b5(s0 - TS + 1);  // row s0: wave 3's last output row
    }
#pragma unroll
    for (int k = 0; k < KXP; ++k) {
      if (!PCS_WAVE_ON(k, M::NXP)) continue;
      const int e = PCS_ITEM(k, M::NXP);
      const int r = e / GXL, g = e - (e / GXL) * GXL;
      st4(XR + ((s0 - 2 * H - PR + r) & 31) * WX + 4 * g, xv[k]);
    }
    // step 0's x rows: in flight with the prologue's (parked after PH) -- one exposed load latency per segment, not
    // two: C3 106.7-106.9 against 107.0-107.8 us loaded after the prologue's PV (profiles/r3_ck43_xe_*ab.txt)
    load_xn(xnx, s0 + 2 * H + 1);
    vm_wait<0>();
  }
  if (stop_raw) return;  // loop already stopped (solver.py:65-66): loads landed, nothing stored
  lds_barrier();
  ph(s0 - 2 * H - PR + ui);  // t rows [s0 - 2H - PR, s0 - 2H - PR + 16)
  if (ui + TS < 4 * H + 1 + PR) ph(s0 - 2 * H - PR + TS + ui);  // t rows [.. + 16, s0 + 2H]
  lds_barrier();
  // u on row s0 (GEN: s0 - 1 too) -> the ring slots of step 0's rows a - 1, a; x' on row s0 (rows above: not own)
  if (wv == 3) pv(s0 - TS, bv, b5, bm1, UR - TS);
  lds_barrier();
  store_xn(xnx, s0 + 2 * H + 1);  // slots of rows [s0 + 2H - 31, s0 + 2H - 15): read by PH above only

  // ================= march: step k covers t rows [a+2H+1, a+2H+17), u / x' rows [a+1, a+17), z' rows [a, a+16)
  const int nsteps = (s1 - s0 + TS - 1) / TS;
  int ub = 0;  // (16 k) mod UR: row r = a + j sits in u ring slot (j + ub) mod UR
  for (int k = 0; k < nsteps; ++k) {
    const int a = s0 + k * TS;
    lds_barrier();  // step k-1 done with U, Z and the t / x ring rows it read; its x rows landed
    asm volatile("" : "+v"(wz));
    Wq = W + wz;
    // this step's z tiles (LDS-DMA) and b, the next step's x rows (registers, landed after P6); they issue at
    // wave priority 3, ahead of other waves' VALU (0 again for the LDS / VALU phases): 113.1-113.6 against
    // 115.9-116.5 us without (4 alternating reps)
    __builtin_amdgcn_s_setprio(3);
    // The z tiles land through LDS-DMA loads; before the barrier that precedes their first read the wave
    // waits until only the loads it issued after them are outstanding.  Forward K: b (bv, b5) and the x
    // rows, counted.  GEN: its b values (bm1 of the extra-column lanes, b5 of the last group) are used on
    // subsets of lanes only, and the compiler sinks those loads to their uses past the wait -- counted,
    // they left the last tile load in flight when the tiles were read (a race: the C3 centred iterate
    // differed between runs from the second iteration on).  GEN therefore issues every load ahead of the
    // tiles and waits for all of them (tools/vmcnt_check.py checks the counts in the assembly).
    if constexpr (GEN) {
      bm1 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vb.r, (int)(vb.row_off(a + 1 + eur) + co_bx), 0, 0));
      bv = bload4a<PCS_NM_LAUX>(vb.r, vb.row_off(a + 1 + ui) + co_u);
      b5 = load_b5(a + 1);
      load_xn(xnx, a + 2 * H + 1 + TS);
      load_z(a, 0);
    } else {
      load_z(a, 0);
      const uint32_t rb = vb.row_off(a + 1 + ui);
      bv = bload4a<PCS_NM_LAUX>(vb.r, rb + co_u);
      b5 = load_b5(a + 1);
      load_xn(xnx, a + 2 * H + 1 + TS);
    }
    __builtin_amdgcn_s_setprio(0);
    ph(a + 2 * H + 1 + ui);
    if constexpr (GEN) vm_wait<0>();
    else vm_wait<KXN + 2>();  // this wave's z tile loads have landed (b and the x rows may be in flight)
    lds_barrier();
    pv(a, bv, b5, bm1, ub);
    lds_barrier();
    p6(a, ub);
    store_xn(xnx, a + 2 * H + 1 + TS);  // x ring slots of rows [a + 2H - 15, a + 2H + 1): read above
    if constexpr (GEN) ub = ub + TS >= UR ? ub + TS - UR : ub + TS;
    else ub = ub == 0 ? 16 : ub - 1;
  }
#undef PCS_WAVE_ON
#undef PCS_ITEM
}

// One block per task (64-column strip x row segment); with `hist` the last workgroups also
// reduce the partials and run the loop control, with `ro.sums` they only reduce.  The C3 kernel
// (forward K):
template <typename T, int H, int HK, int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(PCS_NM_WPE))) void k_pds2d_nmarch(
    const T* __restrict__ x, T* __restrict__ xn, const T* __restrict__ z, T* __restrict__ zn,
    const T* __restrict__ b, const T* __restrict__ tq, Slab32 s, Params<T> P, int gk, double* __restrict__ partials,
    Ctrl* ctrl, double* hist, void* ws, RedOut ro, int tiles_x, Bands bd, int ntasks) {
  using M = NMarch<H, false>;
  __shared__ __attribute__((aligned(16))) T sm[M::SZ];
  __shared__ __attribute__((aligned(16))) T zs0[4 * M::ZSLOTS];  // z tiles: own arrays, so the LDS-DMA
  __shared__ __attribute__((aligned(16))) T zs1[4 * M::ZSLOTS];  // into them never aliases a ring read
  __shared__ double red[4 * (NT / 64)];
  __shared__ int flag[2];
  if (fin_slot(ro, ntasks, ctrl, hist, red, flag)) return;  // deferred finalization (pds_ctrl.hpp)
  const int stop_raw = stop_flag_early(ctrl, ro);  // consumed in the task
  const bool stopped = !stop_deferred(ro) && stop_requested(ctrl, ro, flag);
  if (stopped && ro.sums == nullptr) return;  // loop already stopped (solver.py:65-66)

  const int task = xcd_task((int)blockIdx.x - fin_shift(ro), ntasks);  // XCD-aware (common.hpp)
  const int seg = task / tiles_x, strip = task - seg * tiles_x;
  int s0, s1;
  band_rows(bd, seg, s0, s1);
  const int c0 = strip * M::TW;

  double part[4] = {0.0, 0.0, 0.0, 0.0};
  if (!stopped) {
    // the G = 0 problem (the C3 benchmark's) runs a copy of the task compiled with that constant, so that prox_g's
    // scalar branches on gk -- four per thread and step -- and the live gk / seg_a / seg_b leave its loop
    if (gk == PCS_G_NULL)  // uniform
      nmarch_task<T, H, HK, NT, PCS_FORWARD>(x, xn, z, zn, b, tq, s, P, PCS_G_NULL, 0, s0, s1, c0, sm, zs0, zs1, part,
                                             stop_raw);
    else
      nmarch_task<T, H, HK, NT, PCS_FORWARD>(x, xn, z, zn, b, tq, s, P, gk, 0, s0, s1, c0, sm, zs0, zs1, part, stop_raw);
  }
  if (stop_raw) return;  // the task returned before any store
  block_sum<4>(part, red);
  publish_partials(part, partials, ntasks, ws, ctrl, hist, flag, ro);
}

// backward / centred K (KK; `edge` = Gradient(edge=...) of the centred kind): the GEN geometry
template <typename T, int H, int HK, int NT, int KK>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(PCS_NM_WPE))) void k_pds2d_nmarch_gen(
    const T* __restrict__ x, T* __restrict__ xn, const T* __restrict__ z, T* __restrict__ zn,
    const T* __restrict__ b, const T* __restrict__ tq, Slab32 s, Params<T> P, int gk, int edge,
    double* __restrict__ partials, Ctrl* ctrl, double* hist, void* ws, RedOut ro, int tiles_x, Bands bd,
    int ntasks) {
  static_assert(KK == PCS_BACKWARD || KK == PCS_CENTERED, "k_pds2d_nmarch is the forward kernel");
  using M = NMarch<H, true>;
  __shared__ __attribute__((aligned(16))) T sm[M::SZ];
  __shared__ __attribute__((aligned(16))) T zs0[4 * M::ZSLOTS];
  __shared__ __attribute__((aligned(16))) T zs1[4 * M::ZSLOTS];
  __shared__ double red[4 * (NT / 64)];
  __shared__ int flag[2];
  if (fin_slot(ro, ntasks, ctrl, hist, red, flag)) return;  // deferred finalization (pds_ctrl.hpp)
  const int stop_raw = stop_flag_early(ctrl, ro);  // consumed in the task
  const bool stopped = !stop_deferred(ro) && stop_requested(ctrl, ro, flag);
  if (stopped && ro.sums == nullptr) return;  // loop already stopped (solver.py:65-66)

  const int task = xcd_task((int)blockIdx.x - fin_shift(ro), ntasks);  // XCD-aware (common.hpp)
  const int seg = task / tiles_x, strip = task - seg * tiles_x;
  int s0, s1;
  band_rows(bd, seg, s0, s1);
  const int c0 = strip * M::TW;

  double part[4] = {0.0, 0.0, 0.0, 0.0};
  if (!stopped) nmarch_task<T, H, HK, NT, KK>(x, xn, z, zn, b, tq, s, P, gk, edge, s0, s1, c0, sm, zs0, zs1, part, stop_raw);
  if (stop_raw) return;  // the task returned before any store
  block_sum<4>(part, red);
  publish_partials(part, partials, ntasks, ws, ctrl, hist, flag, ro);
}

}  // namespace pcs
