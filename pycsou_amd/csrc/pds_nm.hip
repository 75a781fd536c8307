// The separable-PSF row marches of the fused 2-D step (fp32, tiers 3 / 7): k_pds2d_march (four
// 15-tap passes) and the normal-operator marches k_pds2d_nmarch / k_pds2d_nmarch_gen (grad F = N x -
// Conv^T y, pds_nmarch.hpp) -- their grids and launches (planning: pds_host.hpp).
#include "pds_host.hpp"

namespace pcs {

// resident workgroups of the march kernel on the whole device (queried once)
template <int H>
static int march_slots() {
  static const int slots = [] {
    const Occupancy o = occupancy(k_pds2d_march<float, H, PCS_H_L21, kMarchNT>, kMarchNT, 0, 3);
    return o.cus * o.per_cu;
  }();
  return slots;
}

template <int H, bool GEN>
static int nmarch_slots() {
  static const int slots = [] {
    const Occupancy o = GEN ? occupancy(k_pds2d_nmarch_gen<float, H, PCS_H_L21, kNMarchNT, PCS_CENTERED>, kNMarchNT, 0, 3)
                            : occupancy(k_pds2d_nmarch<float, H, PCS_H_L21, kNMarchNT>, kNMarchNT, 0, 3);
    return env_override("PCS_NMARCH_SLOTS", o.cus * o.per_cu);
  }();
  return slots;
}

int march_slots_h(int H) { return H == 3 ? march_slots<3>() : march_slots<7>(); }
int nmarch_slots_h(int H, bool gen) {
  if (gen) return H == 3 ? nmarch_slots<3, true>() : nmarch_slots<7, true>();
  return H == 3 ? nmarch_slots<3, false>() : nmarch_slots<7, false>();
}

enum MarchKernel { kFourPass, kNormalFwd, kNormalGen };  // k_pds2d_march, k_pds2d_nmarch, k_pds2d_nmarch_gen

template <int H, int HK>
static int launch_march_k(const pcs_pds2d_args* a, MarchKernel which, const MarchPlan& p, hipStream_t st) {
  const Slab32 s = to_slab32(make_slab(a));
  const Params<float> P = make_params<float>(a);
  const unsigned grid = (unsigned)p.ntasks + fin_extra(a, p.fin_n);
  if (which == kNormalGen) {
    auto kern = a->kkind == PCS_K_GRAD_BACKWARD ? k_pds2d_nmarch_gen<float, H, HK, kNMarchNT, PCS_BACKWARD>
                                                : k_pds2d_nmarch_gen<float, H, HK, kNMarchNT, PCS_CENTERED>;
    kern<<<grid, kNMarchNT, 0, st>>>((const float*)a->x, (float*)a->xn, (const float*)a->z, (float*)a->zn,
                                     (const float*)a->cty, (const float*)a->ntaps, s, P, a->gkind, a->edge,
                                     a->partials, (Ctrl*)a->ctrl, a->hist, a->ws, red_out(a, p.fin_n), p.tiles_x, p.bd,
                                     p.ntasks);
  } else if (which == kNormalFwd) {
    k_pds2d_nmarch<float, H, HK, kNMarchNT><<<grid, kNMarchNT, 0, st>>>(
        (const float*)a->x, (float*)a->xn, (const float*)a->z, (float*)a->zn, (const float*)a->cty,
        (const float*)a->ntaps, s, P, a->gkind, a->partials, (Ctrl*)a->ctrl, a->hist, a->ws, red_out(a, p.fin_n),
        p.tiles_x, p.bd, p.ntasks);
  } else {
    k_pds2d_march<float, H, HK, kMarchNT><<<grid, kMarchNT, 0, st>>>(
        (const float*)a->x, (float*)a->xn, (const float*)a->z, (float*)a->zn, (const float*)a->y,
        (const float*)a->taps0, (const float*)a->taps1, a->half, s, P, a->gkind, a->partials, (Ctrl*)a->ctrl, a->hist,
        a->ws, red_out(a, p.fin_n), p.tiles_x, p.bd, p.ntasks);
  }
  return launch_status();
}

template <int H>
static int launch_march_k(const pcs_pds2d_args* a, MarchKernel which, const MarchPlan& p, hipStream_t st) {
  return a->hkind == PCS_H_L21 ? launch_march_k<H, PCS_H_L21>(a, which, p, st)
                               : launch_march_k<H, PCS_H_L1>(a, which, p, st);
}

// path: PCS_PATH_MARCH (forward K) or PCS_PATH_NMARCH (select_path)
int launch_march(const pcs_pds2d_args* a, int path, const MarchPlan& p, hipStream_t st) {
  if (p.ntasks == 0) return PCS_OK;
  const MarchKernel which = path == PCS_PATH_MARCH ? kFourPass : a->kkind == PCS_K_GRAD_FORWARD ? kNormalFwd : kNormalGen;
  return tier_for(a->half) == 3 ? launch_march_k<3>(a, which, p, st) : launch_march_k<7>(a, which, p, st);
}

}  // namespace pcs
