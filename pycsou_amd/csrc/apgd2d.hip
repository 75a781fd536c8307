// One launch per AcceleratedProximalGradientDescent iteration for F = (1/2)||C x - y||^2 with a separable
// blur C of half width <= 7 (pycsou/opt/proxalgs.py:586-622 inside pycsou/core/solver.py:55-76):
//
//   g = N x - C^T y  (N = C^T C: the two-pass normal-operator march of sep_nrm.hpp)
//   w = prox_G(x - tau g) ; x' = w + a (w - aux) ; aux' = w ; ||x - x'||^2, ||x||^2 ; loop control
//
// The march's PV phase hands each output chunk to the NrmApgd policy instead of storing it: 5 words of
// traffic per pixel (x, C^T y, aux in; x', aux' out).  The momentum coefficient a of every iteration comes
// from the host (it depends on the iteration index alone), so the device holds no momentum state.
#include "sep_nrm.hpp"

namespace pcs {

template <typename T>
static const void* apgd_fn() {
  if constexpr (sizeof(T) == 8) return reinterpret_cast<const void*>(&k_sep2d_nrmm<T, true, NrmApgd<T>, NrmApgd<T>>);
  else return reinterpret_cast<const void*>(&k_sep2d_nrm<T, true, NrmApgd<T>, NrmApgd<T>>);
}

// the kernel's LDS (> 48 KB) is dynamic: raise the function's limit once per type
template <typename T>
static void apgd_attr() {
  static bool done = false;
  if (!done) {
    (void)hipFuncSetAttribute(apgd_fn<T>(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)nrm_lds<T>());
    (void)hipGetLastError();
    done = true;
  }
}

// resident workgroups of the APGD march on the device (queried once per type)
template <typename T>
static int apgd_slots() {
  static const int slots = [] {
    apgd_attr<T>();
    const Occupancy o = occupancy(apgd_fn<T>(), 256, nrm_lds<T>(), 1);
    return o.cus * o.per_cu;
  }();
  return slots;
}

static bool apgd_ok(const pcs_apgd2d_args* a) {
  if (!a || (a->dtype != PCS_F32 && a->dtype != PCS_F64)) return false;
  if (a->gkind != PCS_G_NULL && a->gkind != PCS_G_NONNEG && a->gkind != PCS_G_SEGMENT && a->gkind != PCS_APGD_G_L1)
    return false;
  if (a->half < 0 || a->half > 7 || !a->taps0 || !a->taps1) return false;
  const int k = 2 * a->half + 1;
  if (!nrm_takes(a->n0, a->n1, k, a->half, k, a->half)) return false;
  const int64_t esz = a->dtype == PCS_F64 ? 8 : 4;
  if (a->n0 * a->n1 * esz >= (1LL << 30)) return false;
  const void* bufs[5] = {a->x, a->xn, a->aux, a->aux_n, a->cty};
  for (const void* p : bufs)
    if (!p || (uintptr_t)p % 16) return false;
  // a workgroup reads rows of x that its neighbours write in xn; every output array is its own
  if (a->x == a->xn || a->aux == a->aux_n || a->xn == a->aux_n || a->xn == a->aux || a->aux_n == a->x ||
      a->cty == a->xn || a->cty == a->aux_n)
    return false;
  if (a->gkind == PCS_APGD_G_L1 && !(a->tau * a->lam > 0)) return false;
  return true;
}

template <typename T>
static NrmGrid apgd_grid(const pcs_apgd2d_args* a) {
  return nrm_grid<T>(1, a->n0, a->n1, apgd_slots<T>());
}

static int64_t apgd_nblocks(const pcs_apgd2d_args* a) {
  return a->dtype == PCS_F64 ? apgd_grid<double>(a).ntasks : apgd_grid<float>(a).ntasks;
}

// one launch: (x, aux) -> (xn, aux_n), or the other way round (swap)
template <typename T>
static int apgd_launch(const pcs_apgd2d_args* a, double am, bool swap, hipStream_t st) {
  const NrmGrid g = apgd_grid<T>(a);
  if (g.ntasks > 0x7fffffff) return PCS_EUNSUPPORTED;
  apgd_attr<T>();
  NrmApgd<T> ep;
  ep.aux = (const T*)(swap ? a->aux_n : a->aux);
  ep.aux_n = (T*)(swap ? const_cast<void*>(a->aux) : a->aux_n);
  ep.tau = (T)a->tau;
  ep.a = (T)am;
  ep.thr = (T)(a->tau * a->lam);
  ep.sa = (T)a->seg_a;
  ep.sb = (T)a->seg_b;
  ep.gk = a->gkind;
  ep.d2 = ep.n2 = 0.0;
  ep.partials = a->partials;
  ep.ws = a->ws;
  ep.ctrl = reinterpret_cast<Ctrl*>(a->ctrl);
  ep.hist = a->hist;
  const T* x = (const T*)(swap ? a->xn : a->x);
  T* xn = (T*)(swap ? const_cast<void*>(a->x) : a->xn);
  const int k = 2 * a->half + 1;
  auto go = [&](auto kern) {
    kern<<<(unsigned)g.ntasks, 256, nrm_lds<T>(), st>>>(x, xn, (int)a->n0, (int)a->n1, (int)g.nstrips, (int)g.nseg,
                                                       (int)g.seg_len, g.ntasks, (const T*)a->taps0, k, a->half,
                                                       (const T*)a->taps1, k, a->half, (const T*)a->cty, ep);
  };
  if constexpr (sizeof(T) == 8) go(k_sep2d_nrmm<T, true, NrmApgd<T>, NrmApgd<T>>);
  else go(k_sep2d_nrm<T, true, NrmApgd<T>, NrmApgd<T>>);
  return launch_status();
}

}  // namespace pcs

using namespace pcs;

extern "C" {

int pcs_apgd2d_supported(const pcs_apgd2d_args* a) { return apgd_ok(a) ? 1 : 0; }

int64_t pcs_apgd2d_nblocks(const pcs_apgd2d_args* a) { return apgd_ok(a) ? apgd_nblocks(a) : -1; }

int64_t pcs_apgd2d_ws_bytes(const pcs_apgd2d_args* a) { return apgd_ok(a) ? red_ws_bytes(apgd_nblocks(a)) : -1; }

int pcs_apgd2d_step(const pcs_apgd2d_args* a, double am, hipStream_t st) {
  if (!a) return PCS_EINVAL;
  if (!apgd_ok(a)) return PCS_EUNSUPPORTED;
  if (!a->partials || !a->ctrl || !a->hist || !a->ws) return PCS_EINVAL;
  return a->dtype == PCS_F64 ? apgd_launch<double>(a, am, false, st) : apgd_launch<float>(a, am, false, st);
}

int pcs_apgd2d_run(const pcs_apgd2d_args* a, const double* a_host, int64_t n, hipStream_t st) {
  if (!a || !a_host || n < 0) return PCS_EINVAL;
  if (!apgd_ok(a)) return PCS_EUNSUPPORTED;
  if (!a->partials || !a->ctrl || !a->hist || !a->ws) return PCS_EINVAL;
  for (int64_t i = 0; i < n; ++i) {
    const bool swap = (i & 1) != 0;
    const int rc = a->dtype == PCS_F64 ? apgd_launch<double>(a, a_host[i], swap, st)
                                       : apgd_launch<float>(a, a_host[i], swap, st);
    if (rc != PCS_OK) return rc;
  }
  return PCS_OK;
}

}  // extern "C"
