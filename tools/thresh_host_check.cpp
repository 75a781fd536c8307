// Stand-alone host check of csrc/thresh.hip for a sanitizer build (CPU only; nothing is launched):
// the bracket selection pcs_thresh_pick_host against a direct evaluation of psi, and every argument check
// of pcs_thresh_l1 / pcs_thresh_ws_bytes, which return before any device call.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//         pycsou_amd/csrc/thresh.hip tools/thresh_host_check.cpp -o build/thresh_host_check
//   ./build/thresh_host_check        (only the host side is instrumented; run it on a CPU machine)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "pycsou_hip.h"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++fails;                                                \
    }                                                         \
  } while (0)

static uint64_t key64(double v) {
  uint64_t u;
  v = fabs(v);
  memcpy(&u, &v, 8);
  return u;
}
static double val64(uint64_t k) {
  double v;
  memcpy(&v, &k, 8);
  return v;
}

// one selection on data x against psi evaluated pivot by pivot
static void pick_case(const std::vector<double>& x, double a, double b, uint64_t lo, uint64_t hi, int expect_k) {
  const int J = PCS_THRESH_PIVOTS;
  std::vector<double> piv(J), sums(J);
  CHECK(pcs_thresh_pick_host(PCS_F64, lo, hi, 0.0, nullptr, a, b, piv.data(), nullptr) == J);
  double sum_abs = 0.0;
  for (double v : x) sum_abs += fabs(v);
  int k = J + 1;
  for (int j = J; j >= 1; --j) {
    double s = 0.0;
    for (double v : x) s += fmax(fabs(v) - piv[j - 1], 0.0);
    sums[j - 1] = s;
    if (!(s - a - b * piv[j - 1] > 0.0)) k = j;
  }
  uint64_t br[2] = {~0ull, ~0ull};
  const int rc = pcs_thresh_pick_host(PCS_F64, lo, hi, sum_abs, sums.data(), a, b, nullptr, br);
  if (sum_abs <= a) {
    CHECK(rc == 0 && br[0] == 0 && br[1] == 0);
    return;
  }
  CHECK(rc == J);
  CHECK(expect_k < 0 || k == expect_k);
  CHECK(val64(br[0]) == (k == 1 ? val64(lo) : piv[k - 2]));
  CHECK(val64(br[1]) == (k == J + 1 ? val64(hi) : piv[k - 1]));
  CHECK(br[0] <= br[1] && br[1] <= hi && br[0] >= lo);
}

int main() {
  const int J = PCS_THRESH_PIVOTS;
  // a bracket of 32 * 4 keys starting at 1.0: pivot j is the key of 1.0 plus 4 j
  const uint64_t lo = key64(1.0), hi = lo + 32 * 4;
  const double p1 = val64(lo + 4), p16 = val64(lo + 64), p31 = val64(lo + 124);
  const std::vector<double> big = {val64(hi), -val64(hi), 0.5};
  // psi(p) = 2 (x_max - p) - a for p >= 0.5: place the root just below pivot 1, 16, 31 and above 31
  pick_case(big, 2 * (val64(hi) - val64(lo + 2)), 0.0, lo, hi, 1);
  pick_case(big, 2 * (val64(hi) - val64(lo + 62)), 0.0, lo, hi, 16);
  pick_case(big, 2 * (val64(hi) - val64(lo + 126)), 0.0, lo, hi, J + 1);
  pick_case(big, 2 * (val64(hi) - p16), 0.0, lo, hi, 16);  // psi exactly 0 on pivot 16: the tie closes the bracket
  pick_case(big, 2 * (val64(hi) - p1), 0.0, lo, hi, 1);
  pick_case(big, 2 * (val64(hi) - p31), 0.0, lo, hi, 31);
  pick_case(big, 1e9, 0.0, lo, hi, -1);                    // sum |x| <= a: t = 0
  pick_case(big, 0.0, 3.0, 0, key64(val64(hi)), -1);       // b > 0 from the full bracket
  // brackets narrower than the pivot count, and the full fp32 / fp64 key ranges
  for (uint64_t w = 0; w <= 40; ++w) pick_case(big, 0.25, 0.0, lo, lo + w, -1);
  uint64_t br[2];
  std::vector<double> zeros(J, 0.0), piv(J);
  CHECK(pcs_thresh_pick_host(PCS_F64, 0, 0x7fffffffffffffffull, 1.0, zeros.data(), 0.5, 0.0, piv.data(), br) == J);
  CHECK(br[0] == 0 && br[1] > 0);
  CHECK(pcs_thresh_pick_host(PCS_F32, 0, 0x7fffffffull, 1.0, zeros.data(), 0.5, 0.0, piv.data(), br) == J);
  CHECK(br[0] == 0 && br[1] == (0x7fffffffull + 31) / 32);
  // argument checks of the selection
  CHECK(pcs_thresh_pick_host(7, 0, 1, 1.0, zeros.data(), 0.5, 0.0, nullptr, br) == PCS_EINVAL);
  CHECK(pcs_thresh_pick_host(PCS_F64, 2, 1, 1.0, zeros.data(), 0.5, 0.0, nullptr, br) == PCS_EINVAL);
  CHECK(pcs_thresh_pick_host(PCS_F32, 0, 1ull << 31, 1.0, zeros.data(), 0.5, 0.0, nullptr, br) == PCS_EINVAL);
  CHECK(pcs_thresh_pick_host(PCS_F64, 0, 1, 1.0, zeros.data(), 0.0, 0.0, nullptr, br) == PCS_EINVAL);
  CHECK(pcs_thresh_pick_host(PCS_F64, 0, 1, 1.0, zeros.data(), 0.5, 0.0, nullptr, nullptr) == PCS_EINVAL);

  // argument checks of the device entry points: refused before any device call (the addresses are stand-ins)
  void* X = (void*)0x10000;
  void* O = (void*)0x20000;
  void* W = (void*)0x30000;
  CHECK(pcs_thresh_ws_bytes(-1) == PCS_EINVAL);
  CHECK(pcs_thresh_ws_bytes(0) > 0 && pcs_thresh_ws_bytes(1ll << 40) >= pcs_thresh_ws_bytes(70001));
  CHECK(pcs_thresh_l1(5, X, O, 8, 1.0, 0.0, PCS_THRESH_SOFT, nullptr, W, nullptr) == PCS_EINVAL);
  CHECK(pcs_thresh_l1(PCS_F32, X, O, -1, 1.0, 0.0, PCS_THRESH_SOFT, nullptr, W, nullptr) == PCS_EINVAL);
  CHECK(pcs_thresh_l1(PCS_F32, nullptr, O, 8, 1.0, 0.0, PCS_THRESH_SOFT, nullptr, W, nullptr) == PCS_EINVAL);
  CHECK(pcs_thresh_l1(PCS_F32, X, nullptr, 8, 1.0, 0.0, PCS_THRESH_SOFT, nullptr, W, nullptr) == PCS_EINVAL);
  CHECK(pcs_thresh_l1(PCS_F32, X, O, 8, 1.0, 0.0, PCS_THRESH_SOFT, nullptr, nullptr, nullptr) == PCS_EINVAL);
  CHECK(pcs_thresh_l1(PCS_F32, X, O, 8, 1.0, 0.0, PCS_THRESH_SOFT, nullptr, (void*)0x30004, nullptr) == PCS_EINVAL);
  CHECK(pcs_thresh_l1(PCS_F64, X, O, 8, -1.0, 0.0, PCS_THRESH_SOFT, nullptr, W, nullptr) == PCS_EINVAL);
  CHECK(pcs_thresh_l1(PCS_F64, X, O, 8, 1.0, -1.0, PCS_THRESH_SOFT, nullptr, W, nullptr) == PCS_EINVAL);
  CHECK(pcs_thresh_l1(PCS_F64, X, O, 8, 0.0, 0.0, PCS_THRESH_SOFT, nullptr, W, nullptr) == PCS_EINVAL);
  CHECK(pcs_thresh_l1(PCS_F64, X, O, 8, NAN, 0.0, PCS_THRESH_SOFT, nullptr, W, nullptr) == PCS_EINVAL);
  CHECK(pcs_thresh_l1(PCS_F64, X, O, 8, 1.0, 0.0, 2, nullptr, W, nullptr) == PCS_EINVAL);
  CHECK(pcs_thresh_l1(PCS_F64, X, O, 0, 1.0, 0.0, PCS_THRESH_CLIP, nullptr, W, nullptr) == PCS_OK);
  printf(fails ? "thresh_host_check: %d failure(s)\n" : "thresh_host_check: ok\n", fails);
  return fails ? 1 : 0;
}
