// Stand-alone check of pycsou_amd/csrc/mcmc_core.hpp on the CPU (no HIP, nothing loaded into Python):
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/mcmc_core_check.cpp -o build/mcmc_core_check && build/mcmc_core_check
//
// Drives the P2 element update over five kinds of stream (Gaussian, values rounded to 0.5, strictly ascending,
// strictly descending, Cauchy; one constant column), in float and double, for three p-values, and asserts after
// every sample: heights non-decreasing, positions strictly increasing, the ends at 1 and count.  Then the
// Philox4x32-10 known answers and the range of the normals.  Exits 0 when everything holds.
#include <stdio.h>
#include <stdlib.h>

#include "../pycsou_amd/csrc/mcmc_core.hpp"

static int failures = 0;
#define CHECK(cond, ...)          \
  do {                            \
    if (!(cond)) {                \
      ++failures;                 \
      printf("FAIL %s: ", #cond); \
      printf(__VA_ARGS__);        \
      printf("\n");               \
    }                             \
  } while (0)

enum { GAUSS, TIES, ASC, DESC, CAUCHY, NKIND };
static const char* kNames[NKIND] = {"gauss", "ties", "ascending", "descending", "cauchy"};

// sample t of column col of a stream, built from the header's own normals
static double stream_value(int kind, int col, int t, double* run) {
  float z[4];
  pcs::mcmc_normal4(1234u + kind, (uint32_t)t, 9u, (uint64_t)col, z);
  if (col == 0) return 0.75;
  switch (kind) {
    case GAUSS: return z[0];
    case TIES: return floor(2.0 * z[0] + 0.5) / 2.0 + 0.0;
    case ASC: *run += 0.05 + fabs((double)z[1]); return *run;
    case DESC: *run -= 0.05 + fabs((double)z[1]); return *run;
    default: return (double)z[0] / (fabs((double)z[1]) + 1e-3);
  }
}

template <typename T>
static void drive(int kind, double p, const char* tname) {
  const int width = 67, samples = 200;
  static T q[67][5];
  static int n[67][5];
  static double run[67];
  for (int c = 0; c < width; ++c) run[c] = 0.0;
  double des[5] = {1, 1 + 2 * p, 1 + 4 * p, 3 + 2 * p, 5};
  const double inc[5] = {0, p / 2, p, (p + 1) / 2, 1};
  long par_or_lin = 0;
  for (int t = 1; t <= samples; ++t) {
    if (t > 5)
      for (int m = 0; m < 5; ++m) des[m] += inc[m];
    for (int c = 0; c < width; ++c) {
      const T s = (T)stream_value(kind, c, t, &run[c]);
      T before2 = q[c][2];
      pcs::p2_add_el<T>(s, q[c], n[c], t, des);
      const int valid = t < 5 ? t : 5;
      for (int m = 1; m < valid; ++m)
        CHECK(q[c][m - 1] <= q[c][m], "%s %s p=%g t=%d col=%d marker %d: %g > %g", kNames[kind], tname, p, t, c, m,
              (double)q[c][m - 1], (double)q[c][m]);
      if (t >= 5) {
        CHECK(n[c][0] == 1 && n[c][4] == t, "%s %s t=%d col=%d ends %d %d", kNames[kind], tname, t, c, n[c][0],
              n[c][4]);
        for (int m = 1; m < 5; ++m)
          CHECK(n[c][m - 1] < n[c][m], "%s %s t=%d col=%d positions %d %d", kNames[kind], tname, t, c, n[c][m - 1],
                n[c][m]);
      }
      if (t > 5 && before2 != q[c][2]) ++par_or_lin;
    }
  }
  CHECK(par_or_lin > 0, "%s %s p=%g: the middle marker never moved", kNames[kind], tname, p);
}

int main() {
  const uint32_t kat[3][10] = {
      {0, 0, 0, 0, 0, 0, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
      {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu,
       0xa20bc7c6u, 0x6d5451fdu},
      {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu,
       0x5001e420u, 0x24126ea1u}};
  for (const auto& k : kat) {
    const uint32_t c[4] = {k[0], k[1], k[2], k[3]}, key[2] = {k[4], k[5]};
    uint32_t o[4];
    pcs::philox4x32_10(c, key, o);
    for (int j = 0; j < 4; ++j) CHECK(o[j] == k[6 + j], "philox word %d: %08x != %08x", j, o[j], k[6 + j]);
  }
  double sum = 0.0, sq = 0.0;
  const int nb = 16384;
  for (int b = 0; b < nb; ++b) {
    float z[4];
    pcs::mcmc_normal4(77u, 3u, 0u, (uint64_t)b, z);
    for (float v : z) {
      CHECK(isfinite(v) && fabsf(v) < 5.8f, "normal out of range: %g", (double)v);
      sum += v;
      sq += (double)v * v;
    }
  }
  const double n = 4.0 * nb, mean = sum / n, var = sq / n - mean * mean;
  CHECK(fabs(mean) <= 5 / sqrt(n) && fabs(var - 1) <= 5 * sqrt(2 / n), "mean %g var %g", mean, var);
  const double ps[3] = {0.1, 0.5, 0.9};
  for (int kind = 0; kind < NKIND; ++kind)
    for (double p : ps) {
      drive<double>(kind, p, "double");
      drive<float>(kind, p, "float");
    }
  printf(failures ? "mcmc_core_check: %d failures\n" : "mcmc_core_check: ok\n", failures);
  return failures ? 1 : 0;
}
