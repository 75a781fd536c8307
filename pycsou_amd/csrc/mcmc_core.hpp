// Shared core of the PMYULA sampler (mcmc.hip): the Philox4x32-10 generator, its mapping to standard
// normals, and the single-element P-square (P2) streaming-quantile update.  Compiles under hipcc (used by the
// kernels and by the host twins pcs_mcmc_*_host / pcs_p2_update_host) and as plain C++
// (tools/mcmc_core_check.cpp), the same pattern as pcs_thresh_pick_host.
//
// Noise contract (part of the ABI: a chain is reproducible from its seed alone)
// -----------------------------------------------------------------------------
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (b & 0xffffffff, iteration, stream_id, b >> 32),  b = element_index / 4   (b < 2^32: word 3 is 0)
//   words w0..w3 = Philox4x32-10(counter, key); element 4 b + j takes
//     j = 0: r(w0) cos(2 pi v(w1))   j = 1: r(w0) sin(2 pi v(w1))
//     j = 2: r(w2) cos(2 pi v(w3))   j = 3: r(w2) sin(2 pi v(w3))
//   r(w) = sqrt(-2 ln u), u = ((w >> 8) + 1) 2^-24 in (0, 1];   v(w) = (w >> 8) 2^-24 in [0, 1)
// Box-Muller runs in fp32 (|z| <= 5.77) and is widened for fp64 chains.  A value depends on the seed, the
// iteration, the stream and the element index only, never on the grid shape.
#pragma once

#include <math.h>
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace pcs {

__host__ __device__ inline void philox4x32_10(const uint32_t (&ctr)[4], const uint32_t (&key)[2], uint32_t (&out)[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// the four raw words of block b (see the contract above)
__host__ __device__ inline void mcmc_words(uint64_t seed, uint32_t iter, uint32_t stream, uint64_t b,
                                           uint32_t (&w)[4]) {
  const uint32_t c[4] = {(uint32_t)b, iter, stream, (uint32_t)(b >> 32)};
  const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  philox4x32_10(c, k, w);
}

// the four standard normals of block b: elements 4 b .. 4 b + 3
__host__ __device__ inline void mcmc_normal4(uint64_t seed, uint32_t iter, uint32_t stream, uint64_t b,
                                             float (&z)[4]) {
  uint32_t w[4];
  mcmc_words(seed, iter, stream, b, w);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u = (float)((w[2 * h] >> 8) + 1u) * 5.9604644775390625e-8f;  // 2^-24
    const float v = (float)(w[2 * h + 1] >> 8) * 5.9604644775390625e-8f;
    const float r = sqrtf(-2.0f * logf(u));
    const float a = 6.2831853071795864769f * v;
    z[2 * h] = r * cosf(a);
    z[2 * h + 1] = r * sinf(a);
  }
}

// One sample of one P2 estimator (pycsou/util/stats.py:79-132), operation for operation.
//   q[5]  marker heights, ascending; q[0 .. count - 2] are valid on entry while count <= 5
//   n[5]  marker positions (1-based); valid from count >= 5, n[0] == 1, n[4] == count - 1 on entry
//   count number of samples including this one;  des[5] desired positions *after* this sample's increment
// count <= 5 is the warm-up: the sample is inserted into the sorted heights (np.sort of the concatenation) and
// sample 5 sets the positions to 1..5.  From the sixth sample on: cell selection with the two end replacements,
// position shift, then for markers 1..3 the parabolic formula, or the linear one when the parabolic result
// leaves (q[i-1], q[i+1]).  d is formed in double; the height arithmetic runs in T in the reference's order and
// must not be contracted to FMA (the branch q[i-1] < q_temp < q[i+1] decides as the reference does).
template <typename T>
__host__ __device__ inline void p2_add_el(T s, T (&q)[5], int (&n)[5], int64_t count, const double* des) {
#pragma clang fp contract(off)
  if (count <= 5) {
    T cur = s;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      if (m < count - 1) {
        if (q[m] > cur) {
          const T t = q[m];
          q[m] = cur;
          cur = t;
        }
      } else if (m == count - 1) {
        q[m] = cur;
      }
    }
    if (count == 5) {
#pragma unroll
      for (int m = 0; m < 5; ++m) n[m] = m + 1;
    }
    return;
  }
  int k;
  if (s < q[0]) {
    q[0] = s;
    k = 0;
  } else if (q[0] <= s && s < q[1]) {
    k = 0;
  } else if (q[1] <= s && s < q[2]) {
    k = 1;
  } else if (q[2] <= s && s < q[3]) {
    k = 2;
  } else if (q[3] <= s && s < q[4]) {
    k = 3;
  } else {
    q[4] = s;
    k = 3;
  }
#pragma unroll
  for (int t = 0; t < 5; ++t) n[t] += (t > k) ? 1 : 0;
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const double d = des[i] - (double)n[i];
    if ((d >= 1.0 && n[i + 1] - n[i] > 1) || (d <= -1.0 && n[i - 1] - n[i] < -1)) {
      const int sd = d > 0.0 ? 1 : -1;
      const T dt = (T)sd;
      const T t1 = ((T)(n[i] - n[i - 1] + sd) * (q[i + 1] - q[i])) / (T)(n[i + 1] - n[i]);
      const T t2 = ((T)(n[i + 1] - n[i] - sd) * (q[i] - q[i - 1])) / (T)(n[i] - n[i - 1]);
      const T qt = q[i] + (dt / (T)(n[i + 1] - n[i - 1])) * (t1 + t2);
      if (q[i - 1] < qt && qt < q[i + 1]) {
        q[i] = qt;
      } else {
        const T qo = sd > 0 ? q[i + 1] : q[i - 1];
        const int no = sd > 0 ? n[i + 1] : n[i - 1];
        q[i] = q[i] + (dt * (qo - q[i])) / (T)(no - n[i]);
      }
      n[i] += sd;
    }
  }
}

}  // namespace pcs
