// Cumulative sum along one axis of an N-D C-order array: Integration1D (pycsou/linop/diff.py:1071-1137 ->
// PyLops 1.x CausalIntegration, halfcurrent=False) and its adjoint (the same sum run backwards).
//
// The axis is the middle of (outer, n, inner).  Two layouts:
//   strided   (inner > 1, or a line shorter than a wave): one thread per (line, segment) marches along n;
//             neighbouring threads hold neighbouring `inner` columns, so every step's loads are coalesced.
//   contiguous (inner == 1): one wave per (line, segment); each lane takes kV consecutive samples of a
//             512-sample chunk (whole chunks with 16-byte loads and stores, two chunks in flight), the lane
//             totals are scanned with __shfl_up and the chunk's total is carried.
// When the lines alone cannot fill the device a line is cut into segments and handled reduce-then-scan
// in three launches -- segment totals into ws, an exclusive scan of each line's totals, the offset scan.
// Stream order is the only dependency between them: no workgroup waits for another inside a launch.
// Sums are carried in fp64 for both dtypes; `step` multiplies the finished sum.  Every sample is read and
// written by the same thread (the totals pass only reads), so out may alias x.
#include "common.hpp"

namespace pcs {

static constexpr int kScanDims = 32;
static constexpr int kV = 8;                    // samples per lane and chunk (contiguous layout)
static constexpr int kChunk = kWave * kV;       // 512
static constexpr int kTotK = 16;                // totals per thread in k_scan_totals
static constexpr int kTotThreads = 512;
static constexpr int64_t kMaxSeg = kTotThreads * kTotK;  // 8192 segments per line at most
static constexpr int64_t kEnoughLines = 4096;   // contiguous: this many lines (one wave each) are never split
static constexpr int64_t kTargetWaves = 8192;   // contiguous: (line, segment) units wanted below that
static constexpr int64_t kTargetThreads = 131072;  // strided: (line, segment) threads wanted

struct ScanPlan {
  int64_t outer, n, inner, lines;
  int64_t seg, nseg;  // segment length and segments per line of this launch
  int64_t cap;        // upper bound of nseg that never decreases in n (the workspace size)
  int contig;
};

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// 0: plan made, 1: empty array, -1: bad arguments
static int make_plan(int ndim, const int64_t* dims, int axis, ScanPlan& P) {
  if (ndim < 1 || ndim > kScanDims || dims == nullptr || axis < 0 || axis >= ndim) return -1;
  int64_t outer = 1, inner = 1;
  bool empty = false;
  for (int i = 0; i < ndim; ++i) {
    if (dims[i] < 0) return -1;
    if (dims[i] == 0) empty = true;
    if (i < axis) outer *= dims[i];
    if (i > axis) inner *= dims[i];
  }
  if (empty) return 1;
  P.outer = outer, P.n = dims[axis], P.inner = inner, P.lines = outer * inner;
  P.contig = (inner == 1 && P.n >= kWave) ? 1 : 0;
  const int64_t target = P.contig ? kTargetWaves : kTargetThreads;
  const int64_t span = P.contig ? PCS_CUMSUM_SPAN : PCS_CUMSUM_SPAN_STRIDED;
  const int64_t round = P.contig ? kChunk : 4;
  int64_t want = (P.contig && P.lines >= kEnoughLines) ? 1 : cdiv(target, P.lines);
  want = want < 1 ? 1 : (want > kMaxSeg ? kMaxSeg : want);
  int64_t seg = cdiv(cdiv(P.n, want), round) * round;
  if (seg < span) seg = span;
  P.seg = seg;
  P.nseg = cdiv(P.n, seg);  // <= want (seg >= n / want) and <= ceil(n / span)
  const int64_t by_span = cdiv(P.n, span);
  P.cap = want < by_span ? want : by_span;
  return 0;
}

__device__ __forceinline__ int64_t scan_pos(int64_t r, int64_t n, int rev) { return rev ? n - 1 - r : r; }

// TOTALS: ws[line * nseg + sg] = sum of the segment; otherwise the scan of the segment from the carried
// prefix ws[line * nseg + sg] (0 without a workspace)
template <typename T, bool TOTALS>
__global__ void k_scan_strided(const T* x, T* out, double* ws, ScanPlan P, double step, int rev, int use_ws) {
  const int64_t work = P.outer * P.nseg * P.inner;
  for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < work; w += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = w % P.inner, t = w / P.inner, sg = t % P.nseg, o = t / P.nseg;
    const int64_t slot = (o * P.inner + j) * P.nseg + sg;
    const int64_t r0 = sg * P.seg, r1 = (r0 + P.seg < P.n) ? r0 + P.seg : P.n;
    const int64_t base = o * P.n * P.inner + j;
    double acc = (!TOTALS && use_ws) ? ws[slot] : 0.0;
    int64_t r = r0;
    for (; r + 4 <= r1; r += 4) {
      int64_t q[4];
      T a[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) q[e] = base + scan_pos(r + e, P.n, rev) * P.inner;
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = x[q[e]];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc += (double)a[e];
        if (!TOTALS) out[q[e]] = (T)(acc * step);
      }
    }
    for (; r < r1; ++r) {
      const int64_t q = base + scan_pos(r, P.n, rev) * P.inner;
      acc += (double)x[q];
      if (!TOTALS) out[q] = (T)(acc * step);
    }
    if (TOTALS) ws[slot] = acc;
  }
}

// Inclusive scan of one value per lane across the wave; returns the inclusive value, and through excl /
// total the exclusive value and the wave's sum
__device__ __forceinline__ double wave_scan(double s, int lane, double& excl, double& total) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const double t = __shfl_up(s, d, kWave);
    if (lane >= d) s += t;
  }
  excl = __shfl_up(s, 1, kWave);
  if (lane == 0) excl = 0.0;
  total = __shfl(s, kWave - 1, kWave);
  return s;
}

template <typename T, bool TOTALS>
__global__ void k_scan_contig(const T* x, T* out, double* ws, ScanPlan P, double step, int rev, int use_ws) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t units = P.lines * P.nseg;
  for (int64_t u = wave; u < units; u += nwaves) {  // u is the same in all lanes of a wave
    const int64_t sg = u % P.nseg, line = u / P.nseg;
    const int64_t r0 = sg * P.seg, r1 = (r0 + P.seg < P.n) ? r0 + P.seg : P.n;
    const int64_t base = line * P.n;
    if (TOTALS) {
      double s4[4] = {0.0, 0.0, 0.0, 0.0};  // four independent chains: the loads of a step go out together
      for (int64_t r = r0 + lane; r < r1; r += 4 * kWave) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (r + k * kWave < r1) s4[k] += (double)x[base + scan_pos(r + k * kWave, P.n, rev)];
      }
      double s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
      s = wave_sum(s);
      if (lane == 0) ws[u] = s;
    } else {
      double carry = use_ws ? ws[u] : 0.0;
      for (int64_t c0 = r0; c0 < r1; c0 += 2 * kChunk) {  // two chunks a step: both chunks' loads first
        double v[2][kV];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int64_t rl = c0 + h * kChunk + (int64_t)lane * kV;
          if (c0 + (h + 1) * kChunk <= r1) {
            // a whole chunk: the lane's kV samples are consecutive in memory in either direction, so they
            // are loaded unconditionally in address order (wide loads) and put in scan order in registers
            const T* p = x + base + (rev ? P.n - kV - rl : rl);
            T t[kV];
#pragma unroll
            for (int e = 0; e < kV; ++e) t[e] = p[e];
#pragma unroll
            for (int e = 0; e < kV; ++e) v[h][e] = (double)(rev ? t[kV - 1 - e] : t[e]);
          } else {
#pragma unroll
            for (int e = 0; e < kV; ++e)
              v[h][e] = (rl + e < r1) ? (double)x[base + scan_pos(rl + e, P.n, rev)] : 0.0;
          }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int64_t rl = c0 + h * kChunk + (int64_t)lane * kV;
#pragma unroll
          for (int e = 1; e < kV; ++e) v[h][e] += v[h][e - 1];
          double excl, total;
          wave_scan(v[h][kV - 1], lane, excl, total);
          const double off = carry + excl;
          if (c0 + (h + 1) * kChunk <= r1) {
            T* p = out + base + (rev ? P.n - kV - rl : rl);
            T t[kV];
#pragma unroll
            for (int e = 0; e < kV; ++e) t[e] = (T)((off + v[h][e]) * step);
#pragma unroll
            for (int e = 0; e < kV; ++e) p[e] = rev ? t[kV - 1 - e] : t[e];
          } else {
#pragma unroll
            for (int e = 0; e < kV; ++e)
              if (rl + e < r1) out[base + scan_pos(rl + e, P.n, rev)] = (T)((off + v[h][e]) * step);
          }
          carry += total;
        }
      }
    }
  }
}

// Exclusive scan of each line's nseg <= kTotThreads * kTotK totals, in place: one workgroup per line
__global__ void __launch_bounds__(kTotThreads) k_scan_totals(double* ws, int64_t lines, int64_t nseg) {
  __shared__ double sm[kTotThreads / kWave];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  for (int64_t line = blockIdx.x; line < lines; line += gridDim.x) {
    double* w = ws + line * nseg;
    const int64_t i0 = (int64_t)threadIdx.x * kTotK;
    double v[kTotK];
#pragma unroll
    for (int e = 0; e < kTotK; ++e) v[e] = (i0 + e < nseg) ? w[i0 + e] : 0.0;
    double run = 0.0;
#pragma unroll
    for (int e = 0; e < kTotK; ++e) {  // v[e] <- exclusive prefix inside the thread
      const double t = v[e];
      v[e] = run;
      run += t;
    }
    double excl, total;
    wave_scan(run, lane, excl, total);
    if (lane == 0) sm[wid] = total;
    __syncthreads();
    double woff = 0.0;
    for (int k = 0; k < wid; ++k) woff += sm[k];
    const double off = woff + excl;
#pragma unroll
    for (int e = 0; e < kTotK; ++e)
      if (i0 + e < nseg) w[i0 + e] = off + v[e];
    __syncthreads();  // sm is rewritten by the next line
  }
}

template <typename T>
static int cumsum(const void* xv, void* outv, const ScanPlan& P, double step, int rev, void* wsv, hipStream_t st) {
  const T* x = (const T*)xv;
  T* out = (T*)outv;
  double* ws = (double*)wsv;
  const int split = P.nseg > 1 ? 1 : 0;
  if (P.contig) {
    const unsigned grid = grid_for(P.lines * P.nseg * kWave, 256);
    if (split) {
      k_scan_contig<T, true><<<grid, 256, 0, st>>>(x, out, ws, P, step, rev, 1);
      k_scan_totals<<<grid_for(P.lines * kTotThreads, kTotThreads), kTotThreads, 0, st>>>(ws, P.lines, P.nseg);
    }
    k_scan_contig<T, false><<<grid, 256, 0, st>>>(x, out, ws, P, step, rev, split);
  } else {
    const unsigned grid = grid_for(P.lines * P.nseg, 256);
    if (split) {
      k_scan_strided<T, true><<<grid, 256, 0, st>>>(x, out, ws, P, step, rev, 1);
      k_scan_totals<<<grid_for(P.lines * kTotThreads, kTotThreads), kTotThreads, 0, st>>>(ws, P.lines, P.nseg);
    }
    k_scan_strided<T, false><<<grid, 256, 0, st>>>(x, out, ws, P, step, rev, split);
  }
  return launch_status();
}

}  // namespace pcs

using namespace pcs;

extern "C" {

int64_t pcs_cumsum_ws_bytes(int ndim, const int64_t* dims, int axis) {
  ScanPlan P;
  const int rc = make_plan(ndim, dims, axis, P);
  if (rc < 0) return -1;
  if (rc > 0 || P.cap <= 1) return 0;
  return P.lines * P.cap * (int64_t)sizeof(double);
}

int pcs_cumsum(int dt, const void* x, void* out, int ndim, const int64_t* dims, int axis, double step, int reverse,
               void* ws, hipStream_t st) {
  if ((dt != PCS_F32 && dt != PCS_F64) || !x || !out) return PCS_EINVAL;
  ScanPlan P;
  const int rc = make_plan(ndim, dims, axis, P);
  if (rc < 0) return PCS_EINVAL;
  if (rc > 0) return PCS_OK;
  if ((P.cap > 1 || P.nseg > 1) && (!ws || ((uintptr_t)ws & 7u))) return PCS_EINVAL;
  const int rev = reverse ? 1 : 0;
  return dt == PCS_F32 ? cumsum<float>(x, out, P, step, rev, ws, st) : cumsum<double>(x, out, P, step, rev, ws, st);
}

}  // extern "C"
