// Launch-order probe: can half of the C3 iterate stay in the Infinity Cache between two iterations?
// Seven R x 4096 fp32 arrays in the step's ping-pong roles (x, z0, z1 in two parities, and C^T y): iteration i
// reads x[p], b, z0[p], z1[p] and writes x[1-p], z0[1-p], z1[1-p], p = i & 1.  Memory only, the 64-column strip
// march of tools/strip_probe.hip (16 rows per workgroup step), about 768 tasks per launch.  Schedules:
//   (a) one launch per iteration over all rows
//   (b) two launches per iteration, rows [0, m) then [m, R), the same order every iteration:  T B | T B
//   (c) two launches per iteration, the order alternating with the parity:                     T B | B T
// In (c) every second band launch follows the previous iteration's launch on the same band, with only that
// band's own seven half-arrays (7 * R/2 * 16 KiB) touched in between.
//   hipcc --offload-arch=gfx950 -O3 -o tools/ic_pair_probe tools/ic_pair_probe.hip && tools/ic_pair_probe
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      return 1;                                                                 \
    }                                                                           \
  } while (0)

constexpr int N1 = 4096;     // columns
constexpr int RMAX = 4096;   // rows allocated
constexpr int W = 64, G = W / 4, RPS = 256 / G;  // strip width, float4 groups per row, rows per step (16)
constexpr int kTasks = 768;

struct Arr {
  const float4* in[4];
  float4* out[3];
};

// task = (segment, strip): rows [lo + seg * L, min(lo + seg * L + L, hi)) of columns [strip * W, strip * W + W)
__global__ __launch_bounds__(256) void k_band(Arr a, int nstrips, int L, int lo, int hi) {
  const int task = blockIdx.x, seg = task / nstrips, strip = task - seg * nstrips;
  const int g = threadIdx.x % G, r0 = threadIdx.x / G;
  const int64_t col4 = (int64_t)strip * G + g;
  const int beg = lo + seg * L, end = min(beg + L, hi);
  for (int r = beg + r0; r < end; r += RPS) {
    const int64_t o = (int64_t)r * (N1 / 4) + col4;
    const float4 v0 = a.in[0][o], v1 = a.in[1][o], v2 = a.in[2][o], v3 = a.in[3][o];
    a.out[0][o] = make_float4(v0.x + v1.x, v0.y + v1.y, v0.z + v1.z, v0.w + v1.w);
    a.out[1][o] = make_float4(v2.x + v3.x, v2.y + v3.y, v2.z + v3.z, v2.w + v3.w);
    a.out[2][o] = make_float4(v0.x + v3.x, v0.y + v3.y, v0.z + v3.z, v0.w + v3.w);
  }
}

struct Bufs {
  float4 *x[2], *z0[2], *z1[2], *b;
};

static Arr roles(const Bufs& B, int p) {
  Arr a;
  a.in[0] = B.x[p], a.in[1] = B.b, a.in[2] = B.z0[p], a.in[3] = B.z1[p];
  a.out[0] = B.x[1 - p], a.out[1] = B.z0[1 - p], a.out[2] = B.z1[1 - p];
  return a;
}

// rows [lo, hi) in about kTasks tasks of whole 16-row steps
static void launch_band(const Arr& a, int lo, int hi) {
  const int nstrips = N1 / W;
  const int steps = (hi - lo + RPS - 1) / RPS;
  const int nseg = std::max(1, std::min(kTasks / nstrips, steps));
  const int L = (steps + nseg - 1) / nseg * RPS;
  const int used = (hi - lo + L - 1) / L;
  k_band<<<nstrips * used, 256>>>(a, nstrips, L, lo, hi);
}

enum Sched { ONE = 0, FIXED = 1, PAIRED = 2 };

static void iterate(const Bufs& B, int rows, Sched s, int i) {
  const Arr a = roles(B, i & 1);
  if (s == ONE) {
    launch_band(a, 0, rows);
    return;
  }
  const int m = (rows / 2 + RPS - 1) / RPS * RPS;
  const bool top_first = s == FIXED || (i & 1) == 0;
  if (top_first) launch_band(a, 0, m), launch_band(a, m, rows);
  else launch_band(a, m, rows), launch_band(a, 0, m);
}

// median over `reps` timed blocks of `iters` iterations each (an even count: both parities, both orders)
static int time_sched(const Bufs& B, int rows, Sched s, int iters, int reps, double* med, double* lo, double* hi) {
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int i = 0; i < 4; ++i) iterate(B, rows, s, i);
  std::vector<double> us;
  for (int r = 0; r < reps; ++r) {
    CK(hipEventRecord(e0));
    for (int i = 0; i < iters; ++i) iterate(B, rows, s, i);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    us.push_back(ms * 1e3 / iters);
  }
  CK(hipGetLastError());
  std::sort(us.begin(), us.end());
  *med = us[us.size() / 2], *lo = us.front(), *hi = us.back();
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  return 0;
}

int main() {
  Bufs B;
  const size_t bytes = (size_t)RMAX * N1 * 4;
  float4** all[7] = {&B.x[0], &B.x[1], &B.z0[0], &B.z0[1], &B.z1[0], &B.z1[1], &B.b};
  for (auto pp : all) {
    void* p;
    CK(hipMalloc(&p, bytes));
    CK(hipMemset(p, 0, bytes));
    *pp = (float4*)p;
  }
  CK(hipDeviceSynchronize());
  const char* names[3] = {"a_one_launch", "b_bands_fixed_TB_TB", "c_bands_paired_TB_BT"};
  const int iters = 24, reps = 7;
  for (int pass = 0; pass < 2; ++pass) {
    for (int rows : {4096, 3584, 3072, 2560, 2048}) {
      const double set_mib = 7.0 * rows * N1 * 4 / (1 << 20);
      for (int s = 0; s < 3; ++s) {
        if (rows != 4096 && s == FIXED) continue;
        double med, lo, hi;
        if (time_sched(B, rows, (Sched)s, iters, reps, &med, &lo, &hi)) return 1;
        const double algo = 7.0 * rows * N1 * 4;
        printf("{\"pass\": %d, \"rows\": %d, \"set_MiB\": %.0f, \"half_set_MiB\": %.0f, \"schedule\": \"%s\", "
               "\"us_per_iter\": %.2f, \"min\": %.2f, \"max\": %.2f, \"algo_TBps\": %.3f}\n",
               pass, rows, set_mib, set_mib / 2, names[s], med, lo, hi, algo / (med * 1e-6) / 1e12);
        fflush(stdout);
      }
    }
  }
  CK(hipDeviceSynchronize());
  return 0;
}
