// What does one stream-to-stream edge cost the PRODUCING queue?  (round 8, profiles/r08_fork_edges.txt)
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 scripts/exp/fork_edge_cost.hip -o fork_edge_cost
//   ./fork_edge_cost [launches = 200] [repetitions = 21] [target_us = 20]
//
// Stream A runs a chain of `launches` element-wise kernels of about target_us each (every element += 1, so after
// launch i every element reads i + 1).  After each launch comes an edge to stream B and a short kernel on B that
// samples what the launch wrote.  The chain on A is timed (host clock from the first enqueue to A's drain, median of
// the repetitions) in these arms:
//   a0  the chain alone, nothing on B
//   a   consumers on B, no edges (the consumers race; not verified)
//   b   hipEventRecord(ev, A) + hipStreamWaitEvent(B, ev), event made with hipEventDisableTiming (the library's flags)
//   c   as b, event made with hipEventDisableTiming | hipEventReleaseToDevice
//   d   the launch made with hipExtLaunchKernelGGL(..., stopEvent = ev, ...), then hipStreamWaitEvent(B, ev) only
//   e   as d with the flags of c
//   d4, e4   as d, e with a ring of 4 events instead of one re-bound on every launch
// Per-edge cost = (arm - a) / launches.  Arms b .. e4 verify that consumer i read >= i + 1 in every sample (a later
// producer may have passed by then: the chain does not wait for B), with the samples weighted to the LAST blocks of
// the grid, which finish last: a wait that bound to the previous launch, or to nothing, reads i there.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(call)                                                                              \
  do {                                                                                           \
    hipError_t e__ = (call);                                                                     \
    if (e__ != hipSuccess) {                                                                     \
      fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e__));     \
      exit(1);                                                                                   \
    }                                                                                            \
  } while (0)

__global__ void __launch_bounds__(256) bump(uint32_t* __restrict__ x, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) x[i] += 1u;
}

constexpr int kSamples = 256;
// seen[t] = min over this thread's samples; half the threads sample the last 64 K elements, half the whole buffer
__global__ void __launch_bounds__(kSamples) sample(const uint32_t* __restrict__ x, int64_t n, uint32_t* __restrict__ seen) {
  const int t = threadIdx.x;
  const int64_t tail = n < 65536 ? n : 65536;
  int64_t i = t < kSamples / 2 ? n - 1 - (int64_t)t * (tail / (kSamples / 2)) : (int64_t)(t - kSamples / 2) * (n / (kSamples / 2));
  if (i < 0) i = 0;
  if (i >= n) i = n - 1;
  seen[t] = __builtin_nontemporal_load(x + i);
}

enum Arm { A0, A, B, C, D, E, D4, E4, N_ARMS };
const char* const kArmName[N_ARMS] = {"a0 chain alone", "a  no edges", "b  record+wait", "c  b, device-scope release",
                                      "d  stopEvent+wait", "e  d, device-scope release", "d4 d, ring of 4",
                                      "e4 e, ring of 4"};

int main(int argc, char** argv) {
  const int launches = argc > 1 ? atoi(argv[1]) : 200;
  const int reps = argc > 2 ? atoi(argv[2]) : 21;
  const double target_us = argc > 3 ? atof(argv[3]) : 20.0;
  if (launches < 1 || launches > 100000 || reps < 1 || target_us <= 0) return 2;

  hipStream_t sa, sb;
  CHECK(hipStreamCreateWithFlags(&sa, hipStreamNonBlocking));
  CHECK(hipStreamCreateWithFlags(&sb, hipStreamNonBlocking));
  const int64_t n_max = 64ll << 20;
  uint32_t *x, *seen;
  CHECK(hipMalloc(&x, n_max * sizeof(uint32_t)));
  CHECK(hipMalloc(&seen, (size_t)launches * kSamples * sizeof(uint32_t)));
  const unsigned grid = 256 * 8;

  // size the element-wise kernel to target_us
  int64_t n = 8ll << 20;
  for (int pass = 0; pass < 3; ++pass) {
    CHECK(hipMemsetAsync(x, 0, n_max * sizeof(uint32_t), sa));
    for (int i = 0; i < 20; ++i) bump<<<grid, 256, 0, sa>>>(x, n);
    CHECK(hipStreamSynchronize(sa));
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < 100; ++i) bump<<<grid, 256, 0, sa>>>(x, n);
    CHECK(hipStreamSynchronize(sa));
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / 100;
    int64_t next = (int64_t)((double)n * target_us / us) & ~(int64_t)1023;
    next = std::min(std::max(next, (int64_t)65536), n_max);
    printf("calibrate: n = %lld -> %.2f us per launch\n", (long long)n, us);
    n = next;
  }
  printf("chain: %d launches of %lld elements, %d repetitions\n", launches, (long long)n, reps);

  hipEvent_t ev[2][4];      // [0]: the library's flags, [1]: device-scope release
  for (int k = 0; k < 4; ++k) {
    CHECK(hipEventCreateWithFlags(&ev[0][k], hipEventDisableTiming));
    CHECK(hipEventCreateWithFlags(&ev[1][k], hipEventDisableTiming | hipEventReleaseToDevice));
  }

  std::vector<uint32_t> host((size_t)launches * kSamples);
  double median[N_ARMS], spread[N_ARMS];
  long long bad[N_ARMS] = {};
  for (int arm = 0; arm < N_ARMS; ++arm) {
    std::vector<double> times;
    for (int rep = 0; rep < reps + 2; ++rep) {        // two warm-up repetitions
      CHECK(hipMemsetAsync(x, 0, n * sizeof(uint32_t), sa));
      CHECK(hipMemsetAsync(seen, 0xFF, host.size() * sizeof(uint32_t), sa));
      CHECK(hipDeviceSynchronize());
      const int flavour = (arm == C || arm == E || arm == E4) ? 1 : 0;
      const int ring = (arm == D4 || arm == E4) ? 4 : 1;
      const auto t0 = std::chrono::steady_clock::now();
      for (int i = 0; i < launches; ++i) {
        hipEvent_t e = ev[flavour][i % ring];
        if (arm >= D) {
          hipExtLaunchKernelGGL(bump, dim3(grid), dim3(256), 0, sa, nullptr, e, 0, x, n);
          CHECK(hipStreamWaitEvent(sb, e, 0));
        } else {
          bump<<<grid, 256, 0, sa>>>(x, n);
          if (arm == B || arm == C) {
            CHECK(hipEventRecord(e, sa));
            CHECK(hipStreamWaitEvent(sb, e, 0));
          }
        }
        if (arm != A0) sample<<<1, kSamples, 0, sb>>>(x, n, seen + (size_t)i * kSamples);
      }
      CHECK(hipGetLastError());
      const auto t_issued = std::chrono::steady_clock::now();
      CHECK(hipStreamSynchronize(sa));
      const auto t1 = std::chrono::steady_clock::now();
      CHECK(hipStreamSynchronize(sb));
      if (rep >= 2) times.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
      if (rep == 2)
        printf("  [%s] host issue %.0f us of %.0f us\n", kArmName[arm],
               std::chrono::duration<double, std::micro>(t_issued - t0).count(), times.back());
      if (arm >= B) {
        CHECK(hipMemcpy(host.data(), seen, host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (int i = 0; i < launches; ++i)
          for (int t = 0; t < kSamples; ++t)
            if (host[(size_t)i * kSamples + t] < (uint32_t)(i + 1) || host[(size_t)i * kSamples + t] > (uint32_t)launches)
              ++bad[arm];
      }
    }
    std::sort(times.begin(), times.end());
    median[arm] = times[times.size() / 2];
    spread[arm] = times[times.size() * 3 / 4] - times[times.size() / 4];
  }

  printf("\n%-30s %12s %10s %14s %10s\n", "arm", "chain us", "iqr us", "per edge us", "stale");
  for (int arm = 0; arm < N_ARMS; ++arm)
    printf("%-30s %12.1f %10.1f %14.3f %10lld\n", kArmName[arm], median[arm], spread[arm],
           arm <= A ? 0.0 : (median[arm] - median[A]) / launches, arm >= B ? bad[arm] : -1ll);
  long long all_bad = 0;
  for (int arm = B; arm < N_ARMS; ++arm) all_bad += bad[arm];
  return all_bad ? 3 : 0;
}
