// dist_profile.hip -- K17: the distance profile of cloud pairs, for gfx950.  The definition is in include/fpsg_hip.h
// (K17) and DESIGN.md: per pair and direction, how many of K1's squared nearest-neighbour distances lie at or under
// each of T squared thresholds (the numerators of precision and recall at a distance, F-score), and the largest of
// them (the directed Hausdorff distance, squared).
//
// Structure:
//   * one workgroup of 256 threads per (pair, direction), grid (B, 2); thread `tid` reads the elements tid, tid + 256,
//     ... of its row with plain dword loads (a row starts at b n 4 bytes: nothing wider is aligned), four in flight;
//   * the thresholds are read once; a thread keeps FPSG_PROFILE_MAX_T integer counters and one running maximum in
//     registers, the threshold loop unrolled over the compile-time maximum (a slot beyond T holds NaN and counts
//     nothing);
//   * the counters are added over the wave in registers (DPP, swizzle, half-wave swap), lane 0 of every wave leaves
//     them in LDS (4 x 17 dwords), and after the one barrier lanes t < T of the first wave add the four and store;
//   * integers and a maximum: the result does not depend on any order, so it is exact and the same bits on every run,
//     whatever B is.  No atomics, no workspace, nothing between workgroups; every trip count comes from N, M and T.
#include "fpsg_common.h"

namespace fpsg {
namespace {

constexpr int kProfileThreads = 256;
constexpr int kProfileWaves = kProfileThreads / kWave;
constexpr int kProfileInFlight = 4;                    // loads a thread issues before it uses the first

// one element: fp32 `<=` against every threshold (NaN on either side: false), and the running maximum, which starts
// at +0 and moves only on `>` -- a NaN and -0 never enter it
__device__ __forceinline__ void profile_take(float v, const float (&tau)[FPSG_PROFILE_MAX_T],
                                             int (&cnt)[FPSG_PROFILE_MAX_T], float& mx) {
#pragma unroll
  for (int t = 0; t < FPSG_PROFILE_MAX_T; ++t) cnt[t] += v <= tau[t] ? 1 : 0;
  mx = v > mx ? v : mx;
}

__global__ __launch_bounds__(kProfileThreads) void dist_profile_kernel(const float* __restrict__ dist1,
                                                                       const float* __restrict__ dist2, int N, int M,
                                                                       const float* __restrict__ tau2, int T,
                                                                       int* __restrict__ counts,
                                                                       float* __restrict__ maxima) {
  __shared__ int s_cnt[kProfileWaves][FPSG_PROFILE_MAX_T];
  __shared__ float s_max[kProfileWaves];

  const unsigned tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const unsigned b = blockIdx.x, dir = blockIdx.y;
  const unsigned n = (unsigned)(dir ? M : N);
  const float* row = (dir ? dist2 : dist1) + (size_t)b * n;

  float tau[FPSG_PROFILE_MAX_T];
  int cnt[FPSG_PROFILE_MAX_T];
#pragma unroll
  for (int t = 0; t < FPSG_PROFILE_MAX_T; ++t) {
    tau[t] = t < T ? tau2[t] : __builtin_nanf("");
    cnt[t] = 0;
  }
  float mx = 0.0f;

  // n < 2^31, so i + 3 * 256 cannot wrap an unsigned
  unsigned i = tid;
  for (; i + (kProfileInFlight - 1) * kProfileThreads < n; i += kProfileInFlight * kProfileThreads) {
    float v[kProfileInFlight];
#pragma unroll
    for (int k = 0; k < kProfileInFlight; ++k) v[k] = row[i + k * kProfileThreads];
#pragma unroll
    for (int k = 0; k < kProfileInFlight; ++k) profile_take(v[k], tau, cnt, mx);
  }
  for (; i < n; i += kProfileThreads) profile_take(row[i], tau, cnt, mx);

#pragma unroll
  for (int t = 0; t < FPSG_PROFILE_MAX_T; ++t) cnt[t] = wave_sum(cnt[t]);
  mx = wave_max(mx);                                    // the operands are >= +0 and never NaN (profile_take)
  if ((tid & 63u) == 0) {
#pragma unroll
    for (int t = 0; t < FPSG_PROFILE_MAX_T; ++t) s_cnt[wave][t] = cnt[t];
    s_max[wave] = mx;
  }
  __syncthreads();
  const size_t slot = (size_t)b * 2 + dir;
  if (tid < (unsigned)T) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kProfileWaves; ++w) c += s_cnt[w][tid];
    counts[slot * (size_t)T + tid] = c;
  }
  if (tid == 0) {
    float m = s_max[0];
#pragma unroll
    for (int w = 1; w < kProfileWaves; ++w) m = s_max[w] > m ? s_max[w] : m;
    maxima[slot] = m;
  }
}

}  // namespace
}  // namespace fpsg

extern "C" int fpsg_dist_profile(const float* dist1, const float* dist2, int B, int N, int M, const float* tau2, int T,
                                 int32_t* counts, float* maxima, fpsg_stream_t stream) {
  using namespace fpsg;
  FPSG_REQUIRE(B > 0 && N > 0 && M > 0, FPSG_E_SHAPE, "fpsg_dist_profile: B,N,M must be positive (got %d,%d,%d)", B, N,
               M);
  FPSG_REQUIRE(T >= 1, FPSG_E_SHAPE, "fpsg_dist_profile: T must be at least 1 (got %d)", T);
  FPSG_REQUIRE(T <= FPSG_PROFILE_MAX_T, FPSG_E_LIMIT, "fpsg_dist_profile: T=%d exceeds the supported maximum of %d", T,
               FPSG_PROFILE_MAX_T);
  // every null pointer before any misaligned one
  FPSG_REQUIRE(dist1 && dist2 && tau2 && counts && maxima, FPSG_E_NULL, "fpsg_dist_profile: null pointer '%s'",
               !dist1 ? "dist1" : !dist2 ? "dist2" : !tau2 ? "tau2" : !counts ? "counts" : "maxima");
  FPSG_REQUIRE_PTR(dist1); FPSG_REQUIRE_PTR(dist2); FPSG_REQUIRE_PTR(tau2);
  FPSG_REQUIRE_PTR(counts); FPSG_REQUIRE_PTR(maxima);
  hipLaunchKernelGGL(dist_profile_kernel, dim3((unsigned)B, 2u), dim3(kProfileThreads), 0,
                     static_cast<hipStream_t>(stream), dist1, dist2, N, M, tau2, T, counts, maxima);
  return launch_status("fpsg_dist_profile");
}
