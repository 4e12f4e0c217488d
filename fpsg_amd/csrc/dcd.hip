// dcd.hip -- K18: the density-aware Chamfer distance of cloud pairs from K1's rows, for gfx950.  The definition is
// in include/fpsg_hip.h (K18) and DESIGN.md: every point's term exp(-alpha d) is divided by the number of queries that
// chose the same nearest neighbour, so a reconstruction that piles its points onto a few targets is charged for it.
//
// Structure:
//   * one workgroup of 1024 threads per pair, grid (B); it runs the two sides one after the other through ONE device
//     routine (dcd_side), so dcd(p1, p2) and dcd(p2, p1) are the same arithmetic on swapped arguments, and thread 0
//     forms 0.5 * (side1 + side2): one launch, no workspace, nothing between workgroups, no tickets;
//   * a side: (1) zero an int32 histogram of the target cloud in LDS (<= 16384 counters = 64 KB); (2) one LDS integer
//     atomic per source point over the argmin list -- a wave whose 64 lanes all name one target (the collapse case)
//     sends ONE add of 64 instead of 64 adds that the LDS would take one after the other; (3) the histogram goes out
//     as the in-degree row, and wave w takes the blocks w, w + 16, ... of 256 source points: four loads in flight,
//     the count gathered from LDS, v_exp_f32, the two outputs per point, K1l's block sum in registers; (4) the block
//     sums pass through the (now dead) histogram and thread 0 adds them in ascending order;
//   * integer atomics and a fixed-order float sum: bitwise the same on every run, whatever B is.  Every trip count
//     comes from N and M; an index outside its range is counted nowhere and touches no memory.
#include "fpsg_common.h"

namespace fpsg {
namespace {

constexpr int kDcdThreads = 1024;
constexpr int kDcdWaves = kDcdThreads / kWave;
constexpr int kDcdBlock = 256;                                   // K1l's block of the row sum
constexpr int kDcdBlocksPerWave = FPSG_DCD_MAX_N / kDcdBlock / kDcdWaves;
static_assert(kDcdBlocksPerWave * kDcdWaves * kDcdBlock == FPSG_DCD_MAX_N, "a wave owns a whole number of blocks");

// One side of one pair: n source points with squared distance dist[i] to, and index idx[i] of, their nearest of the m
// target points.  Writes deg[0..m) and (w != null) w[0..n); returns the side's value in thread 0 (other threads: 0).
// `hist` is the workgroup's FPSG_DCD_MAX_N-dword LDS array; the routine begins and ends with every thread past its
// last access to it.
__device__ __forceinline__ float dcd_side(const float* __restrict__ dist, const int32_t* __restrict__ idx, int n, int m,
                                          float alpha, int32_t* __restrict__ deg, float* __restrict__ w, int* hist) {
  const int tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  for (int j = tid; j < m; j += kDcdThreads) hist[j] = 0;
  __syncthreads();

  for (int i0 = wave * kWave; i0 < n; i0 += kDcdThreads) {        // i0: wave-uniform
    const int i = i0 + lane;
    const int j = i < n ? idx[i] : -1;
    const bool ok = (unsigned)j < (unsigned)m;
    const int first = __builtin_amdgcn_readfirstlane(j);
    const unsigned long long all = __ballot(true), same = __ballot(ok && j == first);
    if (same == all) {                                            // every lane is live, in range and names `first`
      if (lane == 0) atomicAdd(&hist[first], kWave);
    } else if (ok) {
      atomicAdd(&hist[j], 1);
    }
  }
  __syncthreads();

  for (int j = tid; j < m; j += kDcdThreads) deg[j] = hist[j];

  // exp(-x) = 2^(-(x log2 e)): v_exp_f32 itself (base 2) -- with -fno-fast-math __expf expands to a range / denormal
  // scaffold around the same instruction (emd.hip); a result below 2^-126 is flushed to +0, far inside the error budget
  constexpr float kLog2e = 1.44269504088896340736f;
  const float rn = 1.0f / (float)n;
  const float wscale = 0.5f * rn;
  const int nblk = (n + kDcdBlock - 1) / kDcdBlock;
  float bsum[kDcdBlocksPerWave];
#pragma unroll
  for (int k = 0; k < kDcdBlocksPerWave; ++k) {
    bsum[k] = 0.f;
    const int blk = wave + k * kDcdWaves;
    if (blk < nblk) {
      float d[4];
      int j[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = blk * kDcdBlock + g * kWave + lane;
        d[g] = i < n ? dist[i] : 0.f;
        j[g] = i < n ? idx[i] : -1;
      }
      float t[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = blk * kDcdBlock + g * kWave + lane;
        const bool ok = (unsigned)j[g] < (unsigned)m;
        const int c = ok ? hist[j[g]] : 1;                        // >= 1 where ok: point i itself was counted
        const float e = __builtin_amdgcn_exp2f(-((alpha * d[g]) * kLog2e));
        const float q = ok ? e / (float)c : 0.f;
        if (w && i < n) w[i] = (alpha * q) * wscale;
        t[g] = i < n ? 1.0f - q : 0.f;
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) t[g] = wave_sum(t[g]);
      bsum[k] = ((t[0] + t[1]) + t[2]) + t[3];
    }
  }
  __syncthreads();                                                // the last gather is done: the histogram is free

  if (lane == 0) {                                                // (as bit patterns: the array stays one of int)
#pragma unroll
    for (int k = 0; k < kDcdBlocksPerWave; ++k) {
      const int blk = wave + k * kDcdWaves;
      if (blk < nblk) hist[blk] = __float_as_int(bsum[k]);
    }
  }
  __syncthreads();
  float s = 0.f;
  if (tid == 0) {
    for (int blk = 0; blk < nblk; ++blk) s += __int_as_float(hist[blk]);
    s *= rn;
  }
  __syncthreads();                                                // the next side zeroes the array
  return s;
}

__global__ __launch_bounds__(kDcdThreads) void dcd_kernel(const float* __restrict__ dist1, const int32_t* __restrict__ idx1,
                                                          const float* __restrict__ dist2, const int32_t* __restrict__ idx2,
                                                          int N, int M, float alpha, float* __restrict__ out,
                                                          float* __restrict__ sides, int32_t* __restrict__ deg1,
                                                          int32_t* __restrict__ deg2, float* __restrict__ w1,
                                                          float* __restrict__ w2) {
  __shared__ int hist[FPSG_DCD_MAX_N];
  const size_t b = blockIdx.x;
  const float s1 = dcd_side(dist1 + b * N, idx1 + b * N, N, M, alpha, deg2 + b * M, w1 ? w1 + b * N : nullptr, hist);
  const float s2 = dcd_side(dist2 + b * M, idx2 + b * M, M, N, alpha, deg1 + b * N, w2 ? w2 + b * M : nullptr, hist);
  if (threadIdx.x == 0) {
    sides[2 * b + 0] = s1;
    sides[2 * b + 1] = s2;
    out[b] = 0.5f * (s1 + s2);
  }
}

}  // namespace
}  // namespace fpsg

extern "C" int fpsg_dcd(const float* dist1, const int32_t* idx1, const float* dist2, const int32_t* idx2, int B, int N,
                        int M, float alpha, float* out, float* sides, int32_t* deg1, int32_t* deg2, float* w1, float* w2,
                        fpsg_stream_t stream) {
  using namespace fpsg;
  // every null pointer before anything else (w1 and w2 may be null: no gradient weights wanted)
  FPSG_REQUIRE(dist1 && idx1 && dist2 && idx2 && out && sides && deg1 && deg2, FPSG_E_NULL,
               "fpsg_dcd: null pointer '%s'",
               !dist1 ? "dist1" : !idx1 ? "idx1" : !dist2 ? "dist2" : !idx2 ? "idx2" : !out ? "out"
               : !sides ? "sides" : !deg1 ? "deg1" : "deg2");
  FPSG_REQUIRE(B > 0 && N > 0 && M > 0, FPSG_E_SHAPE, "fpsg_dcd: B,N,M must be positive (got %d,%d,%d)", B, N, M);
  FPSG_REQUIRE(N <= FPSG_DCD_MAX_N && M <= FPSG_DCD_MAX_N, FPSG_E_LIMIT,
               "fpsg_dcd: N=%d, M=%d exceed the supported maximum of %d points", N, M, FPSG_DCD_MAX_N);
  FPSG_REQUIRE_PTR(dist1); FPSG_REQUIRE_PTR(idx1); FPSG_REQUIRE_PTR(dist2); FPSG_REQUIRE_PTR(idx2);
  FPSG_REQUIRE_PTR(out); FPSG_REQUIRE_PTR(sides); FPSG_REQUIRE_PTR(deg1); FPSG_REQUIRE_PTR(deg2);
  FPSG_REQUIRE(!(w1 && misaligned4(w1)) && !(w2 && misaligned4(w2)), FPSG_E_ALIGN,
               "fpsg_dcd: '%s' not 4-byte aligned", w1 && misaligned4(w1) ? "w1" : "w2");
  hipLaunchKernelGGL(dcd_kernel, dim3((unsigned)B), dim3(kDcdThreads), 0, static_cast<hipStream_t>(stream), dist1, idx1,
                     dist2, idx2, N, M, alpha, out, sides, deg1, deg2, w1, w2);
  return launch_status("fpsg_dcd");
}
