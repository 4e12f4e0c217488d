// swd.hip -- K22: the sliced Wasserstein distance of two clouds of equal size under L given directions, with its exact
// gradient and, on request, the two matchings, for gfx950.  The definition is in include/fpsg_hip.h (K22) and DESIGN.md.
//
// Structure:
//   * main kernel: grid (G, B).  A workgroup owns ONE pair and the directions [g L / G, (g + 1) L / G) of it.  It keeps
//     both clouds in LDS (x, y, z interleaved: stride 3 floats, conflict-free) and per direction
//       1. forms the fp32 key of every point and stores (monotone image of the key) << 32 | index as one 64-bit word per
//          slot, for both clouds; slots N .. P - 1 (P the power of two >= N, a template parameter) get sentinels
//          0xFFFFFFFF << 32 | slot, which are above every real word -- a NaN's image 0xFFFFFFFF included, because a real
//          index is below N -- and distinct, so the order is total and ranks 0 .. N - 1 hold exactly the real points;
//       2. sorts both arrays with one bitonic network (P / 2 compare-exchanges per array and stage, one per thread and
//          array where P >= 128; a barrier after every stage).  Every trip count comes from P: no input can change one;
//       3. walks the ranks: the thread of rank r < N unpacks (key, index) of both clouds, adds d_r^2 to its own running
//          sum and d_r theta to the LDS accumulator rows pi1[r] / pi2[r].  pi is a permutation and r < N never meets a
//          sentinel, so no two threads touch one row in a direction; a barrier separates directions.
//     At the end the workgroup writes its partial value (threads' sums by the wave tree, waves in ascending order) and
//     its partial gradient rows to the workspace.
//   * finalize kernel: adds a pair's G partials in ascending g from +0 and scales: 1 / (L N) for the value, 2 / (L N)
//     for the gradients (both rounded to fp32 on the host).
// No atomics; nothing between workgroups inside a launch; every output has one writer and one fixed order.
#include "fpsg_common.h"

namespace fpsg {
namespace {

constexpr int kSwdGroupDirs = 8;                                  // directions per workgroup while G is below its cap
constexpr int kSwdMaxGroups = 16;

inline int swd_groups(int L) {
  const int g = (L + kSwdGroupDirs - 1) / kSwdGroupDirs;
  return g < kSwdMaxGroups ? g : kSwdMaxGroups;
}

constexpr int swd_threads(int P) { return P / 2 < kWave ? kWave : P / 2; }

// The monotone 32-bit image of an fp32 value: unsigned order of the images = numeric order of the values (-0 is
// excluded by the key's "+ 0.0f"); NaNs land above +inf (sign clear) or below -inf (sign set).
__device__ __forceinline__ uint32_t swd_image(float k) {
  const uint32_t u = __float_as_uint(k);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float swd_unimage(uint32_t m) {
  return __uint_as_float(m ^ ((m >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// fl(fl(fl(x tx) + fl(y ty)) + fl(z tz)) + 0.0f: the library is built with -ffp-contract=off, so nothing fuses
__device__ __forceinline__ float swd_key(const float* p, float tx, float ty, float tz) {
  return ((p[0] * tx + p[1] * ty) + p[2] * tz) + 0.0f;
}

__device__ __forceinline__ void swd_exchange(uint64_t* s, int i, int j, bool up) {
  const uint64_t a = s[i], b = s[j];
  if ((a > b) == up) {
    s[i] = b;
    s[j] = a;
  }
}

template <int P>
__global__ __launch_bounds__(swd_threads(P)) void swd_kernel(const float* __restrict__ xyz1,
                                                             const float* __restrict__ xyz2,
                                                             const float* __restrict__ dirs, int N, int L,
                                                             float* __restrict__ pval, float* __restrict__ pg1,
                                                             float* __restrict__ pg2, int32_t* __restrict__ perm1,
                                                             int32_t* __restrict__ perm2) {
  constexpr int T = swd_threads(P);
  constexpr int kWaves = T / kWave;
  __shared__ __attribute__((aligned(16))) uint64_t s1[P];
  __shared__ __attribute__((aligned(16))) uint64_t s2[P];
  __shared__ float p1[3 * P];
  __shared__ float p2[3 * P];
  __shared__ float a1[3 * P];
  __shared__ float a2[3 * P];
  __shared__ float wsum[kWaves];
  const int tid = (int)threadIdx.x;
  const int g = (int)blockIdx.x, G = (int)gridDim.x;
  const size_t b = blockIdx.y;
  const bool want1 = pg1 != nullptr, want2 = pg2 != nullptr;

  const float* __restrict__ x1 = xyz1 + b * (size_t)N * 3;
  const float* __restrict__ x2 = xyz2 + b * (size_t)N * 3;
  for (int e = tid; e < 3 * N; e += T) {
    p1[e] = x1[e];
    p2[e] = x2[e];
    a1[e] = 0.f;
    a2[e] = 0.f;
  }
  __syncthreads();

  const int l0 = (int)(((long)g * L) / G), l1 = (int)(((long)(g + 1) * L) / G);
  float vsum = 0.f;
  for (int l = l0; l < l1; ++l) {
    const float tx = dirs[3 * l + 0], ty = dirs[3 * l + 1], tz = dirs[3 * l + 2];
    for (int s = tid; s < P; s += T) {
      uint64_t w1 = 0xFFFFFFFF00000000ull | (uint32_t)s, w2 = w1;    // the sentinel of slot s >= N
      if (s < N) {
        w1 = ((uint64_t)swd_image(swd_key(p1 + 3 * s, tx, ty, tz)) << 32) | (uint32_t)s;
        w2 = ((uint64_t)swd_image(swd_key(p2 + 3 * s, tx, ty, tz)) << 32) | (uint32_t)s;
      }
      s1[s] = w1;
      s2[s] = w2;
    }
    __syncthreads();
#pragma unroll 1
    for (int k = 2; k <= P; k <<= 1) {
#pragma unroll 1
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < P / 2; t += T) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // t with a zero bit inserted at j's position
          const bool up = (i & k) == 0;
          swd_exchange(s1, i, i | j, up);
          swd_exchange(s2, i, i | j, up);
        }
        __syncthreads();
      }
    }
    for (int r = tid; r < N; r += T) {                           // r < N: real points only, indices below N
      const uint64_t w1 = s1[r], w2 = s2[r];
      const int i1 = (int)(uint32_t)w1, i2 = (int)(uint32_t)w2;
      const float d = swd_unimage((uint32_t)(w1 >> 32)) - swd_unimage((uint32_t)(w2 >> 32));
      vsum += d * d;
      if (want1 && (unsigned)i1 < (unsigned)N) {
        a1[3 * i1 + 0] += d * tx;
        a1[3 * i1 + 1] += d * ty;
        a1[3 * i1 + 2] += d * tz;
      }
      if (want2 && (unsigned)i2 < (unsigned)N) {
        a2[3 * i2 + 0] -= d * tx;
        a2[3 * i2 + 1] -= d * ty;
        a2[3 * i2 + 2] -= d * tz;
      }
      if (perm1 != nullptr) perm1[(b * (size_t)L + (size_t)l) * (size_t)N + (size_t)r] = i1;
      if (perm2 != nullptr) perm2[(b * (size_t)L + (size_t)l) * (size_t)N + (size_t)r] = i2;
    }
    __syncthreads();                                              // the next direction overwrites the sort arrays
  }

  vsum = wave_sum(vsum);
  if ((tid & (kWave - 1)) == 0) wsum[tid / kWave] = vsum;
  __syncthreads();
  if (tid == 0) {
    float s = wsum[0];
    for (int w = 1; w < kWaves; ++w) s += wsum[w];
    pval[b * (size_t)G + (size_t)g] = s;
  }
  const size_t row = (b * (size_t)G + (size_t)g) * (size_t)N * 3;
  for (int e = tid; e < 3 * N; e += T) {
    if (want1) pg1[row + e] = a1[e];
    if (want2) pg2[row + e] = a2[e];
  }
}

// value[b] and the gradient elements of pair b: the G partials in ascending g from +0, then the scale
__global__ void swd_finalize_kernel(const float* __restrict__ pval, const float* __restrict__ pg1,
                                    const float* __restrict__ pg2, int N, int G, float vscale, float gscale,
                                    float* __restrict__ value, float* __restrict__ g1, float* __restrict__ g2) {
  const size_t b = blockIdx.y;
  const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e == 0) {
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += pval[b * (size_t)G + (size_t)g];
    value[b] = s * vscale;
  }
  if (e >= 3 * N) return;
  const size_t stride = (size_t)N * 3, first = b * (size_t)G * stride + (size_t)e;
  if (g1 != nullptr) {
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += pg1[first + (size_t)g * stride];
    g1[b * stride + (size_t)e] = s * gscale;
  }
  if (g2 != nullptr) {
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += pg2[first + (size_t)g * stride];
    g2[b * stride + (size_t)e] = s * gscale;
  }
}

inline bool swd_shape_served(int B, int N, int L) {
  return B >= 1 && N >= 1 && L >= 1 && B <= FPSG_SWD_MAX_B && N <= FPSG_SWD_MAX_N && L <= FPSG_SWD_MAX_L;
}

}  // namespace
}  // namespace fpsg

// Layout: partial values [B,G] | partial gradients of cloud 1 [B,G,N,3] | of cloud 2 [B,G,N,3], all fp32.
extern "C" size_t fpsg_swd_workspace_bytes(int B, int N, int L) {
  using namespace fpsg;
  if (!swd_shape_served(B, N, L)) return 0;
  return (size_t)B * (size_t)swd_groups(L) * ((size_t)1 + (size_t)6 * (size_t)N) * sizeof(float);
}

extern "C" int fpsg_swd(const float* xyz1, const float* xyz2, const float* dirs, int B, int N, int L, float* value,
                        float* gxyz1, float* gxyz2, int32_t* perm1, int32_t* perm2, void* ws, size_t ws_bytes,
                        fpsg_stream_t stream) {
  using namespace fpsg;
  FPSG_REQUIRE(B > 0, FPSG_E_SHAPE, "fpsg_swd: B must be positive (got %d)", B);
  FPSG_REQUIRE(N > 0, FPSG_E_SHAPE, "fpsg_swd: N must be positive (got %d)", N);
  FPSG_REQUIRE(L > 0, FPSG_E_SHAPE, "fpsg_swd: L must be positive (got %d)", L);
  FPSG_REQUIRE(N <= FPSG_SWD_MAX_N, FPSG_E_LIMIT, "fpsg_swd: N=%d exceeds the supported maximum of %d points", N,
               FPSG_SWD_MAX_N);
  FPSG_REQUIRE(L <= FPSG_SWD_MAX_L, FPSG_E_LIMIT, "fpsg_swd: L=%d exceeds the supported maximum of %d directions", L,
               FPSG_SWD_MAX_L);
  FPSG_REQUIRE(B <= FPSG_SWD_MAX_B, FPSG_E_LIMIT, "fpsg_swd: B=%d exceeds the supported maximum of %d pairs", B,
               FPSG_SWD_MAX_B);
  FPSG_REQUIRE_PTR(xyz1); FPSG_REQUIRE_PTR(xyz2); FPSG_REQUIRE_PTR(dirs); FPSG_REQUIRE_PTR(value); FPSG_REQUIRE_PTR(ws);
  FPSG_REQUIRE(!misaligned4(gxyz1) && !misaligned4(gxyz2) && !misaligned4(perm1) && !misaligned4(perm2), FPSG_E_ALIGN,
               "fpsg_swd: an optional output is not 4-byte aligned");
  FPSG_REQUIRE(ws_bytes >= fpsg_swd_workspace_bytes(B, N, L), FPSG_E_SHAPE,
               "fpsg_swd: workspace of %zu bytes, %zu needed", ws_bytes, fpsg_swd_workspace_bytes(B, N, L));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int G = swd_groups(L);
  float* pval = static_cast<float*>(ws);
  float* pg1 = pval + (size_t)B * (size_t)G;
  float* pg2 = pg1 + (size_t)B * (size_t)G * (size_t)N * 3;
  if (gxyz1 == nullptr) pg1 = nullptr;
  if (gxyz2 == nullptr) pg2 = nullptr;
  const dim3 grid((unsigned)G, (unsigned)B);
#define FPSG_SWD_LAUNCH(P)                                                                                          \
  hipLaunchKernelGGL(swd_kernel<P>, grid, dim3(swd_threads(P)), 0, s, xyz1, xyz2, dirs, N, L, pval, pg1, pg2, perm1, \
                     perm2)
  if (N <= 64) FPSG_SWD_LAUNCH(64);
  else if (N <= 128) FPSG_SWD_LAUNCH(128);
  else if (N <= 256) FPSG_SWD_LAUNCH(256);
  else if (N <= 512) FPSG_SWD_LAUNCH(512);
  else if (N <= 1024) FPSG_SWD_LAUNCH(1024);
  else FPSG_SWD_LAUNCH(2048);
#undef FPSG_SWD_LAUNCH
  static_assert(FPSG_SWD_MAX_N == 2048, "the largest instantiation of swd_kernel serves FPSG_SWD_MAX_N");
  if (const int rc = launch_status("fpsg_swd")) return rc;
  const float vscale = (float)(1.0 / ((double)L * (double)N));
  const float gscale = (float)(2.0 / ((double)L * (double)N));
  hipLaunchKernelGGL(swd_finalize_kernel, dim3((unsigned)((3 * N + 255) / 256), (unsigned)B), dim3(256), 0, s, pval, pg1,
                     pg2, N, G, vscale, gscale, value, gxyz1, gxyz2);
  return launch_status("fpsg_swd");
}
