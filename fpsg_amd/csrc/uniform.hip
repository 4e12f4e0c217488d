// uniform.hip -- K25: PU-GAN's uniform loss of a cloud (balls of several sizes around seed points, each charged for the
// imbalance of its point count and for the clutter of its members' nearest-neighbour distances), forward and backward,
// for gfx950.  The two building blocks are a ball query and a nearest-neighbour search inside a group.  The definition
// is in include/fpsg_hip.h (K25) and DESIGN.md.
//
// Structure:
//   * forward: ONE wavefront owns one (cloud, seed); four of them share a workgroup, each with its own LDS slice, and
//     nothing passes between them (the barriers only order a wave's own LDS writes and reads; every wave reaches every
//     one of them, because every trip count comes from N, T and the cap).  The wave sweeps the cloud 64 points at a
//     time against the seed: ONE distance per point, then per percentage a ballot of d2 <= r2_t -- its popcount goes to
//     the ball's count, the lane's rank in the mask is its slot in that ball's ascending member list in LDS, up to the
//     cap.  Then, per percentage, the retained members' coordinates are gathered into LDS and registers (member
//     lane + 64 s belongs to lane `lane`, slot s; V = cap / 64 slots, a template parameter), every member takes its
//     nearest other member from broadcast ds_read_b128 reads, four candidates a read, in ascending list order with a
//     strict compare (ties: the lowest slot, which is the lowest index), and the terms are reduced by the fixed tree.
//     Slots past the ball's end hold NaN coordinates: every compare with a NaN distance is false.
//   * two tiny launches close the forward: one wave per (cloud, percentage) adds that row's S ball values, one thread
//     per cloud adds the T row sums.
//   * backward: GATHER form, one thread per point, 256 a workgroup.  The balls' parameters (seed coordinates, r2, dhat,
//     the ball's factor, the retained count) are formed once per workgroup and tile of 256 balls and staged through
//     LDS; the thread walks the balls in ascending (t, j), repeats the forward's compare on the same bits, and only
//     inside a ball looks for its slot in the ascending list (a binary search), takes its own term and then the terms
//     of the members whose nn it is, in list order.  One writer per output, one fixed order, no float atomics.  (A
//     build that also staged the lists through LDS, in tiles of 2048 / cap balls, was slower: DESIGN.md K25.)
//   * no index is dereferenced unchecked: a seed outside [0, N) owns an empty ball, counts are clamped to the cap,
//     member and nn entries outside [0, N) are skipped.
#include <cmath>

#include "chamfer_dist.h"

namespace fpsg {
namespace {

constexpr int kUniWaves = 4;                                      // (cloud, seed) pairs per forward workgroup
constexpr int kUniThreads = kUniWaves * kWave;
constexpr int kUniBwdThreads = 256;
constexpr int kUniMaxT = FPSG_UNIFORM_MAX_T;

// per percentage, formed in double on the host and rounded once (fpsg_hip.h K25)
struct UniParams {
  float r2[kUniMaxT];                                             // p_t R^2
  float area[kUniMaxT];                                           // (2 pi / sqrt 3) r2_t
  float nhat[kUniMaxT];                                           // N p_t
};

// the expected spacing of a ball with full count c >= 1; the forward and the backward share the expression
__device__ __forceinline__ float uni_dhat(float area, int c) { return sqrtf(area / (float)c); }

// (c - nhat)^2 / nhat
__device__ __forceinline__ float uni_weight(float nhat, int c) {
  const float dc = (float)c - nhat;
  return (dc * dc) / nhat;
}

template <int V>
__global__ __launch_bounds__(kUniThreads) void uniform_fwd_kernel(
    const float* __restrict__ xyz, const int32_t* __restrict__ seeds, int N, int S, int T, int total, UniParams prm,
    int32_t* __restrict__ count, int32_t* __restrict__ member, int32_t* __restrict__ nn, float* __restrict__ nn_d2,
    float* __restrict__ ball_value) {
  constexpr int C = V * kWave;                                    // the cap
  __shared__ int list[kUniWaves][kUniMaxT][C];                    // the balls' retained members, ascending
  __shared__ __attribute__((aligned(16))) float cx[kUniWaves][C];
  __shared__ __attribute__((aligned(16))) float cy[kUniWaves][C];
  __shared__ __attribute__((aligned(16))) float cz[kUniWaves][C];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int g = (int)blockIdx.x * kUniWaves + wave;               // cloud g / S, seed g % S
  const bool live = g < total;
  const int b = (live ? g : 0) / S, j = (live ? g : 0) % S;
  const float* __restrict__ x = xyz + (size_t)b * (size_t)N * 3;
  const int seed = seeds[(size_t)b * S + j];
  const bool valid = live & ((unsigned)seed < (unsigned)N);       // a seed outside the cloud owns an empty ball
  const int sd = valid ? seed : 0;
  const float qx = x[3 * (size_t)sd + 0], qy = x[3 * (size_t)sd + 1], qz = x[3 * (size_t)sd + 2];
  const unsigned long long below = (1ull << lane) - 1ull;

  int cnt[kUniMaxT];
#pragma unroll
  for (int t = 0; t < kUniMaxT; ++t) cnt[t] = 0;

  for (int i0 = 0; i0 < N; i0 += kWave) {                         // the ball query: N / 64 trips
    const int i = i0 + lane;
    const bool in = valid & (i < N);
    const size_t ii = in ? (size_t)i : 0;
    const float d2 = sq_dist(qx, qy, qz, x[3 * ii + 0], x[3 * ii + 1], x[3 * ii + 2]);
#pragma unroll
    for (int t = 0; t < kUniMaxT; ++t) {
      if (t < T) {
        const bool hit = in & (d2 <= prm.r2[t]);                  // fp32 <=: on the sphere is inside, a NaN is outside
        const unsigned long long m = __ballot(hit);
        const int slot = cnt[t] + (int)__builtin_popcountll(m & below);
        if (hit & (slot < C)) list[wave][t][slot] = i;
        cnt[t] += (int)__builtin_popcountll(m);
      }
    }
  }
  __syncthreads();                                                // the lists are written

#pragma unroll
  for (int t = 0; t < kUniMaxT; ++t) {
    if (t < T) {                                                  // uniform over the workgroup
      const int c = cnt[t];
      const int m = c < C ? c : C;
      const size_t ball = ((size_t)b * T + t) * (size_t)S + j;

      float px[V], py[V], pz[V], best[V];
      int bq[V];
#pragma unroll
      for (int s = 0; s < V; ++s) {
        const int q = lane + s * kWave;
        const int i = q < m ? list[wave][t][q] : -1;
        const bool ok = i >= 0;
        px[s] = ok ? x[3 * (size_t)(ok ? i : 0) + 0] : NAN;
        py[s] = ok ? x[3 * (size_t)(ok ? i : 0) + 1] : NAN;
        pz[s] = ok ? x[3 * (size_t)(ok ? i : 0) + 2] : NAN;
        cx[wave][q] = px[s];
        cy[wave][q] = py[s];
        cz[wave][q] = pz[s];
        best[s] = INFINITY;
        bq[s] = -1;
        if (live) member[ball * C + q] = i;
      }
      __syncthreads();

      for (int q0 = 0; q0 < C; q0 += 4) {                         // nearest other member: cap / 4 trips
        const v4f X = *reinterpret_cast<const v4f*>(&cx[wave][q0]);
        const v4f Y = *reinterpret_cast<const v4f*>(&cy[wave][q0]);
        const v4f Z = *reinterpret_cast<const v4f*>(&cz[wave][q0]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int s = 0; s < V; ++s) {
            const float d = sq_dist(px[s], py[s], pz[s], X[u], Y[u], Z[u]);
            const bool lower = (d < best[s]) & ((q0 + u) != (lane + s * kWave));   // strictly: the lowest slot wins
            best[s] = lower ? d : best[s];
            bq[s] = lower ? q0 + u : bq[s];
          }
        }
      }

      // c >= 1 wherever a term is used (m >= 2); the guard keeps the division defined elsewhere
      const float dhat = uni_dhat(prm.area[t], c > 0 ? c : 1);
      float ls = 0.f;
#pragma unroll
      for (int s = 0; s < V; ++s) {
        const int q = lane + s * kWave;
        const bool has = bq[s] >= 0;
        const int other = has ? list[wave][t][bq[s]] : -1;
        float term = 0.f;
        if (q < m) {
          const float dev = sqrtf(best[s]) - dhat;
          term = best[s] == 0.f ? dhat : (dev * dev) / dhat;      // a duplicate contributes dhat
        }
        ls += term;
        if (live) {
          nn[ball * C + q] = (q < m) ? other : -1;
          nn_d2[ball * C + q] = (q < m) ? best[s] : INFINITY;
        }
      }
      const float tot = wave_sum(ls);
      if (live & (lane == 0)) {
        count[ball] = c;
        ball_value[ball] = m >= 2 ? uni_weight(prm.nhat[t], c) * tot : 0.f;
      }
      __syncthreads();                                            // the slice is read before the next ball overwrites it
    }
  }
}

// rows[b, t] = the S ball values of (b, t): lane l adds j = l, l + 64, ... in ascending order from +0, the lanes by the
// balanced tree; per_percent[b, t] = rows / S.  One wave per (b, t).
__global__ __launch_bounds__(kWave) void uniform_rows_kernel(const float* __restrict__ ball_value, int S,
                                                             float* __restrict__ rows,
                                                             float* __restrict__ per_percent) {
  const size_t row = blockIdx.x;
  const float* __restrict__ v = ball_value + row * (size_t)S;
  float s = 0.f;
  for (int j = (int)threadIdx.x; j < S; j += kWave) s += v[j];
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    rows[row] = s;
    per_percent[row] = s / (float)S;
  }
}

// value[b] = (the T row sums of cloud b added in ascending order from +0) / (T S); one thread per cloud
__global__ void uniform_finalize_kernel(const float* __restrict__ rows, int B, int T, int S, float* __restrict__ value) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= B) return;
  float s = 0.f;
  for (int t = 0; t < T; ++t) s += rows[(size_t)b * T + t];
  value[b] = s / ((float)T * (float)S);
}

// The slot of point i in the ascending list l[0 .. m), -1 where it is not there.  At most nine probes for m <= 256; on
// a list that is not ascending the answer is unspecified but inside [-1, m).
__device__ __forceinline__ int uni_find(const int32_t* __restrict__ l, int m, int i) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (l[mid] < i) lo = mid + 1;
    else hi = mid;
  }
  return (lo < m && l[lo] == i) ? lo : -1;
}

__global__ __launch_bounds__(kUniBwdThreads) void uniform_bwd_kernel(
    const float* __restrict__ xyz, const int32_t* __restrict__ seeds, const int32_t* __restrict__ count,
    const int32_t* __restrict__ member, const int32_t* __restrict__ nn, const float* __restrict__ nn_d2,
    const float* __restrict__ gvalue, int N, int S, int T, int C, UniParams prm, float scale,
    float* __restrict__ gxyz) {
  __shared__ __attribute__((aligned(16))) v4f sball[kUniBwdThreads];   // seed x, y, z and r2 (-1: the ball is skipped)
  __shared__ float sdhat[kUniBwdThreads];
  __shared__ float scoef[kUniBwdThreads];                         // 2 w / dhat
  __shared__ int sm[kUniBwdThreads];                              // retained members
  const size_t b = blockIdx.y;
  const float* __restrict__ x = xyz + b * (size_t)N * 3;
  const int i = (int)blockIdx.x * kUniBwdThreads + (int)threadIdx.x;
  const bool live = i < N;
  const size_t ii = live ? (size_t)i : 0;
  const float qx = x[3 * ii + 0], qy = x[3 * ii + 1], qz = x[3 * ii + 2];
  const int balls = T * S;

  float ax = 0.f, ay = 0.f, az = 0.f;
  for (int k0 = 0; k0 < balls; k0 += kUniBwdThreads) {            // the same trip count for every thread
    __syncthreads();                                              // the previous tile has been read
    {
      const int k = k0 + (int)threadIdx.x;                        // ball (t, j) = (k / S, k % S): ascending (t, j)
      v4f rec = {0.f, 0.f, 0.f, -1.f};
      float dh = 1.f, cf = 0.f;
      int m = 0;
      if (k < balls) {
        const int t = k / S, j = k - t * S;
        const int seed = seeds[b * (size_t)S + j];
        const int c = count[(b * (size_t)T + t) * (size_t)S + j];
        m = c < C ? c : C;
        if (((unsigned)seed < (unsigned)N) & (m >= 2)) {
          dh = uni_dhat(prm.area[t], c);
          cf = (2.f * uni_weight(prm.nhat[t], c)) / dh;
          rec = v4f{x[3 * (size_t)seed + 0], x[3 * (size_t)seed + 1], x[3 * (size_t)seed + 2], prm.r2[t]};
        }
      }
      sball[threadIdx.x] = rec;
      sdhat[threadIdx.x] = dh;
      scoef[threadIdx.x] = cf;
      sm[threadIdx.x] = m;
    }
    __syncthreads();
    const int tile = min(kUniBwdThreads, balls - k0);
    for (int u = 0; u < tile; ++u) {
      const v4f rec = sball[u];                                   // a broadcast read
      const float d2 = sq_dist(rec.x, rec.y, rec.z, qx, qy, qz);  // the forward's expression on the same bits
      if (live & (d2 <= rec.w)) {                                 // r2 = -1 holds nobody
        const size_t base = (b * (size_t)balls + (size_t)(k0 + u)) * (size_t)C;
        const int32_t* __restrict__ l = member + base;
        const int m = sm[u];
        const int slot = uni_find(l, m, i);
        if (slot >= 0) {                                          // retained: beyond the cap a member has no term
          const float dh = sdhat[u], cf = scoef[u];
          {                                                       // the point's own term
            const int o = nn[base + slot];
            const float e = nn_d2[base + slot];
            if (((unsigned)o < (unsigned)N) & (e > 0.f)) {
              const float d = sqrtf(e);
              const float w = (cf * (d - dh)) / d;
              ax = fma_rn(w, qx - x[3 * (size_t)o + 0], ax);
              ay = fma_rn(w, qy - x[3 * (size_t)o + 1], ay);
              az = fma_rn(w, qz - x[3 * (size_t)o + 2], az);
            }
          }
          for (int q = 0; q < m; ++q) {                           // the members whose nearest neighbour is this point
            if (nn[base + q] != i) continue;
            const int o = l[q];
            const float e = nn_d2[base + q];
            if (((unsigned)o < (unsigned)N) & (e > 0.f)) {
              const float d = sqrtf(e);
              const float w = (cf * (d - dh)) / d;
              ax = fma_rn(w, qx - x[3 * (size_t)o + 0], ax);
              ay = fma_rn(w, qy - x[3 * (size_t)o + 1], ay);
              az = fma_rn(w, qz - x[3 * (size_t)o + 2], az);
            }
          }
        }
      }
    }
  }

  if (live) {
    const float gs = gvalue[b] * scale;
    float* __restrict__ o = gxyz + (b * (size_t)N + (size_t)i) * 3;
    o[0] = ax * gs;
    o[1] = ay * gs;
    o[2] = az * gs;
  }
}

inline bool uni_cap_ok(int cap) { return cap == 64 || cap == 128 || cap == 256; }

// The integer shape checks, the radius and the limits: everything that can be told without reading `percent`.
int uni_check_ints(const char* who, int B, int N, int S, int T, float radius, int cap) {
  FPSG_REQUIRE(B > 0, FPSG_E_SHAPE, "%s: B must be positive (got %d)", who, B);
  FPSG_REQUIRE(S > 0, FPSG_E_SHAPE, "%s: S must be positive (got %d)", who, S);
  FPSG_REQUIRE(T > 0, FPSG_E_SHAPE, "%s: T must be positive (got %d)", who, T);
  FPSG_REQUIRE(N >= 2, FPSG_E_SHAPE, "%s: N must be at least 2 (got %d)", who, N);
  FPSG_REQUIRE(S <= N, FPSG_E_SHAPE, "%s: S must not exceed N (got S=%d, N=%d)", who, S, N);
  FPSG_REQUIRE(std::isfinite(radius) && radius > 0.f, FPSG_E_SHAPE, "%s: radius must be positive and finite (got %g)",
               who, (double)radius);
  FPSG_REQUIRE(uni_cap_ok(cap), FPSG_E_SHAPE, "%s: cap must be 64, 128 or 256 (got %d)", who, cap);
  FPSG_REQUIRE(N <= FPSG_UNIFORM_MAX_N, FPSG_E_LIMIT, "%s: N=%d exceeds the supported maximum of %d points", who, N,
               FPSG_UNIFORM_MAX_N);
  FPSG_REQUIRE(T <= FPSG_UNIFORM_MAX_T, FPSG_E_LIMIT, "%s: T=%d exceeds the supported maximum of %d percentages", who, T,
               FPSG_UNIFORM_MAX_T);
  return 0;
}

// Reads the host array `percent` (T <= 8 entries) and forms the per-percentage parameters in double, rounded once.
int uni_params(const char* who, const float* percent, int N, int T, float radius, UniParams* prm) {
  if (percent == nullptr) {
    set_error("%s: null pointer 'percent'", who);
    return FPSG_E_NULL;
  }
  const double two_pi_over_sqrt3 = 2.0 * 3.14159265358979323846 / std::sqrt(3.0);
  for (int t = 0; t < kUniMaxT; ++t) prm->r2[t] = prm->area[t] = prm->nhat[t] = 0.f;
  for (int t = 0; t < T; ++t) {
    const float p = percent[t];
    FPSG_REQUIRE(std::isfinite(p) && p > 0.f && p <= 1.f, FPSG_E_SHAPE,
                 "%s: percent[%d] must be in (0, 1] (got %g)", who, t, (double)p);
    prm->r2[t] = (float)((double)p * (double)radius * (double)radius);
    prm->area[t] = (float)(two_pi_over_sqrt3 * (double)prm->r2[t]);
    prm->nhat[t] = (float)((double)N * (double)p);
  }
  return 0;
}

}  // namespace
}  // namespace fpsg

extern "C" size_t fpsg_uniform_workspace_bytes(int B, int N, int S, int T, int cap) {
  using namespace fpsg;
  if (B <= 0 || S <= 0 || T <= 0 || N < 2 || S > N || !uni_cap_ok(cap) || N > FPSG_UNIFORM_MAX_N ||
      T > FPSG_UNIFORM_MAX_T)
    return 0;
  return (size_t)B * (size_t)T * sizeof(float);                   // the row sums
}

extern "C" int fpsg_uniform_fwd(const float* xyz, const int32_t* seeds, int B, int N, int S, const float* percent, int T,
                                float radius, int cap, int32_t* count, int32_t* member, int32_t* nn, float* nn_d2,
                                float* ball_value, float* per_percent, float* value, void* workspace,
                                size_t workspace_bytes, fpsg_stream_t stream) {
  using namespace fpsg;
  if (const int rc = uni_check_ints("fpsg_uniform_fwd", B, N, S, T, radius, cap)) return rc;
  UniParams prm;
  if (const int rc = uni_params("fpsg_uniform_fwd", percent, N, T, radius, &prm)) return rc;
  FPSG_REQUIRE_PTR(xyz); FPSG_REQUIRE_PTR(seeds); FPSG_REQUIRE_PTR(count); FPSG_REQUIRE_PTR(member);
  FPSG_REQUIRE_PTR(nn); FPSG_REQUIRE_PTR(nn_d2); FPSG_REQUIRE_PTR(ball_value); FPSG_REQUIRE_PTR(per_percent);
  FPSG_REQUIRE_PTR(value); FPSG_REQUIRE_PTR(workspace);
  FPSG_REQUIRE(workspace_bytes >= fpsg_uniform_workspace_bytes(B, N, S, T, cap), FPSG_E_SHAPE,
               "fpsg_uniform_fwd: workspace of %zu bytes, %zu needed", workspace_bytes,
               fpsg_uniform_workspace_bytes(B, N, S, T, cap));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int total = B * S;                                        // at most 16384 B: B is bounded by the outputs' size
  const unsigned blocks = (unsigned)((total + kUniWaves - 1) / kUniWaves);
  float* rows = static_cast<float*>(workspace);
#define FPSG_UNI_FWD(V)                                                                                             \
  hipLaunchKernelGGL(uniform_fwd_kernel<V>, dim3(blocks), dim3(kUniThreads), 0, s, xyz, seeds, N, S, T, total, prm, \
                     count, member, nn, nn_d2, ball_value);
  if (cap == 64) { FPSG_UNI_FWD(1) }
  else if (cap == 128) { FPSG_UNI_FWD(2) }
  else { FPSG_UNI_FWD(4) }
#undef FPSG_UNI_FWD
  if (const int rc = launch_status("fpsg_uniform_fwd")) return rc;
  hipLaunchKernelGGL(uniform_rows_kernel, dim3((unsigned)(B * T)), dim3(kWave), 0, s, ball_value, S, rows, per_percent);
  if (const int rc = launch_status("fpsg_uniform_fwd")) return rc;
  hipLaunchKernelGGL(uniform_finalize_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, rows, B, T, S, value);
  return launch_status("fpsg_uniform_fwd");
}

extern "C" int fpsg_uniform_bwd(const float* xyz, const int32_t* seeds, const int32_t* count, const int32_t* member,
                                const int32_t* nn, const float* nn_d2, const float* gvalue, int B, int N, int S, int T,
                                const float* percent, float radius, int cap, float* gxyz, fpsg_stream_t stream) {
  using namespace fpsg;
  if (const int rc = uni_check_ints("fpsg_uniform_bwd", B, N, S, T, radius, cap)) return rc;
  UniParams prm;
  if (const int rc = uni_params("fpsg_uniform_bwd", percent, N, T, radius, &prm)) return rc;
  FPSG_REQUIRE_PTR(xyz); FPSG_REQUIRE_PTR(seeds); FPSG_REQUIRE_PTR(count); FPSG_REQUIRE_PTR(member);
  FPSG_REQUIRE_PTR(nn); FPSG_REQUIRE_PTR(nn_d2); FPSG_REQUIRE_PTR(gvalue); FPSG_REQUIRE_PTR(gxyz);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((N + kUniBwdThreads - 1) / kUniBwdThreads), (unsigned)B);
  const float scale = (float)(1.0 / ((double)T * (double)S));
  hipLaunchKernelGGL(uniform_bwd_kernel, grid, dim3(kUniBwdThreads), 0, s, xyz, seeds, count, member, nn, nn_d2, gvalue,
                     N, S, T, cap, prm, scale, gxyz);
  return launch_status("fpsg_uniform_bwd");
}
