// repulsion.hip -- K21: the repulsion regulariser of a cloud against itself (PU-Net's eta(r) w(r) over each point's k
// nearest neighbours in its own cloud), forward and backward, for gfx950.  The definition is in include/fpsg_hip.h
// (K21) and DESIGN.md.
//
// Structure:
//   * forward: grid (ceil(N / 256), B), 256 threads; a lane owns ONE query point and sweeps every candidate j of its
//     cloud in ascending order: the sweep of self_knn.h (K33a calls it as self_knn_sweep; here its pieces, see the
//     kernel).  Candidates pass through LDS in tiles of 1024 (x, y, z as three arrays: every lane of a wave reads the
//     same four candidates with one broadcast ds_read_b128 per coordinate).  The sorted top-k of (d2, j) lives in
//     registers: a K-slot array, K a template parameter (1..8), every loop over it fully unrolled, no dynamic index.
//     The sweep is ascending in j, so a candidate enters only where d2 < the list's last d2 (strictly): an equal
//     distance belongs to a higher index and loses the tie.  j == i is skipped by index.  After the sweep the lane
//     writes its list and adds its K terms (a balanced tree over eight slots, absent ones +0), the wave sums them by
//     the fixed tree, thread 0 adds the four wave sums as (w0 + w1) + (w2 + w3) and writes ONE partial per workgroup;
//     a second, tiny launch adds a cloud's partials in ascending order and scales by 1 / (N k).  No atomics, nothing
//     between workgroups inside a launch.
//   * backward: the same grid and sweep in GATHER form.  The lane that owns point j adds its own k terms in list order
//     (x_m gathered by index), then sweeps every i in ascending order -- x_i and i's k-th pair (d2, idx) staged through
//     LDS -- and adds the reverse term wherever (d2(i, j), j) <= that pair lexicographically, i != j: exactly j in K(i),
//     because sq_dist is bitwise symmetric.  One writer per output, one fixed order: no float atomics, no reverse lists.
//   * padding of the last tile is NaN coordinates: every comparison with a NaN distance is false, so a padded candidate
//     enters no list and no sum.  Every trip count comes from N and k; an index outside [0, N) is never dereferenced.
#include <cmath>

#include "self_knn.h"

namespace fpsg {
namespace {

constexpr int kRepThreads = 256;
constexpr int kRepWaves = kRepThreads / kWave;
constexpr int kRepTile = kSelfKnnTile;                            // candidates per LDS tile
constexpr int kRepPerThread = kRepTile / kRepThreads;
constexpr float kRepFloorD2 = 1e-12f;                             // below this squared distance: r = 1e-6, derivative 0
constexpr float kRepFloorR = 1e-6f;
constexpr float kLog2e = 1.44269504088896340736f;

// exp(-d2 / h^2) = 2^(-((d2 * ih2) * log2 e)): v_exp_f32 itself (dcd.hip); below 2^-126 the result is +0
__device__ __forceinline__ float rep_exp(float d2, float ih2) {
  return __builtin_amdgcn_exp2f(-((d2 * ih2) * kLog2e));
}

__device__ __forceinline__ float rep_radius(float d2) {
  return d2 > kRepFloorD2 ? __builtin_amdgcn_sqrtf(d2) : kRepFloorR;
}

// rho(d2) = -r exp(-d2 / h^2)
__device__ __forceinline__ float rep_term(float d2, float ih2) { return -(rep_radius(d2) * rep_exp(d2, ih2)); }

// rho'(d2) = -exp(-d2 / h^2) (1 / (2 r) - r / h^2); 0 at and below the floor.  Written as e / (2 r) - (e r) / h^2 so
// that an underflowed exponential gives 0 whatever h is (never 0 * inf).
__device__ __forceinline__ float rep_slope(float d2, float ih2) {
  if (!(d2 > kRepFloorD2)) return 0.f;
  const float r = __builtin_amdgcn_sqrtf(d2);
  const float e = rep_exp(d2, ih2);
  return -(e * (0.5f * __builtin_amdgcn_rcpf(r)) - (e * r) * ih2);
}

template <int K>
__global__ __launch_bounds__(kRepThreads) void repulsion_fwd_kernel(const float* __restrict__ xyz, int N, float ih2,
                                                                    int32_t* __restrict__ nbr_idx,
                                                                    float* __restrict__ nbr_d2,
                                                                    float* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float sx[kRepTile];
  __shared__ __attribute__((aligned(16))) float sy[kRepTile];
  __shared__ __attribute__((aligned(16))) float sz[kRepTile];
  __shared__ float wsum[kRepWaves];
  const size_t b = blockIdx.y;
  const float* __restrict__ x = xyz + b * (size_t)N * 3;
  const int i = (int)blockIdx.x * kRepThreads + (int)threadIdx.x;
  const bool live = i < N;
  const float qx = live ? x[3 * (size_t)i + 0] : 0.f;
  const float qy = live ? x[3 * (size_t)i + 1] : 0.f;
  const float qz = live ? x[3 * (size_t)i + 2] : 0.f;

  float d[K];
  int ix[K];
#pragma unroll
  for (int s = 0; s < K; ++s) {
    d[s] = INFINITY;
    ix[s] = -1;
  }

  // self_knn_sweep<K, kRepThreads> of self_knn.h, written out: called as the helper, K = 2 takes one VGPR more (36
  // for 35; the other K one fewer, a different instruction stream for all), so K21 keeps the loop it was measured with.
  for (int j0 = 0; j0 < N; j0 += kRepTile) {                      // every thread of the workgroup: uniform trip count
    __syncthreads();                                              // the previous tile has been read
    stage_xyz_tile<kRepThreads>(x, N, j0, sx, sy, sz);
    __syncthreads();
    const int groups = (min(kRepTile, N - j0) + 3) >> 2;
    for (int g = 0; g < groups; ++g) {
      const v4f X = *reinterpret_cast<const v4f*>(sx + 4 * g);
      const v4f Y = *reinterpret_cast<const v4f*>(sy + 4 * g);
      const v4f Z = *reinterpret_cast<const v4f*>(sz + 4 * g);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + 4 * g + c;
        const float d2 = sq_dist(qx, qy, qz, X[c], Y[c], Z[c]);
        if ((d2 < d[K - 1]) & (j != i)) topk_insert<K>(d, ix, d2, j);
      }
    }
  }

  float term[8];                                                  // the point's terms: a balanced tree over 8 slots
#pragma unroll
  for (int s = 0; s < 8; ++s) term[s] = 0.f;
  if (live) {
    const size_t row = (b * (size_t)N + (size_t)i) * K;
#pragma unroll
    for (int s = 0; s < K; ++s) {
      nbr_idx[row + s] = ix[s];
      nbr_d2[row + s] = d[s];
      term[s] = rep_term(d[s], ih2);
    }
  }
  float t = ((term[0] + term[1]) + (term[2] + term[3])) + ((term[4] + term[5]) + (term[6] + term[7]));
  t = wave_sum(t);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = t;
  __syncthreads();
  static_assert(kRepWaves == 4, "the workgroup's partial is a tree over four wave sums");
  if (threadIdx.x == 0) partials[b * gridDim.x + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// value[b] = (partials of cloud b added in ascending order) * (1 / (N k)); one thread per cloud
__global__ void repulsion_finalize_kernel(const float* __restrict__ partials, int B, int nblk, float rnk,
                                          float* __restrict__ value) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= B) return;
  float s = 0.f;
  for (int p = 0; p < nblk; ++p) s += partials[(size_t)b * nblk + p];
  value[b] = s * rnk;
}

template <int K>
__global__ __launch_bounds__(kRepThreads) void repulsion_bwd_kernel(const float* __restrict__ xyz,
                                                                    const int32_t* __restrict__ nbr_idx,
                                                                    const float* __restrict__ nbr_d2,
                                                                    const float* __restrict__ gvalue, int N, float ih2,
                                                                    float scale, float* __restrict__ gxyz) {
  __shared__ __attribute__((aligned(16))) float sx[kRepTile];
  __shared__ __attribute__((aligned(16))) float sy[kRepTile];
  __shared__ __attribute__((aligned(16))) float sz[kRepTile];
  __shared__ __attribute__((aligned(16))) float sd[kRepTile];     // d2 of candidate i's k-th neighbour (-1: none)
  __shared__ __attribute__((aligned(16))) int si[kRepTile];       // ... and its index
  const size_t b = blockIdx.y;
  const float* __restrict__ x = xyz + b * (size_t)N * 3;
  const int32_t* __restrict__ li = nbr_idx + b * (size_t)N * K;
  const float* __restrict__ ld = nbr_d2 + b * (size_t)N * K;
  const int j = (int)blockIdx.x * kRepThreads + (int)threadIdx.x;
  const bool live = j < N;
  const float qx = live ? x[3 * (size_t)j + 0] : 0.f;
  const float qy = live ? x[3 * (size_t)j + 1] : 0.f;
  const float qz = live ? x[3 * (size_t)j + 2] : 0.f;

  float ax = 0.f, ay = 0.f, az = 0.f;
  if (live) {                                                     // j's own list, nearest first
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const int m = li[(size_t)j * K + s];
      if ((unsigned)m < (unsigned)N) {
        const float w = rep_slope(ld[(size_t)j * K + s], ih2);
        ax = fma_rn(w, qx - x[3 * (size_t)m + 0], ax);
        ay = fma_rn(w, qy - x[3 * (size_t)m + 1], ay);
        az = fma_rn(w, qz - x[3 * (size_t)m + 2], az);
      }
    }
  }

  for (int i0 = 0; i0 < N; i0 += kRepTile) {
    __syncthreads();
    stage_xyz_tile<kRepThreads>(x, N, i0, sx, sy, sz);
#pragma unroll
    for (int u = 0; u < kRepPerThread; ++u) {
      const int t = (int)threadIdx.x + u * kRepThreads;
      const int i = i0 + t;
      int m = -1;
      float dk = -1.f;
      if (i < N) {
        m = li[(size_t)i * K + (K - 1)];
        dk = ld[(size_t)i * K + (K - 1)];
      }
      const bool ok = (unsigned)m < (unsigned)N;                  // a row without a k-th neighbour holds nobody
      sd[t] = ok ? dk : -1.f;
      si[t] = ok ? m : -1;
    }
    __syncthreads();
    const int groups = (min(kRepTile, N - i0) + 3) >> 2;
    for (int g = 0; g < groups; ++g) {
      const v4f X = *reinterpret_cast<const v4f*>(sx + 4 * g);
      const v4f Y = *reinterpret_cast<const v4f*>(sy + 4 * g);
      const v4f Z = *reinterpret_cast<const v4f*>(sz + 4 * g);
      const v4f D = *reinterpret_cast<const v4f*>(sd + 4 * g);
      const v4i I = *reinterpret_cast<const v4i*>(si + 4 * g);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = i0 + 4 * g + c;
        const float d2 = sq_dist(qx, qy, qz, X[c], Y[c], Z[c]);
        // j is in K(i); one predicate, one branch (the short-circuit form costs three scalar branches a candidate)
        if (((d2 < D[c]) | ((d2 == D[c]) & (j <= I[c]))) & (i != j)) {
          const float w = rep_slope(d2, ih2);
          ax = fma_rn(w, qx - X[c], ax);
          ay = fma_rn(w, qy - Y[c], ay);
          az = fma_rn(w, qz - Z[c], az);
        }
      }
    }
  }

  if (live) {
    const float gs = gvalue[b] * scale;
    float* __restrict__ o = gxyz + (b * (size_t)N + (size_t)j) * 3;
    o[0] = ax * gs;
    o[1] = ay * gs;
    o[2] = az * gs;
  }
}

inline int rep_blocks(int N) { return (N + kRepThreads - 1) / kRepThreads; }

// 1 / h^2 as the kernels take it: formed in double, kept inside the finite fp32 range
inline float rep_inv_h2(float h) {
  const double v = 1.0 / ((double)h * (double)h);
  return v > 3.0e38 ? 3.0e38f : (float)v;
}

// Shape and limit checks shared by the two entries (before any pointer check); 0 when the shape is served.
int rep_check_shape(const char* who, int B, int N, int k, float h) {
  FPSG_REQUIRE(B > 0, FPSG_E_SHAPE, "%s: B must be positive (got %d)", who, B);
  FPSG_REQUIRE(k >= 1 && k <= FPSG_REPULSION_MAX_K, FPSG_E_SHAPE, "%s: k must be in 1..%d (got %d)", who,
               FPSG_REPULSION_MAX_K, k);
  FPSG_REQUIRE(N >= k + 1, FPSG_E_SHAPE, "%s: N must be at least k + 1 (got N=%d, k=%d)", who, N, k);
  FPSG_REQUIRE(std::isfinite(h) && h > 0.f, FPSG_E_SHAPE, "%s: h must be positive and finite (got %g)", who, (double)h);
  FPSG_REQUIRE(N <= FPSG_REPULSION_MAX_N, FPSG_E_LIMIT, "%s: N=%d exceeds the supported maximum of %d points", who, N,
               FPSG_REPULSION_MAX_N);
  return 0;
}

}  // namespace
}  // namespace fpsg

extern "C" size_t fpsg_repulsion_workspace_bytes(int B, int N, int k) {
  using namespace fpsg;
  if (B <= 0 || k < 1 || k > FPSG_REPULSION_MAX_K || N < k + 1 || N > FPSG_REPULSION_MAX_N) return 0;
  return (size_t)B * (size_t)rep_blocks(N) * sizeof(float);
}

extern "C" int fpsg_repulsion_fwd(const float* xyz, int B, int N, int k, float h, int32_t* nbr_idx, float* nbr_d2,
                                  float* value, void* workspace, size_t workspace_bytes, fpsg_stream_t stream) {
  using namespace fpsg;
  if (const int rc = rep_check_shape("fpsg_repulsion_fwd", B, N, k, h)) return rc;
  FPSG_REQUIRE_PTR(xyz); FPSG_REQUIRE_PTR(nbr_idx); FPSG_REQUIRE_PTR(nbr_d2); FPSG_REQUIRE_PTR(value);
  FPSG_REQUIRE_PTR(workspace);
  FPSG_REQUIRE(workspace_bytes >= fpsg_repulsion_workspace_bytes(B, N, k), FPSG_E_SHAPE,
               "fpsg_repulsion_fwd: workspace of %zu bytes, %zu needed", workspace_bytes,
               fpsg_repulsion_workspace_bytes(B, N, k));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nblk = rep_blocks(N);
  const dim3 grid((unsigned)nblk, (unsigned)B);
  const float ih2 = rep_inv_h2(h);
  float* partials = static_cast<float*>(workspace);
#define FPSG_REP_FWD(K)                                                                                              \
  case K:                                                                                                            \
    hipLaunchKernelGGL(repulsion_fwd_kernel<K>, grid, dim3(kRepThreads), 0, s, xyz, N, ih2, nbr_idx, nbr_d2, partials); \
    break;
  switch (k) {
    FPSG_REP_FWD(1) FPSG_REP_FWD(2) FPSG_REP_FWD(3) FPSG_REP_FWD(4)
    FPSG_REP_FWD(5) FPSG_REP_FWD(6) FPSG_REP_FWD(7) FPSG_REP_FWD(8)
  }
#undef FPSG_REP_FWD
  if (const int rc = launch_status("fpsg_repulsion_fwd")) return rc;
  const float rnk = (float)(1.0 / ((double)N * (double)k));
  hipLaunchKernelGGL(repulsion_finalize_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, partials, B, nblk, rnk,
                     value);
  return launch_status("fpsg_repulsion_fwd");
}

extern "C" int fpsg_repulsion_bwd(const float* xyz, const int32_t* nbr_idx, const float* nbr_d2, const float* gvalue,
                                  int B, int N, int k, float h, float* gxyz, fpsg_stream_t stream) {
  using namespace fpsg;
  if (const int rc = rep_check_shape("fpsg_repulsion_bwd", B, N, k, h)) return rc;
  FPSG_REQUIRE_PTR(xyz); FPSG_REQUIRE_PTR(nbr_idx); FPSG_REQUIRE_PTR(nbr_d2); FPSG_REQUIRE_PTR(gvalue);
  FPSG_REQUIRE_PTR(gxyz);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)rep_blocks(N), (unsigned)B);
  const float ih2 = rep_inv_h2(h);
  const float scale = (float)(2.0 / ((double)N * (double)k));
#define FPSG_REP_BWD(K)                                                                                             \
  case K:                                                                                                           \
    hipLaunchKernelGGL(repulsion_bwd_kernel<K>, grid, dim3(kRepThreads), 0, s, xyz, nbr_idx, nbr_d2, gvalue, N, ih2, \
                       scale, gxyz);                                                                                \
    break;
  switch (k) {
    FPSG_REP_BWD(1) FPSG_REP_BWD(2) FPSG_REP_BWD(3) FPSG_REP_BWD(4)
    FPSG_REP_BWD(5) FPSG_REP_BWD(6) FPSG_REP_BWD(7) FPSG_REP_BWD(8)
  }
#undef FPSG_REP_BWD
  return launch_status("fpsg_repulsion_bwd");
}
