// expansion.hip -- K24: MSN's expansion penalty of a multi-patch cloud (the minimum spanning tree of every patch of P
// consecutive points, a charge for the tree edges longer than lambda times the patch's mean edge), forward and
// backward, for gfx950.  The definition is in include/fpsg_hip.h (K24) and DESIGN.md.
//
// Structure:
//   * forward: ONE wavefront owns one patch; four patches (two at V = 16) share a workgroup, each with its own LDS
//     slice, and nothing passes between them (one barrier behind the staging, none inside the loop).  Lane t owns the
//     local vertices t, t + 64, ...: V = ceil(P / 64) rounded up to a power of two (a template parameter; 1, 2, 4, 8,
//     16), their coordinates, keys, parents and steps in registers, every loop over them unrolled, no dynamic index.
//     Prim's from vertex 0 under K1's sq_dist: each of the P - 1 steps packs (bits(key) << 32) | vertex per slot --
//     d2 is never negative, so its bits order as unsigned integers; tree members and the padding past P carry the
//     all-ones word -- takes the lane's minimum over its V words and the wave's by six lane exchanges, reads the new
//     vertex's coordinates from LDS (one broadcast read per axis) and lowers every non-tree key that is STRICTLY above
//     the distance to it.  The packing is the tie rule: the smallest (key, index); an equal distance keeps the earlier
//     parent.  Behind the loop: r = sqrt(edge_d2), the patch's mean edge, the penalised sum, ONE partial per patch; a
//     second, tiny launch adds a cloud's K partials in ascending order and divides by K.
//   * backward: the same ownership in GATHER form.  The patch's coordinates, parents and penalised lengths (0 where the
//     edge is not penalised) go through LDS; the lane that owns u adds its own edge's term, then the wave walks the
//     penalised vertices v in ascending order (a ballot per slot: the walk is wave-uniform) and the owner of
//     parent[v] adds the child term.  One writer per output, one fixed order, no float atomics.
//   * every trip count comes from P; the index of the new vertex is masked to the slice, a parent outside [0, P) is
//     skipped: no index is dereferenced unchecked, whatever the coordinates or the saved arrays hold.
#include <cmath>

#include "chamfer_dist.h"

namespace fpsg {
namespace {

// patches per workgroup: four, two at V = 16 (the backward's five slices of 1024 words each stay below 64 KB of LDS)
template <int V>
struct ExpShape {
  static constexpr int kWaves = V >= 16 ? 2 : 4;
  static constexpr int kThreads = kWaves * kWave;
};

// the length of a tree edge; the forward's penalised test and the backward's recompute it from the same bits
__device__ __forceinline__ float exp_len(float d2) { return sqrtf(d2); }

template <int V>
__global__ __launch_bounds__(ExpShape<V>::kThreads) void expansion_fwd_kernel(
    const float* __restrict__ xyz, int P, int total, float lambda, int32_t* __restrict__ parent,
    float* __restrict__ edge_d2, int32_t* __restrict__ order, float* __restrict__ mean_len,
    float* __restrict__ partials) {
  constexpr int S = V * kWave;                                    // the slice: P rounded up
  constexpr int kExpWaves = ExpShape<V>::kWaves;
  __shared__ float sx[kExpWaves][S];
  __shared__ float sy[kExpWaves][S];
  __shared__ float sz[kExpWaves][S];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int g = (int)blockIdx.x * kExpWaves + wave;               // the patch: cloud g / K, patch g % K (N = K P)
  const bool live = g < total;
  const size_t base = (size_t)(live ? g : 0) * (size_t)P;
  const float* __restrict__ x = xyz + base * 3;

  float px[V], py[V], pz[V];
#pragma unroll
  for (int s = 0; s < V; ++s) {
    const int v = lane + s * kWave;
    const bool ok = live & (v < P);
    px[s] = ok ? x[3 * (size_t)v + 0] : 0.f;
    py[s] = ok ? x[3 * (size_t)v + 1] : 0.f;
    pz[s] = ok ? x[3 * (size_t)v + 2] : 0.f;
    sx[wave][v] = px[s];
    sy[wave][v] = py[s];
    sz[wave][v] = pz[s];
  }
  __syncthreads();                                                // the only one; every wave reaches it
  if (!live) return;

  float key[V];
  int par[V], ord[V];
  unsigned in = 0;                                                // bit s: slot s is a tree member (or padding)
  {
    const float ux = sx[wave][0], uy = sy[wave][0], uz = sz[wave][0];
#pragma unroll
    for (int s = 0; s < V; ++s) {
      const int v = lane + s * kWave;
      const bool root = v == 0;
      key[s] = root ? 0.f : sq_dist(px[s], py[s], pz[s], ux, uy, uz);
      par[s] = root ? -1 : 0;
      ord[s] = 0;
      in |= (unsigned)(root | (v >= P)) << s;
    }
  }

  for (int step = 1; step < P; ++step) {                          // P - 1 dependent steps; the count comes from P alone
    unsigned long long best = ~0ull;
#pragma unroll
    for (int s = 0; s < V; ++s) {
      const unsigned long long w = ((unsigned long long)__float_as_uint(key[s]) << 32) | (unsigned)(lane + s * kWave);
      const unsigned long long c = ((in >> s) & 1u) ? ~0ull : w;
      best = c < best ? c : best;
    }
    best = wave_min_u64(best);
    // a non-tree vertex below P exists at every step, so the word is never all ones; the mask keeps the read inside
    // the slice whatever happens
    const int u = __builtin_amdgcn_readfirstlane((int)((unsigned)best & (unsigned)(S - 1)));
    const float ux = sx[wave][u], uy = sy[wave][u], uz = sz[wave][u];
#pragma unroll
    for (int s = 0; s < V; ++s) {
      const bool me = (lane + s * kWave) == u;
      ord[s] = me ? step : ord[s];
      in |= (unsigned)me << s;
      const float d = sq_dist(px[s], py[s], pz[s], ux, uy, uz);
      const bool lower = (((in >> s) & 1u) == 0u) & (d < key[s]);  // strictly: on a tie the earlier parent stays
      key[s] = lower ? d : key[s];
      par[s] = lower ? u : par[s];
    }
  }

  float r[V];
  float ls = 0.f;
#pragma unroll
  for (int s = 0; s < V; ++s) {
    const bool ok = (lane + s * kWave) < P;
    r[s] = ok ? exp_len(key[s]) : 0.f;
    ls += r[s];
  }
  const float l = wave_sum(ls) / (float)(P - 1);
  const float thr = lambda * l;
  float es = 0.f;
#pragma unroll
  for (int s = 0; s < V; ++s) es += (r[s] > thr) ? r[s] : 0.f;
  es = wave_sum(es);

#pragma unroll
  for (int s = 0; s < V; ++s) {
    const int v = lane + s * kWave;
    if (v < P) {
      parent[base + (size_t)v] = par[s];
      edge_d2[base + (size_t)v] = key[s];
      order[base + (size_t)v] = ord[s];
    }
  }
  if (lane == 0) {
    mean_len[g] = l;
    partials[g] = es / (float)(P - 1);
  }
}

// value[b] = (the K partials of cloud b added in ascending order from +0) / K; one thread per cloud
__global__ void expansion_finalize_kernel(const float* __restrict__ partials, int B, int K, float* __restrict__ value) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= B) return;
  float s = 0.f;
  for (int q = 0; q < K; ++q) s += partials[(size_t)b * K + q];
  value[b] = s / (float)K;
}

template <int V>
__global__ __launch_bounds__(ExpShape<V>::kThreads) void expansion_bwd_kernel(
    const float* __restrict__ xyz, const int32_t* __restrict__ parent, const float* __restrict__ edge_d2,
    const float* __restrict__ mean_len, const float* __restrict__ gvalue, int P, int K, int total, float lambda,
    float scale, float* __restrict__ gxyz) {
  constexpr int S = V * kWave;
  constexpr int kExpWaves = ExpShape<V>::kWaves;
  __shared__ float sx[kExpWaves][S];
  __shared__ float sy[kExpWaves][S];
  __shared__ float sz[kExpWaves][S];
  __shared__ float sr[kExpWaves][S];                              // the edge's length where it is penalised, else 0
  __shared__ int sp[kExpWaves][S];                                // the parent where it is inside [0, P), else -1
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int g = (int)blockIdx.x * kExpWaves + wave;
  const bool live = g < total;
  const size_t base = (size_t)(live ? g : 0) * (size_t)P;
  const float* __restrict__ x = xyz + base * 3;
  const float thr = live ? lambda * mean_len[g] : 0.f;            // the forward's expression on the forward's bits

#pragma unroll
  for (int s = 0; s < V; ++s) {
    const int v = lane + s * kWave;
    const bool ok = live & (v < P);
    sx[wave][v] = ok ? x[3 * (size_t)v + 0] : 0.f;
    sy[wave][v] = ok ? x[3 * (size_t)v + 1] : 0.f;
    sz[wave][v] = ok ? x[3 * (size_t)v + 2] : 0.f;
    const int p = ok ? parent[base + (size_t)v] : -1;
    const float len = ok ? exp_len(edge_d2[base + (size_t)v]) : 0.f;
    const bool pen = ok & ((unsigned)p < (unsigned)P) & (len > thr) & (len > 0.f);
    sr[wave][v] = pen ? len : 0.f;
    sp[wave][v] = pen ? p : -1;
  }
  __syncthreads();
  if (!live) return;

  // (x_a - x_b) / r per axis, for the owner of a: the own edge's term with (a, b) = (u, par(u)), a child's with (u, v)
  float ax[V], ay[V], az[V];
#pragma unroll
  for (int s = 0; s < V; ++s) {                                   // the vertex's own edge
    const int v = lane + s * kWave;
    const int p = sp[wave][v];
    ax[s] = ay[s] = az[s] = 0.f;
    if (p >= 0) {
      const float rv = sr[wave][v];
      ax[s] = (sx[wave][v] - sx[wave][p]) / rv;
      ay[s] = (sy[wave][v] - sy[wave][p]) / rv;
      az[s] = (sz[wave][v] - sz[wave][p]) / rv;
    }
  }
#pragma unroll
  for (int s = 0; s < V; ++s) {                                   // the penalised children, ascending v
    unsigned long long m = __ballot(sp[wave][lane + s * kWave] >= 0);
    while (m) {                                                   // wave-uniform
      const int v = s * kWave + (int)__builtin_ctzll(m);
      m &= m - 1;
      const int u = __builtin_amdgcn_readfirstlane(sp[wave][v]);  // inside [0, P): checked when it was staged
      const float rv = sr[wave][v];
      const float tx = (sx[wave][u] - sx[wave][v]) / rv;          // broadcast reads: every lane forms the same term
      const float ty = (sy[wave][u] - sy[wave][v]) / rv;
      const float tz = (sz[wave][u] - sz[wave][v]) / rv;
      const int slot = u >> 6;
      const bool hit = lane == (u & 63);
#pragma unroll
      for (int t = 0; t < V; ++t) {
        const bool add = hit & (t == slot);
        ax[t] = add ? ax[t] + tx : ax[t];
        ay[t] = add ? ay[t] + ty : ay[t];
        az[t] = add ? az[t] + tz : az[t];
      }
    }
  }

  const float gs = gvalue[g / K] * scale;
#pragma unroll
  for (int s = 0; s < V; ++s) {
    const int v = lane + s * kWave;
    if (v < P) {
      float* __restrict__ o = gxyz + (base + (size_t)v) * 3;
      o[0] = ax[s] * gs;
      o[1] = ay[s] * gs;
      o[2] = az[s] * gs;
    }
  }
}

// Shape and limit checks shared by the two entries (before any pointer check); 0 when the shape is served.
int exp_check_shape(const char* who, int B, int N, int P, float lambda) {
  FPSG_REQUIRE(B > 0, FPSG_E_SHAPE, "%s: B must be positive (got %d)", who, B);
  FPSG_REQUIRE(P >= 2, FPSG_E_SHAPE, "%s: P must be at least 2 (got %d)", who, P);
  FPSG_REQUIRE(N >= P && N % P == 0, FPSG_E_SHAPE, "%s: N must be a positive multiple of P (got N=%d, P=%d)", who, N, P);
  FPSG_REQUIRE(std::isfinite(lambda) && lambda >= 1.f, FPSG_E_SHAPE, "%s: lambda must be finite and at least 1 (got %g)",
               who, (double)lambda);
  FPSG_REQUIRE(P <= FPSG_EXPANSION_MAX_P, FPSG_E_LIMIT, "%s: P=%d exceeds the supported maximum of %d points per patch",
               who, P, FPSG_EXPANSION_MAX_P);
  FPSG_REQUIRE(N <= FPSG_EXPANSION_MAX_N, FPSG_E_LIMIT, "%s: N=%d exceeds the supported maximum of %d points", who, N,
               FPSG_EXPANSION_MAX_N);
  return 0;
}

template <int V>
inline unsigned exp_blocks(int total) {
  return (unsigned)((total + ExpShape<V>::kWaves - 1) / ExpShape<V>::kWaves);
}

}  // namespace
}  // namespace fpsg

extern "C" size_t fpsg_expansion_workspace_bytes(int B, int N, int P) {
  if (B <= 0 || P < 2 || P > FPSG_EXPANSION_MAX_P || N < P || N % P != 0 || N > FPSG_EXPANSION_MAX_N) return 0;
  return (size_t)B * (size_t)(N / P) * sizeof(float);
}

// V for P: ceil(P / 64) rounded up to a power of two
#define FPSG_EXP_DISPATCH(P, LAUNCH)        \
  do {                                      \
    if ((P) <= 64) { LAUNCH(1) }            \
    else if ((P) <= 128) { LAUNCH(2) }      \
    else if ((P) <= 256) { LAUNCH(4) }      \
    else if ((P) <= 512) { LAUNCH(8) }      \
    else { LAUNCH(16) }                     \
  } while (0)

extern "C" int fpsg_expansion_fwd(const float* xyz, int B, int N, int P, float lambda, int32_t* parent, float* edge_d2,
                                  int32_t* order, float* mean_len, float* value, void* workspace,
                                  size_t workspace_bytes, fpsg_stream_t stream) {
  using namespace fpsg;
  if (const int rc = exp_check_shape("fpsg_expansion_fwd", B, N, P, lambda)) return rc;
  FPSG_REQUIRE_PTR(xyz); FPSG_REQUIRE_PTR(parent); FPSG_REQUIRE_PTR(edge_d2); FPSG_REQUIRE_PTR(order);
  FPSG_REQUIRE_PTR(mean_len); FPSG_REQUIRE_PTR(value); FPSG_REQUIRE_PTR(workspace);
  FPSG_REQUIRE(workspace_bytes >= fpsg_expansion_workspace_bytes(B, N, P), FPSG_E_SHAPE,
               "fpsg_expansion_fwd: workspace of %zu bytes, %zu needed", workspace_bytes,
               fpsg_expansion_workspace_bytes(B, N, P));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int K = N / P, total = B * K;
  float* partials = static_cast<float*>(workspace);
#define FPSG_EXP_FWD(V)                                                                                      \
  hipLaunchKernelGGL(expansion_fwd_kernel<V>, dim3(exp_blocks<V>(total)), dim3(ExpShape<V>::kThreads), 0, s, xyz, P, \
                     total, lambda, parent, edge_d2, order, mean_len, partials);
  FPSG_EXP_DISPATCH(P, FPSG_EXP_FWD);
#undef FPSG_EXP_FWD
  if (const int rc = launch_status("fpsg_expansion_fwd")) return rc;
  hipLaunchKernelGGL(expansion_finalize_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, partials, B, K, value);
  return launch_status("fpsg_expansion_fwd");
}

extern "C" int fpsg_expansion_bwd(const float* xyz, const int32_t* parent, const float* edge_d2, const float* mean_len,
                                  const float* gvalue, int B, int N, int P, float lambda, float* gxyz,
                                  fpsg_stream_t stream) {
  using namespace fpsg;
  if (const int rc = exp_check_shape("fpsg_expansion_bwd", B, N, P, lambda)) return rc;
  FPSG_REQUIRE_PTR(xyz); FPSG_REQUIRE_PTR(parent); FPSG_REQUIRE_PTR(edge_d2); FPSG_REQUIRE_PTR(mean_len);
  FPSG_REQUIRE_PTR(gvalue); FPSG_REQUIRE_PTR(gxyz);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int K = N / P, total = B * K;
  const float scale = (float)(1.0 / ((double)K * (double)(P - 1)));
#define FPSG_EXP_BWD(V)                                                                                    \
  hipLaunchKernelGGL(expansion_bwd_kernel<V>, dim3(exp_blocks<V>(total)), dim3(ExpShape<V>::kThreads), 0, s, xyz, \
                     parent, edge_d2, mean_len, gvalue, P, K, total, lambda, scale, gxyz);
  FPSG_EXP_DISPATCH(P, FPSG_EXP_BWD);
#undef FPSG_EXP_BWD
  return launch_status("fpsg_expansion_bwd");
}
