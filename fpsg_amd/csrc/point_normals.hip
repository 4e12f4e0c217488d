// point_normals.hip -- K33: normals of a bare point cloud (Hoppe et al. 1992), for gfx950.  K33a: the k nearest
// neighbours of every point in its own cloud, PCA of the neighbourhood, the eigenvector of the smallest eigenvalue with
// a local sign rule.  K33b: a consistent orientation, propagated along the minimum spanning forest of the neighbour
// graph.  The definitions are in include/fpsg_hip.h (K33) and DESIGN.md.
//
// Structure:
//   * K33a, selection: K21's sweep (self_knn_sweep of self_knn.h, described in repulsion.hip) with longer lists.  One
//     wave per workgroup, grid (ceil(N / 64), B); a lane owns ONE query.  K is a template parameter (8, 16 or 32: the
//     call's k rounded up; the first k slots of the sorted top-K ARE the top-k).  The lists go to nbr_idx, or to the
//     workspace when the caller does not want them.
//   * K33a, PCA: one thread per point reads its list back, gathers the neighbours, and works on offsets from the point
//     itself (exact where the cloud sits far from the origin): mean, centred covariance, trace-scaled, eight cyclic
//     Jacobi sweeps on the 3x3 (a fixed count), the column of the smallest diagonal entry, normalised; then the sign.
//   * K33b: two gather sweeps build the reverse lists (who names u as a neighbour) as a CSR without atomics -- count,
//     then fill, the fill's workgroups summing the counts in front of them -- and ONE workgroup per cloud runs Prim's
//     for exactly N steps: keys (order-preserving integer images of the fp32 weights) and parents in LDS, the smallest
//     (key, index) by a wave exchange tree and one LDS round, the new vertex's forward and reverse lists relaxed by
//     the workgroup, its sign fixed by thread 0 from its parent's oriented normal.  Racing writers of one key write
//     the same words.  No atomics, nothing between workgroups.
//   * every index read from a list is checked against [0, N) before it is used; every trip count comes from N and k.
#include <cmath>

#include "self_knn.h"

namespace fpsg {
namespace {

constexpr int kPnThreads = 64;                                    // selection: one wave per workgroup
constexpr int kPnPcaThreads = 256;
constexpr int kPnJacobiSweeps = 8;

template <int K>
__global__ __launch_bounds__(kPnThreads) void pn_select_kernel(const float* __restrict__ xyz, int N, int k,
                                                               int32_t* __restrict__ nbr_idx) {
  __shared__ __attribute__((aligned(16))) float sx[kSelfKnnTile];
  __shared__ __attribute__((aligned(16))) float sy[kSelfKnnTile];
  __shared__ __attribute__((aligned(16))) float sz[kSelfKnnTile];
  const size_t b = blockIdx.y;
  const float* __restrict__ x = xyz + b * (size_t)N * 3;
  const int i = (int)blockIdx.x * kPnThreads + (int)threadIdx.x;
  const bool live = i < N;
  const float qx = live ? x[3 * (size_t)i + 0] : 0.f;
  const float qy = live ? x[3 * (size_t)i + 1] : 0.f;
  const float qz = live ? x[3 * (size_t)i + 2] : 0.f;

  float d[K];
  int ix[K];
  self_knn_sweep<K, kPnThreads>(x, N, i, qx, qy, qz, d, ix, sx, sy, sz);     // every thread of the workgroup

  if (live) {
    int32_t* __restrict__ row = nbr_idx + (b * (size_t)N + (size_t)i) * (size_t)k;
#pragma unroll
    for (int s = 0; s < K; ++s)                                   // a slot nobody entered (non-finite coordinates): i itself
      if (s < k) row[s] = (unsigned)ix[s] < (unsigned)N ? ix[s] : i;
  }
}

// One Jacobi rotation of the symmetric 3x3 in the plane (p, q); r is the third index.  A' = J^T A J, V' = V J with
// J_pp = J_qq = c, J_pq = s, J_qp = -s; theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)),
// c = 1 / sqrt(t^2 + 1), s = t c.  a_pq == 0 (and a theta whose square overflows) gives t = 0: the identity.
__device__ __forceinline__ void pn_rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float& v0p,
                                          float& v0q, float& v1p, float& v1q, float& v2p, float& v2q) {
  const float theta = (aqq - app) / (2.f * apq);
  const float t0 = copysignf(1.f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
  const float t = apq != 0.f ? t0 : 0.f;
  const float c = 1.f / sqrtf(t * t + 1.f);
  const float s = t * c;
  const float h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.f;
  const float rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp; arq = rq;
  const float x0 = c * v0p - s * v0q, y0 = s * v0p + c * v0q;
  const float x1 = c * v1p - s * v1q, y1 = s * v1p + c * v1q;
  const float x2 = c * v2p - s * v2q, y2 = s * v2p + c * v2q;
  v0p = x0; v0q = y0; v1p = x1; v1q = y1; v2p = x2; v2q = y2;
}

__global__ __launch_bounds__(kPnPcaThreads) void pn_pca_kernel(const float* __restrict__ xyz,
                                                               const int32_t* __restrict__ nbr_idx, int N, int k,
                                                               long long total, int sign_mode,
                                                               const float* __restrict__ ref,
                                                               float* __restrict__ normals,
                                                               float* __restrict__ variation) {
  const long long t = (long long)blockIdx.x * kPnPcaThreads + threadIdx.x;      // b N + i
  if (t >= total) return;
  const long long b = t / N;
  const int i = (int)(t - b * N);
  const float* __restrict__ x = xyz + (size_t)b * (size_t)N * 3;
  const int32_t* __restrict__ row = nbr_idx + (size_t)t * (size_t)k;
  const float px = x[3 * (size_t)i + 0], py = x[3 * (size_t)i + 1], pz = x[3 * (size_t)i + 2];

  // offsets from the point itself; the point's own offset is 0 and adds nothing to the sums
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int s = 0; s < k; ++s) {
    int j = row[s];
    j = (unsigned)j < (unsigned)N ? j : i;
    sx += x[3 * (size_t)j + 0] - px;
    sy += x[3 * (size_t)j + 1] - py;
    sz += x[3 * (size_t)j + 2] - pz;
  }
  const float n1 = (float)(k + 1);
  const float mx = sx / n1, my = sy / n1, mz = sz / n1;
  float c00 = mx * mx, c01 = mx * my, c02 = mx * mz, c11 = my * my, c12 = my * mz, c22 = mz * mz;   // the point: 0 - m
  for (int s = 0; s < k; ++s) {
    int j = row[s];
    j = (unsigned)j < (unsigned)N ? j : i;
    const float dx = (x[3 * (size_t)j + 0] - px) - mx;
    const float dy = (x[3 * (size_t)j + 1] - py) - my;
    const float dz = (x[3 * (size_t)j + 2] - pz) - mz;
    c00 += dx * dx; c01 += dx * dy; c02 += dx * dz;
    c11 += dy * dy; c12 += dy * dz; c22 += dz * dz;
  }
  const float trace = (c00 + c11) + c22;
  const float sc = 1.f / trace;
  float nx = 0.f, ny = 0.f, nz = 0.f, var = 0.f;
  if (trace > 0.f && sc > 0.f && sc < INFINITY) {                 // false for a NaN trace
    float a00 = c00 * sc, a01 = c01 * sc, a02 = c02 * sc, a11 = c11 * sc, a12 = c12 * sc, a22 = c22 * sc;
    float v00 = 1.f, v01 = 0.f, v02 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v20 = 0.f, v21 = 0.f, v22 = 1.f;
    for (int sweep = 0; sweep < kPnJacobiSweeps; ++sweep) {       // a fixed count
      pn_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
      pn_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
      pn_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    const int m = (a00 <= a11 && a00 <= a22) ? 0 : (a11 <= a22 ? 1 : 2);
    const float ex = m == 0 ? v00 : m == 1 ? v01 : v02;
    const float ey = m == 0 ? v10 : m == 1 ? v11 : v12;
    const float ez = m == 0 ? v20 : m == 1 ? v21 : v22;
    const float l0 = m == 0 ? a00 : m == 1 ? a11 : a22;
    const float r = 1.f / sqrtf((ex * ex + ey * ey) + ez * ez);
    nx = ex * r; ny = ey * r; nz = ez * r;
    var = __builtin_fminf(__builtin_fmaxf(l0, 0.f) / ((a00 + a11) + a22), 1.f / 3.f);
    // canonical sign: the component of largest magnitude positive, the lowest axis on ties
    const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
    const float lead = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
    bool flip = lead < 0.f;
    if (sign_mode != 0) {
      const float* __restrict__ q = ref + (size_t)b * 3;
      const float dot = (nx * (q[0] - px) + ny * (q[1] - py)) + nz * (q[2] - pz);
      const float toward = flip ? -dot : dot;                     // n . (ref - p) under the canonical sign
      if (sign_mode == 1 && toward < 0.f) flip = !flip;
      if (sign_mode == 2 && toward > 0.f) flip = !flip;
    }
    if (flip) { nx = -nx; ny = -ny; nz = -nz; }
    if (!(nx == nx && ny == ny && nz == nz)) { nx = ny = nz = 0.f; var = 0.f; }   // non-finite input: unspecified, kept plain
  }
  normals[(size_t)t * 3 + 0] = nx;
  normals[(size_t)t * 3 + 1] = ny;
  normals[(size_t)t * 3 + 2] = nz;
  if (variation != nullptr) variation[t] = var;
}

// ---- K33b -------------------------------------------------------------------------------------------------------------
constexpr int kRvThreads = 256;
constexpr int kRvRows = 128;                                      // list rows per LDS tile (k padded to a multiple of 4)
constexpr unsigned kKeyTree = 0xffffffffu;                        // the vertex is in the tree
constexpr unsigned kKeyNone = 0xfffffffeu;                        // no tree vertex is adjacent yet
constexpr unsigned kKeyMax = 0xfffffffdu;                         // the largest image of a weight

// an unsigned image of a float with the same order (negative values below positive ones)
__device__ __forceinline__ unsigned pn_ordered(float f) {
  const unsigned u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

// Reverse lists in gather form: the lane that owns u sweeps every row v of the table in ascending order and takes the
// entries equal to u (v != u).  FILL = false counts them; FILL = true writes the rows v at off[u] onwards, off = the
// exclusive sum of the counts in index order (each workgroup adds up the counts in front of it).
template <bool FILL>
__global__ __launch_bounds__(kRvThreads) void pn_reverse_kernel(const int32_t* __restrict__ nbr_idx, int N, int k,
                                                                int32_t* __restrict__ cnt, int32_t* __restrict__ off,
                                                                int32_t* __restrict__ rev) {
  __shared__ __attribute__((aligned(16))) int tile[kRvRows * FPSG_NORMALS_POINTS_MAX_K];
  __shared__ int scan[kRvThreads];
  const size_t b = blockIdx.y;
  const int tid = (int)threadIdx.x;
  const int first = (int)blockIdx.x * kRvThreads;
  const int u = first + tid < N ? first + tid : -2;               // -2 matches no entry (padding is -1)
  const int32_t* __restrict__ L = nbr_idx + b * (size_t)N * (size_t)k;
  const int kp = (k + 3) & ~3;
  const long long cap = (long long)N * k;

  long long base = 0;
  if (FILL) {
    int before = 0;
    for (int j = tid; j < first; j += kRvThreads) before += cnt[b * (size_t)N + (size_t)j];
    scan[tid] = before;
    __syncthreads();
    int total = 0;
#pragma unroll 4
    for (int j = 0; j < kRvThreads; ++j) total += scan[j];        // integers: the order does not matter
    __syncthreads();
    scan[tid] = u >= 0 ? cnt[b * (size_t)N + (size_t)u] : 0;
    __syncthreads();
    int mine = 0;
#pragma unroll 1
    for (int j = 0; j < tid; ++j) mine += scan[j];
    base = (long long)total + mine;
  }

  int n = 0;
  for (int v0 = 0; v0 < N; v0 += kRvRows) {
    __syncthreads();
    for (int e = tid; e < kRvRows * kp; e += kRvThreads) {
      const int r = e / kp, s = e - r * kp, v = v0 + r;
      int val = (v < N && s < k) ? L[(size_t)v * (size_t)k + (size_t)s] : -1;
      tile[e] = val == v ? -1 : val;                              // a row's own index is no edge
    }
    __syncthreads();
    const int rows = min(kRvRows, N - v0);
    for (int r = 0; r < rows; ++r) {
      for (int s = 0; s < kp; s += 4) {
        const v4i q = *reinterpret_cast<const v4i*>(tile + r * kp + s);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (q[c] == u) {
            if (FILL && base + n < cap) rev[b * (size_t)cap + (size_t)(base + n)] = v0 + r;
            ++n;
          }
        }
      }
    }
  }
  if (u >= 0) {
    if (FILL) off[b * (size_t)N + (size_t)u] = (int32_t)(base < cap ? base : cap);
    else cnt[b * (size_t)N + (size_t)u] = n;
  }
}

constexpr int kOrMaxThreads = 1024;
constexpr int kOrMaxWaves = kOrMaxThreads / kWave;

inline size_t orient_lds_bytes(int N) { return (size_t)(2 * kOrMaxWaves) * 8 + (size_t)N * 8; }
inline int orient_threads(int N) { return N <= 512 ? 64 : N <= 4096 ? 256 : kOrMaxThreads; }

__global__ __launch_bounds__(kOrMaxThreads) void pn_orient_kernel(const float* __restrict__ xyz,
                                                                  const float* __restrict__ normals_in,
                                                                  const int32_t* __restrict__ nbr_idx,
                                                                  const int32_t* __restrict__ cnt,
                                                                  const int32_t* __restrict__ off,
                                                                  const int32_t* __restrict__ rev, int N, int k, int axis,
                                                                  float* normals_out, int32_t* __restrict__ parent) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long pn_lds[];
  unsigned long long* red = pn_lds;                               // [kOrMaxWaves] minima, [kOrMaxWaves] maxima
  unsigned* key = reinterpret_cast<unsigned*>(pn_lds + 2 * kOrMaxWaves);   // [N]
  int* par = reinterpret_cast<int*>(key + N);                     // [N]
  const size_t b = blockIdx.x;
  const int tid = (int)threadIdx.x, T = (int)blockDim.x, lane = tid & 63, wave = tid >> 6, waves = T >> 6;
  const long long cap = (long long)N * k;
  const float* __restrict__ x = xyz + b * (size_t)N * 3;
  const float* __restrict__ nin = normals_in + b * (size_t)N * 3;
  const int32_t* __restrict__ L = nbr_idx + b * (size_t)cap;
  const int32_t* __restrict__ R = rev + b * (size_t)cap;
  const int32_t* __restrict__ C = cnt + b * (size_t)N;
  const int32_t* __restrict__ O = off + b * (size_t)N;
  float* nout = normals_out + b * (size_t)N * 3;

  for (int v = tid; v < N; v += T) {
    key[v] = kKeyNone;
    par[v] = -1;
  }
  __syncthreads();

  for (int step = 0; step < N; ++step) {                          // exactly N steps: one vertex joins per step
    unsigned long long best = ~0ull;
    for (int v = tid; v < N; v += T) {
      const unsigned long long w = ((unsigned long long)key[v] << 32) | (unsigned)v;
      best = w < best ? w : best;
    }
    best = wave_min_u64(best);
    if (lane == 0) red[wave] = best;
    __syncthreads();
    best = red[0];
    for (int w = 1; w < waves; ++w) best = red[w] < best ? red[w] : best;
    const bool root = (unsigned)(best >> 32) >= kKeyNone;          // the same in every thread
    unsigned pick = (unsigned)best;
    if (root) {                                                   // nobody has a key: the topmost vertex outside the tree
      unsigned long long top = 0ull;
      for (int v = tid; v < N; v += T) {
        if (key[v] != kKeyTree) {
          const unsigned long long w =
              ((unsigned long long)pn_ordered(x[3 * (size_t)v + (size_t)axis]) << 32) | (0xffffffffu - (unsigned)v);
          top = w > top ? w : top;
        }
      }
      top = wave_max_u64(top);
      if (lane == 0) red[kOrMaxWaves + wave] = top;
      __syncthreads();
      top = red[kOrMaxWaves];
      for (int w = 1; w < waves; ++w) top = red[kOrMaxWaves + w] > top ? red[kOrMaxWaves + w] : top;
      pick = 0xffffffffu - (unsigned)top;
    }
    const int u = __builtin_amdgcn_readfirstlane((int)(pick < (unsigned)N ? pick : (unsigned)(N - 1)));
    const int p = root ? -1 : par[u];
    const float ux = nin[3 * (size_t)u + 0], uy = nin[3 * (size_t)u + 1], uz = nin[3 * (size_t)u + 2];

    long long deg = C[u], o = O[u];
    deg = deg < 0 ? 0 : deg;
    o = o < 0 ? 0 : o;
    deg = o + deg > cap ? (o < cap ? cap - o : 0) : deg;          // the reverse list stays inside the cloud's slice
    const int edges = k + (int)deg;
    for (int e = tid; e < edges; e += T) {
      const int v = e < k ? L[(size_t)u * (size_t)k + (size_t)e] : R[(size_t)(o + (e - k))];
      if ((unsigned)v < (unsigned)N && v != u) {
        const unsigned kv = key[v];
        if (kv != kKeyTree) {
          const float vx = nin[3 * (size_t)v + 0], vy = nin[3 * (size_t)v + 1], vz = nin[3 * (size_t)v + 2];
          const float w = 1.f - fabsf((ux * vx + uy * vy) + uz * vz);
          const unsigned img = pn_ordered(w);
          const unsigned mk = img < kKeyMax ? img : kKeyMax;
          if (mk < kv) {                                          // strictly: on a tie the earlier parent stays
            key[v] = mk;
            par[v] = u;
          }
        }
      }
    }
    if (tid == 0) {
      bool flip;
      if ((unsigned)p < (unsigned)N) {
        const float qx = nout[3 * (size_t)p + 0], qy = nout[3 * (size_t)p + 1], qz = nout[3 * (size_t)p + 2];
        flip = ((qx * ux + qy * uy) + qz * uz) < 0.f;
      } else {
        flip = (axis == 0 ? ux : axis == 1 ? uy : uz) < 0.f;
      }
      nout[3 * (size_t)u + 0] = flip ? -ux : ux;
      nout[3 * (size_t)u + 1] = flip ? -uy : uy;
      nout[3 * (size_t)u + 2] = flip ? -uz : uz;
      if (parent != nullptr) parent[b * (size_t)N + (size_t)u] = (unsigned)p < (unsigned)N ? p : -1;
      key[u] = kKeyTree;
    }
    __syncthreads();
  }
}

// Shape and limit checks shared by the entries (before any pointer check); 0 when the shape is served.
int pn_check_shape(const char* who, int B, int N, int k) {
  FPSG_REQUIRE(B > 0, FPSG_E_SHAPE, "%s: B must be positive (got %d)", who, B);
  FPSG_REQUIRE(k >= FPSG_NORMALS_POINTS_MIN_K && k <= FPSG_NORMALS_POINTS_MAX_K, FPSG_E_SHAPE,
               "%s: k must be in %d..%d (got %d)", who, FPSG_NORMALS_POINTS_MIN_K, FPSG_NORMALS_POINTS_MAX_K, k);
  FPSG_REQUIRE(N >= k + 1, FPSG_E_SHAPE, "%s: N must be at least k + 1 (got N=%d, k=%d)", who, N, k);
  return 0;
}
int pn_check_limit(const char* who, int B, int N) {
  FPSG_REQUIRE(N <= FPSG_NORMALS_POINTS_MAX_N && B <= FPSG_NORMALS_POINTS_MAX_B, FPSG_E_LIMIT,
               "%s: N=%d, B=%d exceed the supported maximum of %d points and %d clouds", who, N, B,
               FPSG_NORMALS_POINTS_MAX_N, FPSG_NORMALS_POINTS_MAX_B);
  return 0;
}
inline bool pn_shape_ok(int B, int N, int k) {
  return B > 0 && B <= FPSG_NORMALS_POINTS_MAX_B && k >= FPSG_NORMALS_POINTS_MIN_K && k <= FPSG_NORMALS_POINTS_MAX_K &&
         N >= k + 1 && N <= FPSG_NORMALS_POINTS_MAX_N;
}

}  // namespace
}  // namespace fpsg

extern "C" size_t fpsg_point_normals_workspace_bytes(int B, int N, int k) {
  if (!fpsg::pn_shape_ok(B, N, k)) return 0;
  return (size_t)B * (size_t)N * (size_t)k * sizeof(int32_t);     // the lists, when the caller does not take them
}

extern "C" int fpsg_point_normals(const float* xyz, int B, int N, int k, int sign_mode, const float* ref, float* normals,
                                  float* variation, int32_t* nbr_idx, void* ws, size_t ws_bytes, fpsg_stream_t stream) {
  using namespace fpsg;
  if (const int rc = pn_check_shape("fpsg_point_normals", B, N, k)) return rc;
  FPSG_REQUIRE(sign_mode >= 0 && sign_mode <= 2, FPSG_E_SHAPE, "fpsg_point_normals: sign_mode must be 0, 1 or 2 (got %d)",
               sign_mode);
  if (const int rc = pn_check_limit("fpsg_point_normals", B, N)) return rc;
  FPSG_REQUIRE(ws_bytes >= fpsg_point_normals_workspace_bytes(B, N, k), FPSG_E_SHAPE,
               "fpsg_point_normals: workspace of %zu bytes, %zu needed", ws_bytes,
               fpsg_point_normals_workspace_bytes(B, N, k));
  FPSG_REQUIRE_PTR(xyz); FPSG_REQUIRE_PTR(normals); FPSG_REQUIRE_PTR(ws);
  if (sign_mode != 0) FPSG_REQUIRE_PTR(ref);
  FPSG_REQUIRE(!misaligned4(ref) && !misaligned4(variation) && !misaligned4(nbr_idx), FPSG_E_ALIGN,
               "fpsg_point_normals: 'ref', 'variation' or 'nbr_idx' not 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int32_t* lists = nbr_idx != nullptr ? nbr_idx : static_cast<int32_t*>(ws);
  const dim3 grid((unsigned)((N + kPnThreads - 1) / kPnThreads), (unsigned)B);
  if (k <= 8) hipLaunchKernelGGL(pn_select_kernel<8>, grid, dim3(kPnThreads), 0, s, xyz, N, k, lists);
  else if (k <= 16) hipLaunchKernelGGL(pn_select_kernel<16>, grid, dim3(kPnThreads), 0, s, xyz, N, k, lists);
  else hipLaunchKernelGGL(pn_select_kernel<32>, grid, dim3(kPnThreads), 0, s, xyz, N, k, lists);
  if (const int rc = launch_status("fpsg_point_normals (selection)")) return rc;
  const long long total = (long long)B * N;
  hipLaunchKernelGGL(pn_pca_kernel, dim3((unsigned)((total + kPnPcaThreads - 1) / kPnPcaThreads)), dim3(kPnPcaThreads), 0,
                     s, xyz, lists, N, k, total, sign_mode, ref, normals, variation);
  return launch_status("fpsg_point_normals (pca)");
}

extern "C" size_t fpsg_point_normals_orient_workspace_bytes(int B, int N, int k) {
  if (!fpsg::pn_shape_ok(B, N, k)) return 0;
  return (size_t)B * (size_t)N * (size_t)(k + 2) * sizeof(int32_t);   // counts [B,N], offsets [B,N], reverse lists [B,N k]
}

extern "C" int fpsg_point_normals_orient(const float* xyz, const float* normals_in, const int32_t* nbr_idx, int B, int N,
                                         int k, int axis, float* normals_out, int32_t* parent, void* ws, size_t ws_bytes,
                                         fpsg_stream_t stream) {
  using namespace fpsg;
  if (const int rc = pn_check_shape("fpsg_point_normals_orient", B, N, k)) return rc;
  FPSG_REQUIRE(axis >= 0 && axis <= 2, FPSG_E_SHAPE, "fpsg_point_normals_orient: axis must be 0, 1 or 2 (got %d)", axis);
  if (const int rc = pn_check_limit("fpsg_point_normals_orient", B, N)) return rc;
  FPSG_REQUIRE(ws_bytes >= fpsg_point_normals_orient_workspace_bytes(B, N, k), FPSG_E_SHAPE,
               "fpsg_point_normals_orient: workspace of %zu bytes, %zu needed", ws_bytes,
               fpsg_point_normals_orient_workspace_bytes(B, N, k));
  FPSG_REQUIRE_PTR(xyz); FPSG_REQUIRE_PTR(normals_in); FPSG_REQUIRE_PTR(nbr_idx); FPSG_REQUIRE_PTR(normals_out);
  FPSG_REQUIRE_PTR(ws);
  FPSG_REQUIRE(!misaligned4(parent), FPSG_E_ALIGN, "fpsg_point_normals_orient: 'parent' not 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int32_t* cnt = static_cast<int32_t*>(ws);
  int32_t* off = cnt + (size_t)B * (size_t)N;
  int32_t* rev = off + (size_t)B * (size_t)N;
  const dim3 grid((unsigned)((N + kRvThreads - 1) / kRvThreads), (unsigned)B);
  hipLaunchKernelGGL(pn_reverse_kernel<false>, grid, dim3(kRvThreads), 0, s, nbr_idx, N, k, cnt, off, rev);
  if (const int rc = launch_status("fpsg_point_normals_orient (count)")) return rc;
  hipLaunchKernelGGL(pn_reverse_kernel<true>, grid, dim3(kRvThreads), 0, s, nbr_idx, N, k, cnt, off, rev);
  if (const int rc = launch_status("fpsg_point_normals_orient (fill)")) return rc;
  const size_t lds = orient_lds_bytes(N);
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pn_orient_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { set_error("fpsg_point_normals_orient: %s", hipGetErrorString(e)); return (int)e; }
  }
  hipLaunchKernelGGL(pn_orient_kernel, dim3((unsigned)B), dim3((unsigned)orient_threads(N)), lds, s, xyz, normals_in,
                     nbr_idx, cnt, off, rev, N, k, axis, normals_out, parent);
  return launch_status("fpsg_point_normals_orient (forest)");
}
