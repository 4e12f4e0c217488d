// occupancy.hip -- K15: the voxel-occupancy grid of a set of clouds (counts, clouds_hit, outside, cells), for the
// Jensen-Shannon divergence between a generated and a reference set, for gfx950.  The definition is in
// include/fpsg_hip.h (K15) and DESIGN.md; every rounding is fixed there, and the kernel reproduces it integer for
// integer.  Integer atomics only, so the results do not depend on launch order, slicing or accumulation.
//
// Structure:
//   * one workgroup of 4 waves per cloud (workgroups stride over the clouds when S exceeds the grid), the cloud in
//     chunks of 256 points, one point per thread;
//   * in LDS: the retained k-range of every (i,j) column (`klo`, one byte per column: the retained nodes of a column
//     are klo .. res-1-klo, the sphere being convex and symmetric; 0xFF = none), built once per workgroup by the
//     integer rule; a bitmap of res^3 bits per cloud, flushed into clouds_hit after the cloud's last chunk;
//   * a point whose rounded node n0 is retained is done in its own lane.  The others are compacted into an LDS
//     list and searched by whole waves, one point per wave at a time, the lanes sharing the point's candidates:
//       1. 64 nodes along the ray from the point (clamped to the grid) to the grid's centre give an upper bound U
//          on the minimum (the innermost one is always retained);
//       2. only columns (i,j) with fl(dx dx) <= U and fl(dy dy) <= U can hold the minimum or a tie, d being monotone
//          in each of its three terms: a window in (i,j) around the point, a superset of those columns, is scanned
//          in 8 x 8 tiles, one column per lane;
//       3. within a column d is strictly monotone in |t_z - k| on either side of t_z, so its minimum is at one of
//          the two retained k nearest t_z: two candidates per column;
//       4. a 64-bit key (d's bits, linear index) is minimised over the wave: the lowest index wins ties.
//     Step 3 needs squares that differ by 1 not to be absorbed by the sum, which holds while |t| <= 256 on every
//     axis; a point beyond that (more than ~18 half extents away at res 28, or overflowed to infinity) is scanned
//     against every retained node, which is the definition itself.
#include "fpsg_common.h"

namespace fpsg {
namespace {

constexpr int kOcThreads = 256;
constexpr int kOcWaves = kOcThreads / 64;
constexpr float kOcNear = 256.0f;                      // |t| bound of the windowed search (see above)
constexpr unsigned long long kOcNoKey = ~0ull;

__device__ __forceinline__ float oc_d(float tx, float ty, float tz, int i, int j, int k) {
  const float dx = tx - (float)i, dy = ty - (float)j, dz = tz - (float)k;
  return (dx * dx + dy * dy) + dz * dz;                // -ffp-contract=off: three products, two sums, no fma
}

// d >= 0 (or +inf): its bit pattern orders like its value; the lowest linear index wins ties
__device__ __forceinline__ unsigned long long oc_key(float d, int lin) {
  return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)lin;
}

__device__ __forceinline__ int oc_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__global__ __launch_bounds__(kOcThreads) void occupancy_kernel(const float* __restrict__ xyz, int S, int N, int r,
                                                              float scale, float centre, float E, float E2,
                                                              int in_sphere, int* __restrict__ counts,
                                                              int* __restrict__ clouds_hit,
                                                              int* __restrict__ outside, int* __restrict__ cells) {
  extern __shared__ __align__(16) unsigned char oc_smem[];
  const int words = (r * r * r + 31) >> 5;
  unsigned* bitmap = reinterpret_cast<unsigned*>(oc_smem);               // [words] cells this cloud has hit
  unsigned char* klo = reinterpret_cast<unsigned char*>(bitmap + words);  // [r r] first retained k of column (i,j)
  __shared__ float fb_t[kOcThreads][3];                                  // points that need the search: t
  __shared__ int fb_slot[kOcThreads];                                    //   and their thread in the chunk
  __shared__ int cellbuf[kOcThreads];
  __shared__ int fb_count;
  __shared__ int out_sum[3];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rm1 = r - 1;
  const float rm1f = (float)rm1;

  for (int w = tid; w < words; w += kOcThreads) bitmap[w] = 0u;
  for (int col = tid; col < r * r; col += kOcThreads) {
    int kl = 0;
    if (in_sphere) {
      const int a = 2 * (col / r) - rm1, b = 2 * (col % r) - rm1;
      const int rem = rm1 * rm1 - a * a - b * b;
      kl = 0xFF;
      for (int k = 0; k < r; ++k) {
        const int cc = 2 * k - rm1;
        if (cc * cc <= rem) { kl = k; break; }
      }
    }
    klo[col] = (unsigned char)kl;
  }
  if (tid == 0) fb_count = 0;
  if (tid < 3) out_sum[tid] = 0;
  __syncthreads();

  int o0 = 0, o1 = 0, o2 = 0;
  for (int cloud = blockIdx.x; cloud < S; cloud += gridDim.x) {
    const size_t first = (size_t)cloud * (size_t)N;
    for (long long base = 0; base < N; base += kOcThreads) {
      const long long pt = base + tid;
      // own lane: t, the rounded node, and whether it is retained
      int cell = -1;
      if (pt < N) {
        const float* p = xyz + (first + (size_t)pt) * 3;
        const float x = p[0], y = p[1], z = p[2];
        const float inf = __builtin_inff();
        if (__builtin_fabsf(x) < inf && __builtin_fabsf(y) < inf && __builtin_fabsf(z) < inf) {
          o0 += (__builtin_fabsf(x) > E || __builtin_fabsf(y) > E || __builtin_fabsf(z) > E) ? 1 : 0;
          o1 += ((x * x + y * y) + z * z > E2) ? 1 : 0;
          const float tx = x * scale + centre, ty = y * scale + centre, tz = z * scale + centre;
          const int ix = (int)__builtin_fminf(__builtin_fmaxf(__builtin_rintf(tx), 0.0f), rm1f);
          const int iy = (int)__builtin_fminf(__builtin_fmaxf(__builtin_rintf(ty), 0.0f), rm1f);
          const int iz = (int)__builtin_fminf(__builtin_fmaxf(__builtin_rintf(tz), 0.0f), rm1f);
          const int kl = klo[ix * r + iy];
          if (iz >= kl && iz <= rm1 - kl) {
            cell = (ix * r + iy) * r + iz;
          } else {
            const int e = atomicAdd(&fb_count, 1);     // the order of the list does not matter: a cell per point
            fb_t[e][0] = tx; fb_t[e][1] = ty; fb_t[e][2] = tz;
            fb_slot[e] = tid;
          }
        } else {
          ++o2;
        }
      }
      cellbuf[tid] = cell;
      __syncthreads();

      // the listed points: one wave per point, the lanes share its candidates
      const int listed = fb_count;
      for (int e = wave; e < listed; e += kOcWaves) {
        const float tx = fb_t[e][0], ty = fb_t[e][1], tz = fb_t[e][2];
        unsigned long long best = kOcNoKey;
        if (__builtin_fabsf(tx) <= kOcNear && __builtin_fabsf(ty) <= kOcNear && __builtin_fabsf(tz) <= kOcNear) {
          // 1. nodes along the ray to the centre: an upper bound U of the minimum
          const float sl = (float)(64 - lane) * (1.0f / 64.0f);
          const float ux = __builtin_fminf(__builtin_fmaxf(tx, 0.0f), rm1f) - centre;
          const float uy = __builtin_fminf(__builtin_fmaxf(ty, 0.0f), rm1f) - centre;
          const float uz = __builtin_fminf(__builtin_fmaxf(tz, 0.0f), rm1f) - centre;
          const int ci = oc_clampi((int)__builtin_rintf(centre + ux * sl), 0, rm1);
          const int cj = oc_clampi((int)__builtin_rintf(centre + uy * sl), 0, rm1);
          const int ck = oc_clampi((int)__builtin_rintf(centre + uz * sl), 0, rm1);
          const int ckl = klo[ci * r + cj];
          if (ck >= ckl && ck <= rm1 - ckl) best = oc_key(oc_d(tx, ty, tz, ci, cj, ck), (ci * r + cj) * r + ck);
          best = wave_min_u64(best);
          const float U = __uint_as_float((unsigned)(best >> 32));   // +NaN pattern if none (never): window = grid
          // 2. the window of columns that can hold a node with d <= U (a superset: one node of margin)
          const float sU = __builtin_sqrtf(U);
          int ilo = 0, ihi = rm1, jlo = 0, jhi = rm1;
          if (sU < __builtin_inff()) {                 // false for a NaN too
            ilo = (int)__builtin_fminf(__builtin_fmaxf(__builtin_floorf(tx - sU), 0.0f), rm1f);
            ihi = (int)__builtin_fminf(__builtin_fmaxf(__builtin_ceilf(tx + sU), 0.0f), rm1f);
            jlo = (int)__builtin_fminf(__builtin_fmaxf(__builtin_floorf(ty - sU), 0.0f), rm1f);
            jhi = (int)__builtin_fminf(__builtin_fmaxf(__builtin_ceilf(ty + sU), 0.0f), rm1f);
          }
          ilo = __builtin_amdgcn_readfirstlane(ilo); ihi = __builtin_amdgcn_readfirstlane(ihi);
          jlo = __builtin_amdgcn_readfirstlane(jlo); jhi = __builtin_amdgcn_readfirstlane(jhi);
          const int fz = (int)__builtin_floorf(tz);
          // 3. two candidates per column, one column per lane
          for (int ti = ilo; ti <= ihi; ti += 8) {
            for (int tj = jlo; tj <= jhi; tj += 8) {
              const int i = ti + (lane >> 3), j = tj + (lane & 7);
              if (i <= ihi && j <= jhi) {
                const int kl = klo[i * r + j];
                if (kl != 0xFF) {
                  const int kh = rm1 - kl;
                  const int k1 = oc_clampi(fz, kl, kh), k2 = oc_clampi(fz + 1, kl, kh);
                  const int lin = (i * r + j) * r;
                  const unsigned long long a = oc_key(oc_d(tx, ty, tz, i, j, k1), lin + k1);
                  const unsigned long long b = oc_key(oc_d(tx, ty, tz, i, j, k2), lin + k2);
                  best = a < best ? a : best;
                  best = b < best ? b : best;
                }
              }
            }
          }
        } else {
          // far away or overflowed: every retained node, as the definition says (distances may tie by absorption)
          for (int col = lane; col < r * r; col += 64) {
            const int kl = klo[col];
            if (kl == 0xFF) continue;
            const int i = col / r, j = col - i * r;
            for (int k = kl; k <= rm1 - kl; ++k) {
              const unsigned long long a = oc_key(oc_d(tx, ty, tz, i, j, k), col * r + k);
              best = a < best ? a : best;
            }
          }
        }
        best = wave_min_u64(best);
        if (lane == 0) cellbuf[fb_slot[e]] = (int)(unsigned)best;       // always a retained node: see step 1
      }
      __syncthreads();

      if (tid == 0) fb_count = 0;                      // read above, before the barrier
      if (pt < N) {
        cell = cellbuf[tid];
        if (cells) cells[first + (size_t)pt] = cell;
        if (cell >= 0) {
          atomicAdd(&counts[cell], 1);
          atomicOr(&bitmap[cell >> 5], 1u << (cell & 31));
        }
      }
      __syncthreads();
    }
    // the cloud's bitmap -> clouds_hit, and clear it for the next cloud
    for (int w = tid; w < words; w += kOcThreads) {
      unsigned bits = bitmap[w];
      bitmap[w] = 0u;
      while (bits) {
        const int b = __builtin_ctz(bits);
        bits &= bits - 1;
        atomicAdd(&clouds_hit[w * 32 + b], 1);
      }
    }
    __syncthreads();
  }

  if (o0) atomicAdd(&out_sum[0], o0);
  if (o1) atomicAdd(&out_sum[1], o1);
  if (o2) atomicAdd(&out_sum[2], o2);
  __syncthreads();
  if (tid < 3 && out_sum[tid]) atomicAdd(&outside[tid], out_sum[tid]);
}

}  // namespace
}  // namespace fpsg

extern "C" size_t fpsg_occupancy_grid_workspace_bytes(int S, int N, int res) {
  return 0;                                            // everything transient lives in LDS
}

extern "C" int fpsg_occupancy_grid(const float* xyz, int S, int N, int res, float half_extent, int in_sphere,
                                   int32_t* counts, int32_t* clouds_hit, int32_t* outside, int32_t* cells, void* ws,
                                   size_t ws_bytes, fpsg_stream_t stream) {
  using namespace fpsg;
  FPSG_REQUIRE(S > 0 && N > 0, FPSG_E_SHAPE, "fpsg_occupancy_grid: S,N must be positive (got %d,%d)", S, N);
  FPSG_REQUIRE(res >= 2, FPSG_E_SHAPE, "fpsg_occupancy_grid: res must be at least 2 (got %d)", res);
  FPSG_REQUIRE(!(in_sphere && res == 2), FPSG_E_SHAPE,
               "fpsg_occupancy_grid: in_sphere retains no node at res 2; res must be at least 3");
  FPSG_REQUIRE(res <= FPSG_OCCUPANCY_MAX_RES, FPSG_E_LIMIT,
               "fpsg_occupancy_grid: res=%d exceeds the supported maximum of %d", res, FPSG_OCCUPANCY_MAX_RES);
  FPSG_REQUIRE(half_extent > 0.0f && half_extent < __builtin_inff(), FPSG_E_SHAPE,
               "fpsg_occupancy_grid: half_extent must be positive and finite (got %g)", (double)half_extent);
  const float scale = (float)((double)(res - 1) / (2.0 * (double)half_extent));
  const float centre = (float)((double)(res - 1) / 2.0);
  FPSG_REQUIRE(scale < __builtin_inff(), FPSG_E_SHAPE,
               "fpsg_occupancy_grid: half_extent %g is too small: (res-1) / (2 half_extent) overflows",
               (double)half_extent);
  FPSG_REQUIRE_PTR(xyz); FPSG_REQUIRE_PTR(counts); FPSG_REQUIRE_PTR(clouds_hit); FPSG_REQUIRE_PTR(outside);
  FPSG_REQUIRE(!misaligned4(cells), FPSG_E_ALIGN, "fpsg_occupancy_grid: 'cells' not 4-byte aligned");
  const int words = (res * res * res + 31) >> 5;
  const size_t lds = (size_t)words * 4 + (((size_t)res * res + 15) & ~(size_t)15);
  const int grid = S < 4096 ? S : 4096;                // workgroups stride over the clouds beyond that
  hipLaunchKernelGGL(occupancy_kernel, dim3((unsigned)grid), dim3(kOcThreads), lds,
                     static_cast<hipStream_t>(stream), xyz, S, N, res, scale, centre, half_extent,
                     half_extent * half_extent, in_sphere ? 1 : 0, counts, clouds_hit, outside, cells);
  return launch_status("fpsg_occupancy_grid");
}
