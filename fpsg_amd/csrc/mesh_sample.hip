// mesh_sample.hip -- K26: area-weighted sampling of a triangle mesh's surface, for gfx950.  The definition is in
// include/fpsg_hip.h (K26) and DESIGN.md: fp32 areas without fma, weights quantised to integers against the largest
// area, an integer CDF (any scan order gives the same integers) and one inverse-CDF lookup per sample.
//
// Structure:
//   * mesh_area_kernel: one face per thread -> area [F] fp32 and the largest area (atomicMax on the bits: areas are
//     >= 0, so their bits order as unsigned integers, and an integer maximum does not depend on arrival order);
//   * mesh_scan_block_kernel: 1024 faces per workgroup (4 per thread): q, an inclusive scan in registers / LDS, the
//     workgroup's sum; mesh_scan_sums_kernel: one workgroup turns the sums into exclusive offsets;
//     mesh_scan_add_kernel adds them.  uint64 throughout: F 2^32 <= 2^56;
//   * mesh_sample_kernel: one sample per thread, a binary search over C (log2 F dependent loads that hit L2 for any
//     mesh that fits it), then 9 gathered floats and 3 stores.
#include "fpsg_common.h"

namespace fpsg {
namespace {

typedef unsigned long long u64;

constexpr int kScanT = 256;              // threads of a scan workgroup
constexpr int kScanP = 4;                // faces per thread
constexpr int kScanB = kScanT * kScanP;  // faces per workgroup

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(256) void mesh_area_kernel(const float* __restrict__ verts, int V,
                                                        const int* __restrict__ faces, int F,
                                                        float* __restrict__ area, unsigned* __restrict__ amax_bits) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  float a = 0.0f;
  if (f < F) {
    const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
      const float* A = verts + (size_t)i0 * 3;
      const float* B = verts + (size_t)i1 * 3;
      const float* C = verts + (size_t)i2 * 3;
      const float e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
      const float e2x = C[0] - A[0], e2y = C[1] - A[1], e2z = C[2] - A[2];
      const float nx = e1y * e2z - e1z * e2y;
      const float ny = e1z * e2x - e1x * e2z;
      const float nz = e1x * e2y - e1y * e2x;
      const float s = (nx * nx + ny * ny) + nz * nz;
      a = 0.5f * __builtin_sqrtf(s);
      if (!finite_f(a)) a = 0.0f;                      // NaN and inf: the face has no weight
    }
    area[f] = a;
  }
  // the wave's maximum first (bits of a >= 0), one atomic per wave
  unsigned m = __float_as_uint(a);
  m = max(m, lane_xor<1>(m)); m = max(m, lane_xor<2>(m)); m = max(m, lane_xor<4>(m));
  m = max(m, lane_xor<8>(m)); m = max(m, lane_xor<16>(m)); m = max(m, lane_xor<32>(m));
  if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(amax_bits, m);
}

__device__ __forceinline__ u64 mesh_weight(float a, double amax) {
  // a in [0, amax], amax > 0: the quotient is in [0, 1] and the product in [0, 2^32]
  return (u64)__builtin_rint((double)a / amax * 4294967296.0);
}

__global__ __launch_bounds__(kScanT) void mesh_scan_block_kernel(const float* __restrict__ area, int F,
                                                                 const unsigned* __restrict__ amax_bits,
                                                                 u64* __restrict__ cdf, u64* __restrict__ sums) {
  __shared__ u64 part[kScanT];
  const int tid = threadIdx.x;
  const float amax_f = __uint_as_float(*amax_bits);
  const double amax = (double)amax_f;
  const size_t base = (size_t)blockIdx.x * kScanB + (size_t)tid * kScanP;
  u64 q[kScanP];
  u64 run = 0;
#pragma unroll
  for (int k = 0; k < kScanP; ++k) {
    const size_t f = base + k;
    const float a = f < (size_t)F ? area[f] : 0.0f;
    run += (amax_f > 0.0f && a > 0.0f) ? mesh_weight(a, amax) : 0ull;
    q[k] = run;
  }
  part[tid] = run;
  __syncthreads();
  for (int d = 1; d < kScanT; d <<= 1) {               // Hillis-Steele over the threads' sums (integers: any order)
    const u64 add = tid >= d ? part[tid - d] : 0ull;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  const u64 before = tid ? part[tid - 1] : 0ull;
#pragma unroll
  for (int k = 0; k < kScanP; ++k) {
    const size_t f = base + k;
    if (f < (size_t)F) cdf[f] = before + q[k];
  }
  if (tid == kScanT - 1) sums[blockIdx.x] = part[tid];
}

// one workgroup: sums[b] -> the sum of the blocks before b, in place
__global__ __launch_bounds__(kScanT) void mesh_scan_sums_kernel(u64* __restrict__ sums, int nb) {
  __shared__ u64 part[kScanT];
  const int tid = threadIdx.x;
  u64 carry = 0;
  for (int b0 = 0; b0 < nb; b0 += kScanT) {
    const int b = b0 + tid;
    const u64 own = b < nb ? sums[b] : 0ull;
    part[tid] = own;
    __syncthreads();
    for (int d = 1; d < kScanT; d <<= 1) {
      const u64 add = tid >= d ? part[tid - d] : 0ull;
      __syncthreads();
      part[tid] += add;
      __syncthreads();
    }
    if (b < nb) sums[b] = carry + part[tid] - own;
    carry += part[kScanT - 1];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kScanT) void mesh_scan_add_kernel(u64* __restrict__ cdf, int F,
                                                               const u64* __restrict__ sums) {
  const u64 off = sums[blockIdx.x];
  const size_t base = (size_t)blockIdx.x * kScanB;
#pragma unroll
  for (int k = 0; k < kScanP; ++k) {
    const size_t f = base + (size_t)k * kScanT + threadIdx.x;
    if (f < (size_t)F) cdf[f] += off;
  }
}

__device__ __forceinline__ float unit_clamp(float v) {
  return __builtin_fminf(__builtin_fmaxf(v, 0.0f), 0x1.fffffep-1f);   // NaN -> 0
}

__global__ __launch_bounds__(256) void mesh_sample_kernel(const float* __restrict__ verts, int V,
                                                          const int* __restrict__ faces, int F,
                                                          const u64* __restrict__ cdf, u64 T,
                                                          const float* __restrict__ u, int m,
                                                          float* __restrict__ points, int* __restrict__ face_idx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const float u0 = unit_clamp(u[(size_t)i * 3]);
  const float u1 = unit_clamp(u[(size_t)i * 3 + 1]);
  const float u2 = unit_clamp(u[(size_t)i * 3 + 2]);
  u64 t = (u64)((double)u0 * (double)T);
  t = t < T - 1 ? t : T - 1;
  int lo = 0, hi = F - 1;                              // the first f with C_f > t; never beyond F - 1
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (cdf[mid] > t) hi = mid; else lo = mid + 1;
  }
  // a chosen face has q > 0 and so indices in range; the clamp keeps a call with a foreign cdf inside verts as well
  int i0 = faces[(size_t)lo * 3], i1 = faces[(size_t)lo * 3 + 1], i2 = faces[(size_t)lo * 3 + 2];
  i0 = min(max(i0, 0), V - 1); i1 = min(max(i1, 0), V - 1); i2 = min(max(i2, 0), V - 1);
  const float* A = verts + (size_t)i0 * 3;
  const float* B = verts + (size_t)i1 * 3;
  const float* C = verts + (size_t)i2 * 3;
  const float s = __builtin_sqrtf(u1);
  const float w0 = 1.0f - s, w1 = s * (1.0f - u2), w2 = s * u2;
#pragma unroll
  for (int k = 0; k < 3; ++k) points[(size_t)i * 3 + k] = (w0 * A[k] + w1 * B[k]) + w2 * C[k];
  face_idx[i] = lo;
}

inline int scan_blocks(int F) { return (F + kScanB - 1) / kScanB; }
inline size_t cdf_ws_bytes(int F) { return 8 + (size_t)scan_blocks(F) * 8 + (size_t)F * 4; }

}  // namespace
}  // namespace fpsg

extern "C" size_t fpsg_mesh_cdf_workspace_bytes(int V, int F) {
  if (V < 1 || F < 1 || F > FPSG_MESH_MAX_FACES) return 0;
  return fpsg::cdf_ws_bytes(F);
}

extern "C" int fpsg_mesh_cdf(const float* verts, int V, const int32_t* faces, int F, uint64_t* cdf, void* ws,
                             size_t ws_bytes, fpsg_stream_t stream) {
  using namespace fpsg;
  FPSG_REQUIRE(V > 0 && F > 0, FPSG_E_SHAPE, "fpsg_mesh_cdf: V,F must be positive (got %d,%d)", V, F);
  FPSG_REQUIRE(F <= FPSG_MESH_MAX_FACES, FPSG_E_LIMIT, "fpsg_mesh_cdf: F=%d exceeds the supported maximum of %d", F,
               FPSG_MESH_MAX_FACES);
  FPSG_REQUIRE_PTR(verts); FPSG_REQUIRE_PTR(faces); FPSG_REQUIRE_PTR(cdf); FPSG_REQUIRE_PTR(ws);
  FPSG_REQUIRE((reinterpret_cast<uintptr_t>(cdf) & 7u) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0,
               FPSG_E_ALIGN, "fpsg_mesh_cdf: 'cdf' and 'ws' must be 8-byte aligned");
  FPSG_REQUIRE(ws_bytes >= cdf_ws_bytes(F), FPSG_E_SHAPE, "fpsg_mesh_cdf: workspace of %zu bytes, %zu needed",
               ws_bytes, cdf_ws_bytes(F));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nb = scan_blocks(F);
  unsigned* amax = static_cast<unsigned*>(ws);
  u64* sums = reinterpret_cast<u64*>(static_cast<char*>(ws) + 8);
  float* area = reinterpret_cast<float*>(static_cast<char*>(ws) + 8 + (size_t)nb * 8);
  hipError_t e = hipMemsetAsync(amax, 0, 8, st);
  if (e != hipSuccess) { set_error("fpsg_mesh_cdf: %s", hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL(mesh_area_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, verts, V, faces, F, area,
                     amax);
  hipLaunchKernelGGL(mesh_scan_block_kernel, dim3((unsigned)nb), dim3(kScanT), 0, st, area, F, amax,
                     reinterpret_cast<u64*>(cdf), sums);
  if (nb > 1) {
    hipLaunchKernelGGL(mesh_scan_sums_kernel, dim3(1), dim3(kScanT), 0, st, sums, nb);
    hipLaunchKernelGGL(mesh_scan_add_kernel, dim3((unsigned)nb), dim3(kScanT), 0, st, reinterpret_cast<u64*>(cdf), F,
                       sums);
  }
  return launch_status("fpsg_mesh_cdf");
}

extern "C" int fpsg_mesh_sample(const float* verts, int V, const int32_t* faces, int F, const uint64_t* cdf,
                                uint64_t total, const float* u, int m, float* points, int32_t* face_idx,
                                fpsg_stream_t stream) {
  using namespace fpsg;
  FPSG_REQUIRE(V > 0 && F > 0 && m > 0, FPSG_E_SHAPE, "fpsg_mesh_sample: V,F,m must be positive (got %d,%d,%d)", V, F,
               m);
  FPSG_REQUIRE(F <= FPSG_MESH_MAX_FACES, FPSG_E_LIMIT, "fpsg_mesh_sample: F=%d exceeds the supported maximum of %d",
               F, FPSG_MESH_MAX_FACES);
  FPSG_REQUIRE(total > 0, FPSG_E_SHAPE, "fpsg_mesh_sample: the mesh has no area (every face is degenerate)");
  FPSG_REQUIRE(total <= ((uint64_t)F << 32), FPSG_E_SHAPE, "fpsg_mesh_sample: total is not the last entry of a cdf of %d faces", F);
  FPSG_REQUIRE_PTR(verts); FPSG_REQUIRE_PTR(faces); FPSG_REQUIRE_PTR(cdf); FPSG_REQUIRE_PTR(u);
  FPSG_REQUIRE_PTR(points); FPSG_REQUIRE_PTR(face_idx);
  FPSG_REQUIRE((reinterpret_cast<uintptr_t>(cdf) & 7u) == 0, FPSG_E_ALIGN, "fpsg_mesh_sample: 'cdf' must be 8-byte aligned");
  hipLaunchKernelGGL(mesh_sample_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), verts, V, faces, F, reinterpret_cast<const u64*>(cdf),
                     (u64)total, u, m, points, face_idx);
  return launch_status("fpsg_mesh_sample");
}
