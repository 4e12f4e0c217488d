// point_mesh.hip -- K32: the nearest triangle of every point, for gfx950.  The definition is in include/fpsg_hip.h (K32)
// and DESIGN.md: four candidates per (point, face) pair -- the nearest points of the three edges and the plane's foot
// when it lies inside -- and the exact minimum over the faces, the lowest face id on ties.
//
// point_mesh_chunk_kernel: 256 threads, two points per thread in registers, grid (point blocks, mesh, chunk).  The faces
// of the chunk stream through LDS in tiles of 256: while staging, thread t builds the record of face t (corners a and b,
// the three edges, three dots and four reciprocals: the divisions happen once per face and workgroup), and in the inner
// loop every lane reads the same record, so the LDS reads broadcast.  The inner loop has no branch: the interior
// candidate is masked to +inf by a select, a skipped face's record is NaN and never wins.  Each chunk writes one packed
// (dist2 bits << 32 | face) word per point; point_mesh_finish_kernel takes their minimum in ascending chunk order and
// recomputes closest and bary of the winner with the same device functions.  No atomics.
#include "render_common.h"

namespace fpsg {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 256;               // faces per LDS tile: one per thread while staging
constexpr int kPointsPerThread = 2;
constexpr int kPointsPerBlock = kThreads * kPointsPerThread;
constexpr int kRecord = 24;              // floats: a, b, e0, e1, e2, d00, d01, d11, r0, r1, r2, rd, two of padding (96 B)

struct FaceRecord {
  float ax, ay, az, bx, by, bz;
  float e0x, e0y, e0z, e1x, e1y, e1z, e2x, e2y, e2z;
  float d00, d01, d11, r0, r1, r2, rd;
};

__device__ __forceinline__ float dot3(float x0, float x1, float x2, float y0, float y1, float y2) {
  return (x0 * y0 + x1 * y1) + x2 * y2;
}
__device__ __forceinline__ float rc(float x) { return (x > 0.0f && finite_f(x)) ? 1.0f / x : 0.0f; }
__device__ __forceinline__ float clamp01(float t) { return __builtin_fminf(__builtin_fmaxf(t, 0.0f), 1.0f); }

// The record of face f of the mesh P; NaN corners (every candidate's distance NaN: the face never wins) when an index
// is outside [0, V).  Nothing is read through such an index.
__device__ __forceinline__ FaceRecord make_record(const float* __restrict__ P, int V, const int* __restrict__ faces,
                                                  size_t f) {
  FaceRecord R;
  const int ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
  const bool ok = (unsigned)ia < (unsigned)V && (unsigned)ib < (unsigned)V && (unsigned)ic < (unsigned)V;
  const float nan = __uint_as_float(0x7fc00000u);
  const float* a = P + (size_t)(ok ? ia : 0) * 3;
  const float* b = P + (size_t)(ok ? ib : 0) * 3;
  const float* c = P + (size_t)(ok ? ic : 0) * 3;
  R.ax = ok ? a[0] : nan; R.ay = ok ? a[1] : nan; R.az = ok ? a[2] : nan;
  R.bx = ok ? b[0] : nan; R.by = ok ? b[1] : nan; R.bz = ok ? b[2] : nan;
  const float cx = ok ? c[0] : nan, cy = ok ? c[1] : nan, cz = ok ? c[2] : nan;
  R.e0x = R.bx - R.ax; R.e0y = R.by - R.ay; R.e0z = R.bz - R.az;
  R.e1x = cx - R.ax;   R.e1y = cy - R.ay;   R.e1z = cz - R.az;
  R.e2x = cx - R.bx;   R.e2y = cy - R.by;   R.e2z = cz - R.bz;
  R.d00 = dot3(R.e0x, R.e0y, R.e0z, R.e0x, R.e0y, R.e0z);
  R.d01 = dot3(R.e0x, R.e0y, R.e0z, R.e1x, R.e1y, R.e1z);
  R.d11 = dot3(R.e1x, R.e1y, R.e1z, R.e1x, R.e1y, R.e1z);
  const float d22 = dot3(R.e2x, R.e2y, R.e2z, R.e2x, R.e2y, R.e2z);
  const float det = R.d00 * R.d11 - R.d01 * R.d01;
  R.r0 = rc(R.d00); R.r1 = rc(R.d11); R.r2 = rc(d22); R.rd = rc(det);
  return R;
}

// The four candidates of the pair (p, R): their squared distances d[4] (d[3] = +inf when qI is not valid), points q[4][3]
// and parameters (t0, t1, t2, v, w).  Both kernels go through this one function, so their bits agree.
struct PairOut {
  float d[4];
  float q[4][3];
  float t0, t1, t2, v, w;
};

__device__ __forceinline__ float dist2_to(float px, float py, float pz, float qx, float qy, float qz) {
  const float x = px - qx, y = py - qy, z = pz - qz;
  return dot3(x, y, z, x, y, z);
}

__device__ __forceinline__ void pair_candidates(float px, float py, float pz, const FaceRecord& R, PairOut& o) {
  const float apx = px - R.ax, apy = py - R.ay, apz = pz - R.az;
  const float bpx = px - R.bx, bpy = py - R.by, bpz = pz - R.bz;
  const float s0 = dot3(apx, apy, apz, R.e0x, R.e0y, R.e0z);
  const float s1 = dot3(apx, apy, apz, R.e1x, R.e1y, R.e1z);
  const float s2 = dot3(bpx, bpy, bpz, R.e2x, R.e2y, R.e2z);
  o.t0 = clamp01(s0 * R.r0);
  o.t1 = clamp01(s1 * R.r1);
  o.t2 = clamp01(s2 * R.r2);
  o.q[0][0] = R.ax + R.e0x * o.t0; o.q[0][1] = R.ay + R.e0y * o.t0; o.q[0][2] = R.az + R.e0z * o.t0;
  o.q[1][0] = R.ax + R.e1x * o.t1; o.q[1][1] = R.ay + R.e1y * o.t1; o.q[1][2] = R.az + R.e1z * o.t1;
  o.q[2][0] = R.bx + R.e2x * o.t2; o.q[2][1] = R.by + R.e2y * o.t2; o.q[2][2] = R.bz + R.e2z * o.t2;
  o.v = (R.d11 * s0 - R.d01 * s1) * R.rd;
  o.w = (R.d00 * s1 - R.d01 * s0) * R.rd;
  o.q[3][0] = R.ax + (R.e0x * o.v + R.e1x * o.w);
  o.q[3][1] = R.ay + (R.e0y * o.v + R.e1y * o.w);
  o.q[3][2] = R.az + (R.e0z * o.v + R.e1z * o.w);
  const bool valid = (R.rd > 0.0f) & (o.v >= 0.0f) & (o.w >= 0.0f) & (o.v + o.w <= 1.0f);
  for (int k = 0; k < 4; ++k) o.d[k] = dist2_to(px, py, pz, o.q[k][0], o.q[k][1], o.q[k][2]);
  o.d[3] = valid ? o.d[3] : __builtin_inff();
}

__device__ __forceinline__ float pair_value(float px, float py, float pz, const FaceRecord& R) {
  PairOut o;
  pair_candidates(px, py, pz, R, o);
  return __builtin_fminf(__builtin_fminf(__builtin_fminf(o.d[0], o.d[1]), o.d[2]), o.d[3]);
}

__global__ __launch_bounds__(kThreads) void point_mesh_chunk_kernel(const float* __restrict__ points, int N,
                                                                    const float* __restrict__ verts, int V,
                                                                    size_t mesh_stride, const int* __restrict__ faces,
                                                                    int F, int per_chunk,
                                                                    unsigned long long* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float tile[kTile * kRecord];
  const int t = threadIdx.x;
  const int b = blockIdx.y, chunk = blockIdx.z, chunks = gridDim.z;
  const float* P = verts + (size_t)b * mesh_stride;
  const long long f_lo = (long long)chunk * per_chunk;
  const long long f_hi = f_lo + per_chunk < (long long)F ? f_lo + per_chunk : (long long)F;

  const float nan = __uint_as_float(0x7fc00000u);
  float px[kPointsPerThread], py[kPointsPerThread], pz[kPointsPerThread], best[kPointsPerThread];
  int who[kPointsPerThread];
#pragma unroll
  for (int k = 0; k < kPointsPerThread; ++k) {
    const int n = blockIdx.x * kPointsPerBlock + k * kThreads + t;
    const bool in = n < N;
    const float* p = points + ((size_t)b * N + (in ? n : 0)) * 3;
    px[k] = in ? p[0] : nan; py[k] = in ? p[1] : nan; pz[k] = in ? p[2] : nan;
    best[k] = __builtin_inff();
    who[k] = -1;
  }

  for (long long base = f_lo; base < f_hi; base += kTile) {
    const int count = (int)(f_hi - base < kTile ? f_hi - base : kTile);
    __syncthreads();                                   // the previous tile has been read
    if (t < count) {
      const FaceRecord R = make_record(P, V, faces, (size_t)(base + t));
      float* r = tile + t * kRecord;
      *reinterpret_cast<v4f*>(r) = v4f{R.ax, R.ay, R.az, R.bx};
      *reinterpret_cast<v4f*>(r + 4) = v4f{R.by, R.bz, R.e0x, R.e0y};
      *reinterpret_cast<v4f*>(r + 8) = v4f{R.e0z, R.e1x, R.e1y, R.e1z};
      *reinterpret_cast<v4f*>(r + 12) = v4f{R.e2x, R.e2y, R.e2z, R.d00};
      *reinterpret_cast<v4f*>(r + 16) = v4f{R.d01, R.d11, R.r0, R.r1};
      *reinterpret_cast<v4f*>(r + 20) = v4f{R.r2, R.rd, 0.0f, 0.0f};
    }
    __syncthreads();
    for (int j = 0; j < count; ++j) {
      const float* r = tile + j * kRecord;             // the same address in every lane: a broadcast
      const v4f r0 = *reinterpret_cast<const v4f*>(r), r1 = *reinterpret_cast<const v4f*>(r + 4);
      const v4f r2 = *reinterpret_cast<const v4f*>(r + 8), r3 = *reinterpret_cast<const v4f*>(r + 12);
      const v4f r4 = *reinterpret_cast<const v4f*>(r + 16), r5 = *reinterpret_cast<const v4f*>(r + 20);
      FaceRecord R;
      R.ax = r0.x; R.ay = r0.y; R.az = r0.z; R.bx = r0.w; R.by = r1.x; R.bz = r1.y;
      R.e0x = r1.z; R.e0y = r1.w; R.e0z = r2.x; R.e1x = r2.y; R.e1y = r2.z; R.e1z = r2.w;
      R.e2x = r3.x; R.e2y = r3.y; R.e2z = r3.z; R.d00 = r3.w;
      R.d01 = r4.x; R.d11 = r4.y; R.r0 = r4.z; R.r1 = r4.w; R.r2 = r5.x; R.rd = r5.y;
      const int f = (int)base + j;
#pragma unroll
      for (int k = 0; k < kPointsPerThread; ++k) {
        const float m = pair_value(px[k], py[k], pz[k], R);
        const bool win = m < best[k];                  // false for NaN; ascending faces: the lowest id keeps a tie
        best[k] = win ? m : best[k];
        who[k] = win ? f : who[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kPointsPerThread; ++k) {
    const int n = blockIdx.x * kPointsPerBlock + k * kThreads + t;
    if (n < N)
      partial[((size_t)b * N + n) * chunks + chunk] =
          ((unsigned long long)__float_as_uint(best[k]) << 32) | (unsigned)who[k];
  }
}

__global__ __launch_bounds__(kThreads) void point_mesh_finish_kernel(const float* __restrict__ points, long long total,
                                                                     int N, const float* __restrict__ verts, int V,
                                                                     size_t mesh_stride, const int* __restrict__ faces,
                                                                     int F, int chunks,
                                                                     const unsigned long long* __restrict__ partial,
                                                                     float* __restrict__ dist2, int* __restrict__ face,
                                                                     float* __restrict__ closest,
                                                                     float* __restrict__ bary) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;      // b N + n
  if (i >= total) return;
  unsigned long long m = partial[(size_t)i * chunks];
  for (int c = 1; c < chunks; ++c) {
    const unsigned long long o = partial[(size_t)i * chunks + c];
    m = o < m ? o : m;                                 // smaller distance first, then the smaller face id
  }
  const float d = __uint_as_float((unsigned)(m >> 32));
  const int f = (int)(unsigned)(m & 0xffffffffull);
  dist2[i] = d;
  face[i] = f;
  if (closest == nullptr && bary == nullptr) return;
  const float nan = __uint_as_float(0x7fc00000u);
  float q[3] = {nan, nan, nan}, w[3] = {nan, nan, nan};
  if ((unsigned)f < (unsigned)F) {
    const float* P = verts + (size_t)(i / N) * mesh_stride;
    const float* p = points + (size_t)i * 3;
    const FaceRecord R = make_record(P, V, faces, (size_t)f);
    PairOut o;
    pair_candidates(p[0], p[1], p[2], R, o);
    const float least = __builtin_fminf(__builtin_fminf(__builtin_fminf(o.d[0], o.d[1]), o.d[2]), o.d[3]);
    const int k = o.d[0] == least ? 0 : o.d[1] == least ? 1 : o.d[2] == least ? 2 : 3;
#pragma unroll
    for (int x = 0; x < 3; ++x)                        // selects: a run-time index would put the candidates in scratch
      q[x] = k == 0 ? o.q[0][x] : k == 1 ? o.q[1][x] : k == 2 ? o.q[2][x] : o.q[3][x];
    if (k == 0) { w[0] = 1.0f - o.t0; w[1] = o.t0; w[2] = 0.0f; }
    else if (k == 1) { w[0] = 1.0f - o.t1; w[1] = 0.0f; w[2] = o.t1; }
    else if (k == 2) { w[0] = 0.0f; w[1] = 1.0f - o.t2; w[2] = o.t2; }
    else { w[0] = (1.0f - o.v) - o.w; w[1] = o.v; w[2] = o.w; }
  }
  if (closest != nullptr) { closest[i * 3] = q[0]; closest[i * 3 + 1] = q[1]; closest[i * 3 + 2] = q[2]; }
  if (bary != nullptr) { bary[i * 3] = w[0]; bary[i * 3 + 1] = w[1]; bary[i * 3 + 2] = w[2]; }
}

// chunks as the entry resolves it: the caller's when positive; otherwise enough slices for about eight workgroups per
// CU of a 256-CU device, none shorter than kMinChunkFaces.  0 for a refused shape.
constexpr int kMinChunkFaces = 64;
int resolve_chunks(int B, int N, int F, int chunks) {
  if (B < 1 || N < 1 || F < 1) return 0;
  if (N > FPSG_POINT_MESH_MAX_POINTS || B > FPSG_POINT_MESH_MAX_MESHES || F > FPSG_MESH_MAX_FACES ||
      (long long)B * N > FPSG_POINT_MESH_MAX_TOTAL || chunks > FPSG_POINT_MESH_MAX_CHUNKS)
    return 0;
  if (chunks > 0) return chunks;
  const long long blocks = (long long)B * ((N + kPointsPerBlock - 1) / kPointsPerBlock);
  long long want = (2048 + blocks - 1) / blocks;
  const long long most = ((long long)F + kMinChunkFaces - 1) / kMinChunkFaces;
  if (want > most) want = most;
  if (want > FPSG_POINT_MESH_MAX_CHUNKS) want = FPSG_POINT_MESH_MAX_CHUNKS;
  return want < 1 ? 1 : (int)want;
}

}  // namespace
}  // namespace fpsg

extern "C" size_t fpsg_point_mesh_workspace_bytes(int B, int N, int F, int chunks) {
  const int c = fpsg::resolve_chunks(B, N, F, chunks);
  return (size_t)B * (size_t)N * (size_t)c * sizeof(unsigned long long);
}

extern "C" int fpsg_point_mesh_distance(const float* points, int B, int N, const float* verts, int V, int verts_per_mesh,
                                        const int32_t* faces, int F, int chunks, float* dist2, int32_t* face,
                                        float* closest, float* bary, void* ws, size_t ws_bytes, fpsg_stream_t stream) {
  using namespace fpsg;
  FPSG_REQUIRE(B > 0 && N > 0 && V > 0 && F > 0, FPSG_E_SHAPE,
               "fpsg_point_mesh_distance: B,N,V,F must be positive (got %d,%d,%d,%d)", B, N, V, F);
  FPSG_REQUIRE(verts_per_mesh == 0 || verts_per_mesh == 1, FPSG_E_SHAPE,
               "fpsg_point_mesh_distance: verts_per_mesh must be 0 or 1 (got %d)", verts_per_mesh);
  FPSG_REQUIRE(N <= FPSG_POINT_MESH_MAX_POINTS && B <= FPSG_POINT_MESH_MAX_MESHES &&
                   (long long)B * N <= FPSG_POINT_MESH_MAX_TOTAL && V <= FPSG_MESH_MAX_FACES && F <= FPSG_MESH_MAX_FACES &&
                   chunks <= FPSG_POINT_MESH_MAX_CHUNKS,
               FPSG_E_LIMIT,
               "fpsg_point_mesh_distance: N <= %d, B <= %d, B N <= %d, V,F <= %d and chunks <= %d are supported (got "
               "B=%d N=%d V=%d F=%d chunks=%d)",
               FPSG_POINT_MESH_MAX_POINTS, FPSG_POINT_MESH_MAX_MESHES, FPSG_POINT_MESH_MAX_TOTAL, FPSG_MESH_MAX_FACES,
               FPSG_POINT_MESH_MAX_CHUNKS, B, N, V, F, chunks);
  const int c = resolve_chunks(B, N, F, chunks);
  const size_t need = fpsg_point_mesh_workspace_bytes(B, N, F, chunks);
  FPSG_REQUIRE(c > 0 && ws_bytes >= need, FPSG_E_SHAPE,
               "fpsg_point_mesh_distance: workspace of %zu bytes, %zu needed", ws_bytes, need);
  FPSG_REQUIRE_PTR(points); FPSG_REQUIRE_PTR(verts); FPSG_REQUIRE_PTR(faces); FPSG_REQUIRE_PTR(dist2);
  FPSG_REQUIRE_PTR(face); FPSG_REQUIRE_PTR(ws);
  FPSG_REQUIRE(!misaligned4(closest) && !misaligned4(bary), FPSG_E_ALIGN,
               "fpsg_point_mesh_distance: 'closest' or 'bary' not 4-byte aligned");
  FPSG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, FPSG_E_ALIGN,
               "fpsg_point_mesh_distance: 'ws' not 8-byte aligned");
  const size_t mesh_stride = verts_per_mesh ? (size_t)V * 3 : 0;
  const int per_chunk = (F + c - 1) / c;
  unsigned long long* partial = static_cast<unsigned long long*>(ws);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(point_mesh_chunk_kernel,
                     dim3((unsigned)((N + kPointsPerBlock - 1) / kPointsPerBlock), (unsigned)B, (unsigned)c),
                     dim3(kThreads), 0, s, points, N, verts, V, mesh_stride, faces, F, per_chunk, partial);
  const int rc1 = launch_status("fpsg_point_mesh_distance (chunks)");
  if (rc1 != 0) return rc1;
  const long long total = (long long)B * N;
  hipLaunchKernelGGL(point_mesh_finish_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                     points, total, N, verts, V, mesh_stride, faces, F, c, partial, dist2, face, closest, bary);
  return launch_status("fpsg_point_mesh_distance (finish)");
}
