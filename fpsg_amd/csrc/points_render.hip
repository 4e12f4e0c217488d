// points_render.hip -- K29: orthographic Phong views of point clouds, every point a small sphere, for gfx950.  The
// definition is in include/fpsg_hip.h (K29) and DESIGN.md: K27's projection and snap per point, coverage by an integer
// circle test, the sphere's depth per sample, a 64-bit (depth, point) minimum per sample, K27's resolve.  The light's
// terms, the colours and the resolve are render_common.h's, the ones the mesh renderers run.
//
// Structure: the z-buffer never leaves the chip.
//   * points_project_kernel: one (cloud, view, point) per thread -> one 16-byte record (X, Y, depth bits, colour and
//     a valid flag) in the workspace;
//   * points_tile_kernel: one workgroup per (cloud, view, tile of 32 x 32 samples).  The tile's 1024 keys live in LDS.
//     The workgroup walks the cloud's records, one per thread and step; a ballot gives each wave the records whose box
//     meets the tile, and for each of them the wave's lanes stride over box and tile and take the 64-bit minimum in
//     LDS.  Behind a barrier the same workgroup shades the winners into LDS, resolves the tile's output pixels in the
//     defined order and writes all four outputs with plain stores: no global atomics, no clear pass, and the minimum
//     makes the result independent of the order in which waves arrive.
#include "render_common.h"

namespace fpsg {
namespace {

typedef unsigned long long u64;

constexpr int kTile = 32;                // samples per tile side: a multiple of every ssaa
constexpr int kTileSamples = kTile * kTile;
constexpr int kThreads = 256;
constexpr u64 kEmpty = ~0ull;
constexpr int kValid = 1 << 24;          // in a record's fourth word, above the packed colour

__global__ __launch_bounds__(256) void points_project_kernel(const float* __restrict__ points,
                                                             const unsigned char* __restrict__ colors, int N,
                                                             const float* __restrict__ views, int n_views,
                                                             float ortho_scale, int W, int H, v4i* __restrict__ rec) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const unsigned bv = blockIdx.y, b = bv / (unsigned)n_views, view = bv % (unsigned)n_views;
  const size_t src = (size_t)b * N + n;
  float x, y, d;
  int X, Y;
  const bool ok = project_point(points + src * 3, views + (size_t)view * 12, ortho_scale, W, H, x, y, d, X, Y);
  int rgb = 0;
  if (colors) rgb = (int)colors[src * 3] | ((int)colors[src * 3 + 1] << 8) | ((int)colors[src * 3 + 2] << 16);
  rec[(size_t)bv * N + n] = v4i{X, Y, (int)__float_as_uint(d), rgb | (ok ? kValid : 0)};
}

// The sphere of a record at the sample centre (px, py): covered iff q < R2; c = sqrt(1 - q / R2).  Inside a point's box
// |dx|, |dy| <= R <= 2^14, so q < 2^29 and the definition's int64 arithmetic is exact in 32 bits.
__device__ __forceinline__ bool sphere_at(int X, int Y, int px, int py, int R2, float fR2, int& dx, int& dy, float& c) {
  dx = px - X;
  dy = py - Y;
  const int q = dx * dx + dy * dy;
  const float t = (float)q / fR2;
  c = __builtin_sqrtf(1.0f - t);
  return q < R2;
}

template <bool COLORS>
__global__ __launch_bounds__(256) void points_tile_kernel(const v4i* __restrict__ rec, int N, int W, int H, int ssaa,
                                                          int R, float radius, MaterialParams Q,
                                                          const unsigned char* __restrict__ bg_img,
                                                          unsigned char* __restrict__ image,
                                                          float* __restrict__ radiance, int* __restrict__ point_id,
                                                          float* __restrict__ depth) {
  __shared__ u64 keys[kTileSamples];
  __shared__ float col[3][kTileSamples];
  const RenderParams& P = Q.base;
  const int tid = threadIdx.x, lane = tid & 63;
  const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
  const int tx1 = min(tx0 + kTile, W) - 1, ty1 = min(ty0 + kTile, H) - 1;      // inclusive, inside the image
  const size_t bv = blockIdx.z;
  const v4i* recs = rec + bv * N;
  const int R2 = R * R;                                                        // R <= 2^14
  const float fR2 = (float)R2, fR = (float)R;

  for (int s = tid; s < kTileSamples; s += kThreads) keys[s] = kEmpty;
  __syncthreads();

  for (int base = 0; base < N; base += kThreads) {
    const int n = base + tid;
    v4i r = v4i{0, 0, 0, 0};
    if (n < N) r = recs[n];
    // samples whose centre 256 i + 128 lies in [X - R, X + R], clipped to the tile (>> of a negative int: floor)
    const int i0 = max((r.x - R + 127) >> 8, tx0), i1 = min((r.x + R - 128) >> 8, tx1);
    const int j0 = max((r.y - R + 127) >> 8, ty0), j1 = min((r.y + R - 128) >> 8, ty1);
    const bool meets = (r.w & kValid) && i0 <= i1 && j0 <= j1;
    u64 live = __ballot(meets);
    while (live) {                                                             // wave-uniform
      const int src = __builtin_ctzll(live);
      live &= live - 1;
      const int X = __builtin_amdgcn_readlane(r.x, src), Y = __builtin_amdgcn_readlane(r.y, src);
      const float z = __uint_as_float((unsigned)__builtin_amdgcn_readlane(r.z, src));
      const int a0 = __builtin_amdgcn_readlane(i0, src), a1 = __builtin_amdgcn_readlane(i1, src);
      const int b0 = __builtin_amdgcn_readlane(j0, src), b1 = __builtin_amdgcn_readlane(j1, src);
      const unsigned index = (unsigned)(base + (tid & ~63) + src);
      const int bw = a1 - a0 + 1, npix = bw * (b1 - b0 + 1);                   // at most 32 x 32
      for (int p = lane; p < npix; p += 64) {
        const int i = a0 + p % bw, j = b0 + p / bw;
        int dx, dy;
        float c;
        if (!sphere_at(X, Y, 256 * i + 128, 256 * j + 128, R2, fR2, dx, dy, c)) continue;
        const float zs = z - radius * c;
        if (!finite_f(zs)) continue;
        // i in [tx0, tx1], j in [ty0, ty1]: the index is inside the tile
        atomicMin(&keys[(j - ty0) * kTile + (i - tx0)], ((u64)depth_key(zs) << 32) | index);
      }
    }
  }
  __syncthreads();

  const size_t plane = (size_t)W * H;
  for (int s = tid; s < kTileSamples; s += kThreads) {
    const int i = tx0 + (s & (kTile - 1)), j = ty0 + s / kTile;
    if (i >= W || j >= H) continue;
    const u64 key = keys[s];
    const bool hit = key != kEmpty;
    const size_t pix = bv * plane + (size_t)j * W + i;
    if (point_id) point_id[pix] = hit ? (int)(unsigned)key : -1;
    if (depth) depth[pix] = hit ? key_depth((unsigned)(key >> 32)) : __builtin_inff();
    if (!hit) continue;
    const v4i r = recs[(unsigned)key];                                         // written above: an index below N
    int dx, dy;
    float c;
    sphere_at(r.x, r.y, 256 * i + 128, 256 * j + 128, R2, fR2, dx, dy, c);
    const float nx = (float)dx / fR, ny = -((float)dy / fR), nz = -c;
    float diff, spec;
    light_terms(P, nx, ny, nz, diff, spec);
    if (COLORS)
      phong_color(Q, (float)(r.w & 255) / 255.0f, (float)((r.w >> 8) & 255) / 255.0f,
                  (float)((r.w >> 16) & 255) / 255.0f, diff, spec, col[0][s], col[1][s], col[2][s]);
    else
      phong_color(P, diff, spec, col[0][s], col[1][s], col[2][s]);
  }
  if (!image && !radiance) return;                                             // uniform
  __syncthreads();

  const int ow = W / ssaa, oh = H / ssaa, side = kTile / ssaa;                 // ssaa divides 32, W and H
  for (int o = tid; o < side * side; o += kThreads) {
    const int lx = o % side, ly = o / side;
    const int ox = tx0 / ssaa + lx, oy = ty0 / ssaa + ly;
    if (ox >= ow || oy >= oh) continue;
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
    int covered = 0;
    for (int sy = 0; sy < ssaa; ++sy) {
      for (int sx = 0; sx < ssaa; ++sx) {
        const int s = (ly * ssaa + sy) * kTile + lx * ssaa + sx;
        if (keys[s] == kEmpty) continue;
        acc0 += col[0][s]; acc1 += col[1][s]; acc2 += col[2][s];
        ++covered;
      }
    }
    resolve_pixel(acc0, acc1, acc2, covered, ssaa, P, bg_img, (size_t)oy * ow + ox, ((bv * oh + oy) * ow + ox) * 3,
                  radiance, image);
  }
}

inline bool points_shape_ok(int B, int N, int NV, int W, int H, int ssaa) {
  return B > 0 && N > 0 && NV > 0 && W > 0 && H > 0 && (ssaa == 1 || ssaa == 2 || ssaa == 4) && W % ssaa == 0 &&
         H % ssaa == 0;
}
inline bool points_limit_ok(int B, int N, int NV, int W, int H) {
  return N <= FPSG_POINTS_MAX_N && W <= FPSG_RENDER_MAX_SIZE && H <= FPSG_RENDER_MAX_SIZE &&
         NV <= FPSG_RENDER_MAX_VIEWS && (uint64_t)B * (uint64_t)NV < 65536ull;
}

}  // namespace
}  // namespace fpsg

extern "C" size_t fpsg_points_render_workspace_bytes(int B, int N, int n_views, int W, int H) {
  using namespace fpsg;
  if (!points_shape_ok(B, N, n_views, W, H, 1) || !points_limit_ok(B, N, n_views, W, H)) return 0;
  return (size_t)16 * B * n_views * N;
}

extern "C" int fpsg_points_render(const float* points, const uint8_t* colors, int B, int N, const float* views,
                                  int n_views, int W, int H, int ssaa, float ortho_scale, float radius,
                                  const float* params, int log2_shininess, const uint8_t* bg_image, uint8_t* image,
                                  float* radiance, int32_t* point_id, float* depth, void* ws, size_t ws_bytes,
                                  fpsg_stream_t stream) {
  using namespace fpsg;
  static_assert(FPSG_RENDER_MAX_SSAA == 4, "the tile is a whole number of output pixels for ssaa 1, 2 and 4");
  FPSG_REQUIRE(points_shape_ok(B, N, n_views, W, H, ssaa), FPSG_E_SHAPE,
               "fpsg_points_render: B,N,n_views,W,H must be positive, ssaa 1, 2 or 4 and a divisor of W and H (got "
               "%d,%d,%d,%d,%d,%d)", B, N, n_views, W, H, ssaa);
  FPSG_REQUIRE(ortho_scale > 0.0f && ortho_scale <= 3.0e38f, FPSG_E_SHAPE,
               "fpsg_points_render: ortho_scale must be positive and finite");
  FPSG_REQUIRE(radius > 0.0f && radius <= 3.0e38f, FPSG_E_SHAPE,
               "fpsg_points_render: radius must be positive and finite");
  // the radius in snapped units (1/256 sample pixel), formed in double
  const double Rd = 256.0 * ((double)radius / (double)ortho_scale) * (double)(W > H ? W : H);
  const long long R64 = (Rd >= 0.0 && Rd <= 1.0e9) ? __builtin_llrint(Rd) : -1;
  FPSG_REQUIRE(R64 >= 1 && R64 <= 256 * FPSG_POINTS_MAX_RADIUS_PX, FPSG_E_SHAPE,
               "fpsg_points_render: a radius of %g sample pixels, from 1/256 to %d are supported", Rd / 256.0,
               FPSG_POINTS_MAX_RADIUS_PX);
  const int R = (int)R64;
  FPSG_REQUIRE(log2_shininess >= 0 && log2_shininess <= FPSG_RENDER_MAX_LOG2_SHININESS, FPSG_E_SHAPE,
               "fpsg_points_render: log2_shininess must be from 0 to %d (got %d)", FPSG_RENDER_MAX_LOG2_SHININESS,
               log2_shininess);
  FPSG_REQUIRE(points_limit_ok(B, N, n_views, W, H), FPSG_E_LIMIT,
               "fpsg_points_render: N <= %d, W,H <= %d, n_views <= %d and B n_views < 65536 are supported (got "
               "%d,%d,%d,%d,%d)", FPSG_POINTS_MAX_N, FPSG_RENDER_MAX_SIZE, FPSG_RENDER_MAX_VIEWS, N, W, H, n_views, B);
  FPSG_REQUIRE_PTR(points); FPSG_REQUIRE_PTR(views); FPSG_REQUIRE_PTR(ws);
  FPSG_REQUIRE(params != nullptr, FPSG_E_NULL, "fpsg_points_render: null pointer 'params'");
  FPSG_REQUIRE(image || radiance || point_id || depth, FPSG_E_NULL, "fpsg_points_render: no output requested");
  FPSG_REQUIRE(!misaligned4(radiance) && !misaligned4(point_id) && !misaligned4(depth), FPSG_E_ALIGN,
               "fpsg_points_render: an output is not 4-byte aligned");
  FPSG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15u) == 0, FPSG_E_ALIGN,
               "fpsg_points_render: 'ws' must be 16-byte aligned");
  const size_t need = (size_t)16 * B * n_views * N;
  FPSG_REQUIRE(ws_bytes >= need, FPSG_E_SHAPE, "fpsg_points_render: workspace of %zu bytes, %zu needed", ws_bytes,
               need);
  MaterialParams Q;
  unpack_material_params(params, log2_shininess, Q);
  hipStream_t st = static_cast<hipStream_t>(stream);
  v4i* rec = static_cast<v4i*>(ws);
  const unsigned bv = (unsigned)B * (unsigned)n_views;                         // below 65536: a grid's y and z take it
  hipLaunchKernelGGL(points_project_kernel, dim3((unsigned)((N + 255) / 256), bv), dim3(256), 0, st, points, colors, N,
                     views, n_views, ortho_scale, W, H, rec);
  const dim3 grid((unsigned)((W + kTile - 1) / kTile), (unsigned)((H + kTile - 1) / kTile), bv);
  if (colors)
    hipLaunchKernelGGL(points_tile_kernel<true>, grid, dim3(kThreads), 0, st, rec, N, W, H, ssaa, R, radius, Q,
                       bg_image, image, radiance, point_id, depth);
  else
    hipLaunchKernelGGL(points_tile_kernel<false>, grid, dim3(kThreads), 0, st, rec, N, W, H, ssaa, R, radius, Q,
                       bg_image, image, radiance, point_id, depth);
  return launch_status("fpsg_points_render");
}
