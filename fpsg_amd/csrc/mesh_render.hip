// mesh_render.hip -- K27: orthographic, flat-shaded Phong views of a triangle mesh, for gfx950.  The definition is in
// include/fpsg_hip.h (K27) and DESIGN.md: vertices snapped to 1/256 pixel, coverage by int64 edge functions with the
// top-left rule, a 64-bit (depth, face) z-buffer filled with atomicMin, so the image does not depend on launch order.
//
// Structure, all views of a mesh in one launch of each kernel:
//   * render_project_kernel: one (vertex, view) per thread -> camera-space (x, y, depth) and the snapped (X, Y);
//   * render_raster_kernel: one (face, view) per thread; a bounding box of at most kSmallBox pixel centres is drawn by
//     the thread, a larger one is appended to a list;
//   * render_raster_large_kernel: a fixed grid strides over the list's entries, kChunks waves each, lanes over the
//     bounding box's pixels;
//   * render_shade_kernel<FLAT>: one output pixel per thread: its ssaa^2 samples shaded and composited over the
//     background.
// K28 (fpsg_mesh_render_materials) and K31b (fpsg_mesh_render_smooth) are the same entry (render_entry), the same three
// kernels and two more instantiations of the shade kernel.  MATERIALS: a base colour per face, a material's Kd or its
// texture looked up at the sample's interpolated uv.  SMOOTH: that, with the light's terms taken from a normal
// interpolated between the face's three corner normals in place of the face's own.  The light's terms, the colours and
// the resolve are render_common.h's, shared with K29.
#include "render_common.h"

namespace fpsg {
namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int kSmallBox = 64;            // pixel centres a single thread still draws
constexpr int kChunks = 16;              // waves that share one large triangle
constexpr u64 kEmpty = ~0ull;

__global__ __launch_bounds__(256) void render_project_kernel(const float* __restrict__ verts, int V,
                                                             const float* __restrict__ views, float ortho_scale,
                                                             int W, int H, v4f* __restrict__ cam,
                                                             v4i* __restrict__ snapped) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  float x, y, d;
  int X, Y;
  const bool ok = project_point(verts + (size_t)v * 3, views + (size_t)blockIdx.y * 12, ortho_scale, W, H, x, y, d, X, Y);
  const size_t o = (size_t)blockIdx.y * V + v;
  cam[o] = v4f{x, y, d, 0.0f};
  snapped[o] = v4i{X, Y, ok ? 1 : 0, 0};
}

// A face of one view ready to draw: winding normalised (A2 > 0), bounding box clipped to the image.
struct Tri {
  int x0, y0, x1, y1, x2, y2;
  float z0, z1, z2;
  i64 A2;
  int b0, b1, b2;                        // 0 for an edge that owns its boundary (top or left), 1 otherwise
  int i0, i1, j0, j1;                    // pixel range, inclusive; empty when i1 < i0 or j1 < j0
};

__device__ __forceinline__ int edge_bias(int ax, int ay, int bx, int by) {
  const int dx = bx - ax, dy = by - ay;
  return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
}

__device__ __forceinline__ bool tri_setup(const int* __restrict__ faces, int f, int V, const v4f* __restrict__ cam,
                                          const v4i* __restrict__ snapped, int W, int H, Tri& t) {
  const int a = faces[(size_t)f * 3], b = faces[(size_t)f * 3 + 1], c = faces[(size_t)f * 3 + 2];
  if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) return false;
  const v4i sa = snapped[a], sb = snapped[b], sc = snapped[c];
  if (!(sa.z & sb.z & sc.z)) return false;
  t.x0 = sa.x; t.y0 = sa.y; t.z0 = cam[a].z;
  t.x1 = sb.x; t.y1 = sb.y; t.z1 = cam[b].z;
  t.x2 = sc.x; t.y2 = sc.y; t.z2 = cam[c].z;
  t.A2 = (i64)(t.x1 - t.x0) * (i64)(t.y2 - t.y0) - (i64)(t.y1 - t.y0) * (i64)(t.x2 - t.x0);
  if (t.A2 == 0) return false;
  if (t.A2 < 0) {                                      // both windings are drawn
    int s = t.x1; t.x1 = t.x2; t.x2 = s;
    s = t.y1; t.y1 = t.y2; t.y2 = s;
    const float z = t.z1; t.z1 = t.z2; t.z2 = z;
    t.A2 = -t.A2;
  }
  t.b0 = edge_bias(t.x1, t.y1, t.x2, t.y2);
  t.b1 = edge_bias(t.x2, t.y2, t.x0, t.y0);
  t.b2 = edge_bias(t.x0, t.y0, t.x1, t.y1);
  const int xmin = min(t.x0, min(t.x1, t.x2)), xmax = max(t.x0, max(t.x1, t.x2));
  const int ymin = min(t.y0, min(t.y1, t.y2)), ymax = max(t.y0, max(t.y1, t.y2));
  // pixel i has its centre at 256 i + 128 (>> on a negative int is an arithmetic shift: floor)
  t.i0 = max((xmin + 127) >> 8, 0); t.i1 = min((xmax - 128) >> 8, W - 1);
  t.j0 = max((ymin + 127) >> 8, 0); t.j1 = min((ymax - 128) >> 8, H - 1);
  return t.i0 <= t.i1 && t.j0 <= t.j1;
}

__device__ __forceinline__ i64 edge_fn(int ax, int ay, int bx, int by, int px, int py) {
  return (i64)(bx - ax) * (i64)(py - ay) - (i64)(by - ay) * (i64)(px - ax);
}

// i in [0, W), j in [0, H) by the clipped bounding box: the z-buffer index is in range
__device__ __forceinline__ void tri_pixel(const Tri& t, int i, int j, unsigned face, u64* __restrict__ zrow0, int W) {
  const int px = 256 * i + 128, py = 256 * j + 128;
  const i64 E0 = edge_fn(t.x1, t.y1, t.x2, t.y2, px, py);
  const i64 E1 = edge_fn(t.x2, t.y2, t.x0, t.y0, px, py);
  const i64 E2 = edge_fn(t.x0, t.y0, t.x1, t.y1, px, py);
  if (E0 < t.b0 || E1 < t.b1 || E2 < t.b2) return;
  const float A = (float)t.A2;
  const float l0 = (float)E0 / A, l1 = (float)E1 / A, l2 = (float)E2 / A;
  const float z = (l0 * t.z0 + l1 * t.z1) + l2 * t.z2;
  if (!finite_f(z)) return;
  atomicMin(zrow0 + (size_t)j * W + i, ((u64)depth_key(z) << 32) | face);
}

__global__ __launch_bounds__(256) void render_raster_kernel(const int* __restrict__ faces, int F, int V,
                                                            const v4f* __restrict__ cam,
                                                            const v4i* __restrict__ snapped, int W, int H,
                                                            u64* __restrict__ zbuf, unsigned* __restrict__ large,
                                                            unsigned* __restrict__ n_large) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const int view = blockIdx.y;
  Tri t;
  if (!tri_setup(faces, f, V, cam + (size_t)view * V, snapped + (size_t)view * V, W, H, t)) return;
  const int bw = t.i1 - t.i0 + 1, bh = t.j1 - t.j0 + 1;
  if ((i64)bw * bh > kSmallBox) {                      // the list has room for every (face, view)
    large[atomicAdd(n_large, 1u)] = (unsigned)view * (unsigned)F + (unsigned)f;
    return;
  }
  u64* z0 = zbuf + (size_t)view * W * H;
  for (int j = t.j0; j <= t.j1; ++j)
    for (int i = t.i0; i <= t.i1; ++i) tri_pixel(t, i, j, (unsigned)f, z0, W);
}

__global__ __launch_bounds__(256) void render_raster_large_kernel(const int* __restrict__ faces, int F, int V,
                                                                  const v4f* __restrict__ cam,
                                                                  const v4i* __restrict__ snapped, int W, int H,
                                                                  u64* __restrict__ zbuf,
                                                                  const unsigned* __restrict__ large,
                                                                  const unsigned* __restrict__ n_large,
                                                                  unsigned n_views) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);
  const unsigned n_waves = gridDim.x * 4u;
  unsigned n = *n_large;
  n = n < n_views * (unsigned)F ? n : n_views * (unsigned)F;   // the list's capacity
  const u64 items = (u64)n * kChunks;
  for (u64 w = wave; w < items; w += n_waves) {
    const unsigned e = large[w / kChunks], chunk = (unsigned)(w % kChunks);
    const unsigned view = e / (unsigned)F, f = e % (unsigned)F;
    if (view >= n_views) continue;
    Tri t;
    if (!tri_setup(faces, (int)f, V, cam + (size_t)view * V, snapped + (size_t)view * V, W, H, t)) continue;
    const unsigned bw = (unsigned)(t.i1 - t.i0 + 1), bh = (unsigned)(t.j1 - t.j0 + 1);
    const unsigned npix = bw * bh;                     // W, H <= FPSG_RENDER_MAX_SIZE: below 2^32
    u64* z0 = zbuf + (size_t)view * W * H;
    for (unsigned p = chunk * 64u + lane; p < npix; p += 64u * kChunks)
      tri_pixel(t, t.i0 + (int)(p % bw), t.j0 + (int)(p / bw), f, z0, W);
  }
}

// ---- the shade pass: K27's flat Phong, K28's materials and textures, K31b's interpolated normals -----------------
// The unit normal of the face (a, b, c) in the frame of the view M, towards the camera, which looks along +z (both
// sides of a face are lit); (0, 0, -1) for a face without area.
__device__ __forceinline__ void face_normal_cam(const float* __restrict__ a, const float* __restrict__ b,
                                                const float* __restrict__ c, const float* __restrict__ M, float& nx,
                                                float& ny, float& nz) {
  // world-space edges turned into the camera frame: no cancellation against the camera's distance
  const float w1x = b[0] - a[0], w1y = b[1] - a[1], w1z = b[2] - a[2];
  const float w2x = c[0] - a[0], w2y = c[1] - a[1], w2z = c[2] - a[2];
  const float e1x = (w1x * M[0] + w1y * M[1]) + w1z * M[2], e1y = (w1x * M[3] + w1y * M[4]) + w1z * M[5],
              e1z = (w1x * M[6] + w1y * M[7]) + w1z * M[8];
  const float e2x = (w2x * M[0] + w2y * M[1]) + w2z * M[2], e2y = (w2x * M[3] + w2y * M[4]) + w2z * M[5],
              e2z = (w2x * M[6] + w2y * M[7]) + w2z * M[8];
  nx = e1y * e2z - e1z * e2y;
  ny = e1z * e2x - e1x * e2z;
  nz = e1x * e2y - e1y * e2x;
  const float len = __builtin_sqrtf((nx * nx + ny * ny) + nz * nz);
  if (len > 0.0f && finite_f(len)) { nx = nx / len; ny = ny / len; nz = nz / len; }
  else { nx = 0.0f; ny = 0.0f; nz = -1.0f; }
  if (nz > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
}

struct MaterialTables {
  const int* face_material;              // [F], outside [0, M): no material
  const v4f* materials;                  // [M]: Kd and the texture index (validated by the entry: -1 or in [0, T))
  const float* face_uv;                  // [F, 3, 2]
  const int* tex_table;                  // [T, 3]: texel offset, width, height (validated: inside texels)
  const unsigned char* texels;
  int M;
};

// t in [0, 1); anything else (1 after rounding, NaN from an overflowed uv) becomes 0
__device__ __forceinline__ float repeat_unit(float u) {
  const float t = u - __builtin_floorf(u);
  return (t >= 0.0f && t < 1.0f) ? t : 0.0f;
}

__device__ __forceinline__ int wrap_index(int i, int n) {
  const int r = i % n;
  return r < 0 ? r + n : r;
}

// Bilinear lookup with repeat; w, h >= 1 and the texture inside texels by the entry's checks, indices wrapped here.
__device__ __forceinline__ void texel_lookup(const unsigned char* __restrict__ tex, int w, int h, float u, float v,
                                             float& r, float& g, float& b) {
  const float tu = repeat_unit(u), tv = repeat_unit(v);
  const float x = tu * (float)w - 0.5f, y = (1.0f - tv) * (float)h - 0.5f;
  const float xf = __builtin_floorf(x), yf = __builtin_floorf(y);
  const float fx = x - xf, fy = y - yf;
  const int ix0 = wrap_index((int)xf, w), ix1 = wrap_index((int)xf + 1, w);
  const int iy0 = wrap_index((int)yf, h), iy1 = wrap_index((int)yf + 1, h);
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  const float w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy;
  const unsigned char* p00 = tex + ((size_t)iy0 * w + ix0) * 3;
  const unsigned char* p10 = tex + ((size_t)iy0 * w + ix1) * 3;
  const unsigned char* p01 = tex + ((size_t)iy1 * w + ix0) * 3;
  const unsigned char* p11 = tex + ((size_t)iy1 * w + ix1) * 3;
  float c[3];
  for (int k = 0; k < 3; ++k)
    c[k] = ((w00 * ((float)p00[k] / 255.0f) + w10 * ((float)p10[k] / 255.0f)) + w01 * ((float)p01[k] / 255.0f)) +
           w11 * ((float)p11[k] / 255.0f);
  r = c[0]; g = c[1]; b = c[2];
}

// K28's barycentrics of the sample centre (i, j) in a drawn face, from the snapped corners; swap: the rasteriser's
// exchange of corners 1 and 2 (A2 < 0) was applied, and what is interpolated must exchange with them.
struct Bary {
  float l0, l1, l2;
  bool swap;
};

__device__ __forceinline__ Bary sample_bary(const v4i* __restrict__ snap_v, int ia, int ib, int ic, int i, int j) {
  const v4i s0 = snap_v[ia];
  v4i s1 = snap_v[ib], s2 = snap_v[ic];
  i64 A2 = (i64)(s1.x - s0.x) * (i64)(s2.y - s0.y) - (i64)(s1.y - s0.y) * (i64)(s2.x - s0.x);
  Bary r;
  r.swap = A2 < 0;
  if (r.swap) {
    const v4i s = s1; s1 = s2; s2 = s;
    A2 = -A2;
  }
  const int px = 256 * i + 128, py = 256 * j + 128;
  const float A = (float)A2;                           // not 0: the face was drawn
  r.l0 = (float)edge_fn(s1.x, s1.y, s2.x, s2.y, px, py) / A;
  r.l1 = (float)edge_fn(s2.x, s2.y, s0.x, s0.y, px, py) / A;
  r.l2 = (float)edge_fn(s0.x, s0.y, s1.x, s1.y, px, py) / A;
  return r;
}

// One output pixel per thread: its ssaa^2 samples shaded and composited over the background.
//   FLAT (K27): the face's normal and the colour in ka, kd.  It reads neither snapped, T, face_normals nor
//     Q.ambient / Q.diffuse: the K27 entry has none of them to give.
//   MATERIALS (K28): a face with a material takes its base colour from the material's Kd or texture.
//   SMOOTH (K31b): K28 with the light's terms from the normal interpolated between face_normals [F,3,3].
enum Shade { FLAT, MATERIALS, SMOOTH };

template <Shade MODE>
__global__ __launch_bounds__(256) void render_shade_kernel(
    const float* __restrict__ verts, const int* __restrict__ faces, int V, const float* __restrict__ views,
    const v4i* __restrict__ snapped, const u64* __restrict__ zbuf, int W, int H, int ssaa, MaterialParams Q,
    MaterialTables T, const float* __restrict__ face_normals, const unsigned char* __restrict__ bg_img,
    unsigned char* __restrict__ image, float* __restrict__ radiance, int* __restrict__ face_id,
    float* __restrict__ depth) {
  const RenderParams& P = Q.base;
  const int ow = W / ssaa, oh = H / ssaa;
  const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (ox >= ow || oy >= oh) return;
  const int view = blockIdx.z;
  const float* M = views + (size_t)view * 12;
  const u64* z0 = zbuf + (size_t)view * W * H;
  const v4i* snap_v = snapped + (size_t)view * V;
  float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
  int covered = 0;
  for (int sy = 0; sy < ssaa; ++sy) {
    for (int sx = 0; sx < ssaa; ++sx) {
      const int i = ox * ssaa + sx, j = oy * ssaa + sy;
      const size_t pix = (size_t)j * W + i;
      const u64 key = z0[pix];
      const bool hit = key != kEmpty;
      if (face_id) face_id[(size_t)view * W * H + pix] = hit ? (int)(unsigned)key : -1;
      if (depth) depth[(size_t)view * W * H + pix] = hit ? key_depth((unsigned)(key >> 32)) : __builtin_inff();
      if (!hit) continue;
      const unsigned f = (unsigned)key;                // written by the rasteriser: a face with indices in range
      const int ia = faces[(size_t)f * 3], ib = faces[(size_t)f * 3 + 1], ic = faces[(size_t)f * 3 + 2];
      float nx, ny, nz;
      face_normal_cam(verts + (size_t)ia * 3, verts + (size_t)ib * 3, verts + (size_t)ic * 3, M, nx, ny, nz);
      Bary L = {0.0f, 0.0f, 0.0f, false};
      if constexpr (MODE == SMOOTH) {
        // the corner normals interpolated in world space, turned into the camera frame like the edges, normalised,
        // and put on the side of the face that the camera sees; without a usable length the face's own normal stays
        L = sample_bary(snap_v, ia, ib, ic, i, j);
        const float* q = face_normals + (size_t)f * 9;
        const float* q1 = L.swap ? q + 6 : q + 3;
        const float* q2 = L.swap ? q + 3 : q + 6;
        const float mx = (L.l0 * q[0] + L.l1 * q1[0]) + L.l2 * q2[0];
        const float my = (L.l0 * q[1] + L.l1 * q1[1]) + L.l2 * q2[1];
        const float mz = (L.l0 * q[2] + L.l1 * q1[2]) + L.l2 * q2[2];
        float cx = (mx * M[0] + my * M[1]) + mz * M[2], cy = (mx * M[3] + my * M[4]) + mz * M[5],
              cz = (mx * M[6] + my * M[7]) + mz * M[8];
        const float mlen = __builtin_sqrtf((cx * cx + cy * cy) + cz * cz);
        if (mlen > 0.0f && finite_f(mlen)) {
          cx = cx / mlen; cy = cy / mlen; cz = cz / mlen;
          const float side = (cx * nx + cy * ny) + cz * nz;
          if (side < 0.0f) { cx = -cx; cy = -cy; cz = -cz; }
          nx = cx; ny = cy; nz = cz;
        }
      }
      float diff, spec, c0, c1, c2;
      light_terms(P, nx, ny, nz, diff, spec);
      int m = -1;
      if constexpr (MODE != FLAT) m = T.M > 0 ? T.face_material[f] : -1;
      if (MODE == FLAT || (unsigned)m >= (unsigned)T.M) {   // no material
        phong_color(P, diff, spec, c0, c1, c2);
      } else {
        const v4f mat = T.materials[m];
        float b0 = mat.x, b1 = mat.y, b2 = mat.z;
        const int tex = (int)mat.w;
        if (tex >= 0) {
          const float* q = T.face_uv + (size_t)f * 6;
          float u0 = q[0], v0 = q[1], u1 = q[2], v1 = q[3], u2 = q[4], v2 = q[5];
          if (finite_f(u0) && finite_f(v0) && finite_f(u1) && finite_f(v1) && finite_f(u2) && finite_f(v2)) {
            if constexpr (MODE != SMOOTH) L = sample_bary(snap_v, ia, ib, ic, i, j);
            if (L.swap) {                              // the rasteriser's swap, and the uv with the corners
              float t = u1; u1 = u2; u2 = t;
              t = v1; v1 = v2; v2 = t;
            }
            const float u = (L.l0 * u0 + L.l1 * u1) + L.l2 * u2;
            const float v = (L.l0 * v0 + L.l1 * v1) + L.l2 * v2;
            const int* e = T.tex_table + (size_t)tex * 3;
            texel_lookup(T.texels + (size_t)e[0] * 3, e[1], e[2], u, v, b0, b1, b2);
          }
        }
        phong_color(Q, b0, b1, b2, diff, spec, c0, c1, c2);
      }
      acc0 += c0; acc1 += c1; acc2 += c2;
      ++covered;
    }
  }
  resolve_pixel(acc0, acc1, acc2, covered, ssaa, P, bg_img, (size_t)oy * ow + ox,
                (((size_t)view * oh + oy) * ow + ox) * 3, radiance, image);
}

struct RenderWs {
  size_t cam, snapped, zbuf, list, counter, total;
};

inline RenderWs render_ws(int V, int F, int NV, int W, int H) {
  RenderWs w;
  size_t o = 0;
  w.cam = o; o += (size_t)NV * V * 16;
  w.snapped = o; o += (size_t)NV * V * 16;
  w.zbuf = o; o += (size_t)NV * W * H * 8;
  w.list = o; o += (((size_t)NV * F * 4) + 15) & ~(size_t)15;
  w.counter = o; o += 16;
  w.total = o;
  return w;
}

// K28's workspace: K27's, then the material and texture tables copied from the host; nothing more for M = T = 0, so
// K27's size is this one's
struct MaterialWs {
  size_t materials, tex_table, total;
};

inline MaterialWs material_ws(const RenderWs& L, int M, int T) {
  MaterialWs w;
  size_t o = L.total;
  w.materials = o; o += (size_t)M * 16;
  w.tex_table = o; o += (((size_t)T * 12) + 15) & ~(size_t)15;
  w.total = o;
  return w;
}

inline bool material_limit_ok(int M, int T, long long n_texels) {
  return M <= FPSG_RENDER_MAX_MATERIALS && T <= FPSG_RENDER_MAX_TEXTURES && n_texels <= FPSG_RENDER_MAX_TEXELS;
}

inline bool render_shape_ok(int V, int F, int NV, int W, int H, int ssaa) {
  return V > 0 && F > 0 && NV > 0 && W > 0 && H > 0 && ssaa >= 1 && ssaa <= FPSG_RENDER_MAX_SSAA && W % ssaa == 0 &&
         H % ssaa == 0;
}
inline bool render_limit_ok(int F, int NV, int W, int H) {
  return W <= FPSG_RENDER_MAX_SIZE && H <= FPSG_RENDER_MAX_SIZE && NV <= FPSG_RENDER_MAX_VIEWS &&
         (uint64_t)F * (uint64_t)NV <= 0x7fffffffull;
}

#define RENDER_REQUIRE_PTR(p)                                                                     \
  do {                                                                                             \
    FPSG_REQUIRE((p) != nullptr, FPSG_E_NULL, "%s: null pointer '%s'", fn, #p);                    \
    FPSG_REQUIRE(!misaligned4(p), FPSG_E_ALIGN, "%s: '%s' not 4-byte aligned", fn, #p);            \
  } while (0)

// The entry of K27, K28 and K31b: the same checks, workspace and launches; mode selects the shade pass.  K27 comes
// with M = T = 0, no tables and 15 floats in params; face_normals is K31b's alone.
int render_entry(const char* fn, Shade mode, const float* verts, int V, const int32_t* faces, int F,
                 const int32_t* face_material, const float* face_uv, const float* face_normals, const float* materials,
                 int M, const int32_t* tex_table, int T, const uint8_t* texels, long long n_texels, const float* views,
                 int n_views, int W, int H, int ssaa, float ortho_scale, const float* params, int log2_shininess,
                 const uint8_t* bg_image, uint8_t* image, float* radiance, int32_t* face_id, float* depth, void* ws,
                 size_t ws_bytes, fpsg_stream_t stream) {
  FPSG_REQUIRE(render_shape_ok(V, F, n_views, W, H, ssaa), FPSG_E_SHAPE,
               "%s: V,F,n_views,W,H must be positive, ssaa from 1 to %d and a divisor of W "
               "and H (got %d,%d,%d,%d,%d,%d)", fn, FPSG_RENDER_MAX_SSAA, V, F, n_views, W, H, ssaa);
  FPSG_REQUIRE(M >= 0 && T >= 0 && n_texels >= 0, FPSG_E_SHAPE,
               "%s: M, T and n_texels must not be negative (got %d,%d,%lld)", fn, M, T, n_texels);
  FPSG_REQUIRE(ortho_scale > 0.0f && ortho_scale <= 3.0e38f, FPSG_E_SHAPE,
               "%s: ortho_scale must be positive and finite", fn);
  FPSG_REQUIRE(log2_shininess >= 0 && log2_shininess <= FPSG_RENDER_MAX_LOG2_SHININESS, FPSG_E_SHAPE,
               "%s: log2_shininess must be from 0 to %d (got %d)", fn, FPSG_RENDER_MAX_LOG2_SHININESS, log2_shininess);
  FPSG_REQUIRE(render_limit_ok(F, n_views, W, H), FPSG_E_LIMIT,
               "%s: W,H <= %d, n_views <= %d and F n_views < 2^31 are supported (got "
               "%d,%d,%d,%d)", fn, FPSG_RENDER_MAX_SIZE, FPSG_RENDER_MAX_VIEWS, W, H, n_views, F);
  FPSG_REQUIRE(material_limit_ok(M, T, n_texels), FPSG_E_LIMIT,
               "%s: M <= %d, T <= %d and n_texels <= %d are supported (got %d,%d,%lld)", fn,
               FPSG_RENDER_MAX_MATERIALS, FPSG_RENDER_MAX_TEXTURES, FPSG_RENDER_MAX_TEXELS, M, T, n_texels);
  RENDER_REQUIRE_PTR(verts); RENDER_REQUIRE_PTR(faces); RENDER_REQUIRE_PTR(views); RENDER_REQUIRE_PTR(ws);
  FPSG_REQUIRE(params != nullptr, FPSG_E_NULL, "%s: null pointer 'params'", fn);
  if (M > 0) { RENDER_REQUIRE_PTR(face_material); RENDER_REQUIRE_PTR(materials); }
  if (T > 0) { RENDER_REQUIRE_PTR(face_uv); RENDER_REQUIRE_PTR(tex_table); }
  if (mode == SMOOTH) RENDER_REQUIRE_PTR(face_normals);
  FPSG_REQUIRE(T == 0 || texels != nullptr, FPSG_E_NULL, "%s: null pointer 'texels'", fn);
  FPSG_REQUIRE(image || radiance || face_id || depth, FPSG_E_NULL, "%s: no output requested", fn);
  FPSG_REQUIRE(!misaligned4(radiance) && !misaligned4(face_id) && !misaligned4(depth), FPSG_E_ALIGN,
               "%s: an output is not 4-byte aligned", fn);
  FPSG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15u) == 0, FPSG_E_ALIGN, "%s: 'ws' must be 16-byte aligned", fn);
  for (int t = 0; t < T; ++t) {                        // tex_table and materials are host memory
    const long long off = tex_table[3 * t], tw = tex_table[3 * t + 1], th = tex_table[3 * t + 2];
    FPSG_REQUIRE(off >= 0 && tw >= 1 && th >= 1 && off + tw * th <= n_texels, FPSG_E_SHAPE,
                 "%s: texture %d (offset %lld, %lld x %lld) reaches outside the %lld texels", fn, t, off, tw, th,
                 n_texels);
  }
  for (int m = 0; m < M; ++m) {
    const float ti = materials[4 * m + 3];
    FPSG_REQUIRE(ti >= -1.0f && ti < (float)T && ti == __builtin_floorf(ti), FPSG_E_SHAPE,
                 "%s: material %d has texture index %g, outside [-1, %d)", fn, m, (double)ti, T);
  }
  const RenderWs L = render_ws(V, F, n_views, W, H);
  const MaterialWs LM = material_ws(L, M, T);
  FPSG_REQUIRE(ws_bytes >= LM.total, FPSG_E_SHAPE, "%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, LM.total);
  MaterialParams Q = {};
  if (mode == FLAT) unpack_render_params(params, log2_shininess, Q.base);
  else unpack_material_params(params, log2_shininess, Q);
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  v4f* cam = reinterpret_cast<v4f*>(base + L.cam);
  v4i* snapped = reinterpret_cast<v4i*>(base + L.snapped);
  u64* zbuf = reinterpret_cast<u64*>(base + L.zbuf);
  unsigned* list = reinterpret_cast<unsigned*>(base + L.list);
  unsigned* counter = reinterpret_cast<unsigned*>(base + L.counter);
  MaterialTables TB;
  TB.face_material = face_material;
  TB.materials = reinterpret_cast<const v4f*>(base + LM.materials);
  TB.face_uv = face_uv;
  TB.tex_table = reinterpret_cast<const int*>(base + LM.tex_table);
  TB.texels = texels;
  TB.M = M;
  hipError_t e = hipMemsetAsync(zbuf, 0xff, (size_t)n_views * W * H * 8, st);
  if (e == hipSuccess) e = hipMemsetAsync(counter, 0, 16, st);
  // the two host tables: pageable memory is staged before hipMemcpyAsync returns (pinned: see the header)
  if (e == hipSuccess && M > 0)
    e = hipMemcpyAsync(base + LM.materials, materials, (size_t)M * 16, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && T > 0)
    e = hipMemcpyAsync(base + LM.tex_table, tex_table, (size_t)T * 12, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) { set_error("%s: %s", fn, hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL(render_project_kernel, dim3((unsigned)((V + 255) / 256), (unsigned)n_views), dim3(256), 0, st,
                     verts, V, views, ortho_scale, W, H, cam, snapped);
  hipLaunchKernelGGL(render_raster_kernel, dim3((unsigned)((F + 255) / 256), (unsigned)n_views), dim3(256), 0, st,
                     faces, F, V, cam, snapped, W, H, zbuf, list, counter);
  // a fixed grid strides over the list, whose length only the device knows
  hipLaunchKernelGGL(render_raster_large_kernel, dim3(1024), dim3(256), 0, st, faces, F, V, cam, snapped, W, H, zbuf,
                     list, counter, (unsigned)n_views);
  const int ow = W / ssaa, oh = H / ssaa;
  const dim3 grid((unsigned)((ow + 63) / 64), (unsigned)((oh + 3) / 4), (unsigned)n_views);
  const auto shade = mode == FLAT ? render_shade_kernel<FLAT>
                     : mode == SMOOTH ? render_shade_kernel<SMOOTH> : render_shade_kernel<MATERIALS>;
  hipLaunchKernelGGL(shade, grid, dim3(256), 0, st, verts, faces, V, views, snapped, zbuf, W, H, ssaa, Q, TB,
                     face_normals, bg_image, image, radiance, face_id, depth);
  return launch_status(fn);
}
#undef RENDER_REQUIRE_PTR

}  // namespace
}  // namespace fpsg

extern "C" size_t fpsg_mesh_render_materials_workspace_bytes(int V, int F, int n_views, int W, int H, int M, int T) {
  using namespace fpsg;
  if (!render_shape_ok(V, F, n_views, W, H, 1) || !render_limit_ok(F, n_views, W, H) || M < 0 || T < 0 ||
      !material_limit_ok(M, T, 0))
    return 0;
  return material_ws(render_ws(V, F, n_views, W, H), M, T).total;
}

extern "C" size_t fpsg_mesh_render_workspace_bytes(int V, int F, int n_views, int W, int H) {
  return fpsg_mesh_render_materials_workspace_bytes(V, F, n_views, W, H, 0, 0);   // material_ws adds nothing
}

extern "C" int fpsg_mesh_render(const float* verts, int V, const int32_t* faces, int F, const float* views,
                                int n_views, int W, int H, int ssaa, float ortho_scale, const float* params,
                                int log2_shininess, const uint8_t* bg_image, uint8_t* image, float* radiance,
                                int32_t* face_id, float* depth, void* ws, size_t ws_bytes, fpsg_stream_t stream) {
  return fpsg::render_entry("fpsg_mesh_render", fpsg::FLAT, verts, V, faces, F, nullptr, nullptr, nullptr, nullptr, 0,
                            nullptr, 0, nullptr, 0, views, n_views, W, H, ssaa, ortho_scale, params, log2_shininess,
                            bg_image, image, radiance, face_id, depth, ws, ws_bytes, stream);
}

extern "C" int fpsg_mesh_render_materials(const float* verts, int V, const int32_t* faces, int F,
                                          const int32_t* face_material, const float* face_uv, const float* materials,
                                          int M, const int32_t* tex_table, int T, const uint8_t* texels,
                                          long long n_texels, const float* views, int n_views, int W, int H, int ssaa,
                                          float ortho_scale, const float* params, int log2_shininess,
                                          const uint8_t* bg_image, uint8_t* image, float* radiance, int32_t* face_id,
                                          float* depth, void* ws, size_t ws_bytes, fpsg_stream_t stream) {
  return fpsg::render_entry("fpsg_mesh_render_materials", fpsg::MATERIALS, verts, V, faces, F, face_material, face_uv,
                            nullptr, materials, M, tex_table, T, texels, n_texels, views, n_views, W, H, ssaa,
                            ortho_scale, params, log2_shininess, bg_image, image, radiance, face_id, depth, ws, ws_bytes,
                            stream);
}

extern "C" size_t fpsg_mesh_render_smooth_workspace_bytes(int V, int F, int n_views, int W, int H, int M, int T) {
  return fpsg_mesh_render_materials_workspace_bytes(V, F, n_views, W, H, M, T);
}

extern "C" int fpsg_mesh_render_smooth(const float* verts, int V, const int32_t* faces, int F,
                                       const int32_t* face_material, const float* face_uv, const float* face_normals,
                                       const float* materials, int M, const int32_t* tex_table, int T,
                                       const uint8_t* texels, long long n_texels, const float* views, int n_views, int W,
                                       int H, int ssaa, float ortho_scale, const float* params, int log2_shininess,
                                       const uint8_t* bg_image, uint8_t* image, float* radiance, int32_t* face_id,
                                       float* depth, void* ws, size_t ws_bytes, fpsg_stream_t stream) {
  return fpsg::render_entry("fpsg_mesh_render_smooth", fpsg::SMOOTH, verts, V, faces, F, face_material, face_uv,
                            face_normals, materials, M, tex_table, T, texels, n_texels, views, n_views, W, H, ssaa,
                            ortho_scale, params, log2_shininess, bg_image, image, radiance, face_id, depth, ws, ws_bytes,
                            stream);
}
