// render_common.h -- what K27/K28/K31b (mesh_render.hip) and K29 (points_render.hip) share, each written once because
// every one of these kernels promises bit-for-bit results: the camera projection with its snap to 1/256 sample pixel, the
// order-preserving depth key, the shading parameters and their unpacking, the light's terms, the two colour forms and
// the resolve of an output pixel.  Definitions: include/fpsg_hip.h.
#pragma once
#include "fpsg_common.h"

namespace fpsg {

constexpr float kSnapLimit = 268435456.0f;   // 2^28: snapped coordinates stay below it, edge functions below 2^60

struct RenderParams {
  float ka[3], kd[3], ks[3], light[3], bg[3];
  int log2_shininess;
};

// K28's and K29's: a base colour b per face or point is scaled by ambient and diffuse in place of ka and kd
struct MaterialParams {
  RenderParams base;
  float ambient, diffuse;
};

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// float -> unsigned with the same order (negative depths included)
__device__ __forceinline__ unsigned depth_key(float z) {
  const unsigned b = __float_as_uint(z);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_depth(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ int snap(float p) {
  const float v = p * 256.0f;
  return (int)__builtin_rintf(__builtin_fminf(__builtin_fmaxf(v, -kSnapLimit), kSnapLimit));
}

// K27's "Project": p (3 floats) seen by the view M (right, up, forward, position) -> camera-space x, y, depth d and the
// snapped X, Y (0 when the point is invalid).  Returns whether px, py and d are finite.
__device__ __forceinline__ bool project_point(const float* __restrict__ p, const float* __restrict__ M,
                                              float ortho_scale, int W, int H, float& x, float& y, float& d, int& X,
                                              int& Y) {
  const float dx = p[0] - M[9], dy = p[1] - M[10], dz = p[2] - M[11];
  x = (dx * M[0] + dy * M[1]) + dz * M[2];
  y = (dx * M[3] + dy * M[4]) + dz * M[5];
  d = (dx * M[6] + dy * M[7]) + dz * M[8];
  const float S = (float)(W > H ? W : H);
  const float px = (x / ortho_scale) * S + 0.5f * (float)W;
  const float py = 0.5f * (float)H - (y / ortho_scale) * S;
  const bool ok = finite_f(px) && finite_f(py) && finite_f(d);
  X = ok ? snap(px) : 0;
  Y = ok ? snap(py) : 0;
  return ok;
}

// The light's terms for the unit camera-frame normal n; the viewer is v = (0, 0, -1).
__device__ __forceinline__ void light_terms(const RenderParams& P, float nx, float ny, float nz, float& diff,
                                            float& spec) {
  const float ndl = (nx * P.light[0] + ny * P.light[1]) + nz * P.light[2];
  diff = __builtin_fmaxf(ndl, 0.0f);
  // r = 2 (n.l) n - l: r.v = l_z - 2 (n.l) n_z
  spec = ndl > 0.0f ? __builtin_fmaxf(P.light[2] - (2.0f * ndl) * nz, 0.0f) : 0.0f;
  for (int k = 0; k < P.log2_shininess; ++k) spec = spec * spec;
}

// The colour of a sample without a base colour of its own: ka and kd as given
__device__ __forceinline__ void phong_color(const RenderParams& P, float diff, float spec, float& c0, float& c1,
                                            float& c2) {
  c0 = (P.ka[0] + P.kd[0] * diff) + P.ks[0] * spec;
  c1 = (P.ka[1] + P.kd[1] * diff) + P.ks[1] * spec;
  c2 = (P.ka[2] + P.kd[2] * diff) + P.ks[2] * spec;
}

// ... and with the base colour b (a material's, a texel's, a point's) in place of the one folded into ka and kd
__device__ __forceinline__ void phong_color(const MaterialParams& Q, float b0, float b1, float b2, float diff,
                                            float spec, float& c0, float& c1, float& c2) {
  const float a0 = Q.ambient * b0, a1 = Q.ambient * b1, a2 = Q.ambient * b2;
  const float d0 = Q.diffuse * b0, d1 = Q.diffuse * b1, d2 = Q.diffuse * b2;
  c0 = (a0 + d0 * diff) + Q.base.ks[0] * spec;
  c1 = (a1 + d1 * diff) + Q.base.ks[1] * spec;
  c2 = (a2 + d2 * diff) + Q.base.ks[2] * spec;
}

__device__ __forceinline__ unsigned char quantize(float r) {
  return (unsigned char)__builtin_rintf(__builtin_fminf(__builtin_fmaxf(r, 0.0f), 1.0f) * 255.0f);
}

// K27's "Resolve" of one output pixel: acc sums the colours of its covered samples; px is the pixel's index in one
// image, where bg_img (null: P.bg) has its background, out that of its first float in radiance and byte in image
// (either may be null).
__device__ __forceinline__ void resolve_pixel(float acc0, float acc1, float acc2, int covered, int ssaa,
                                              const RenderParams& P, const unsigned char* __restrict__ bg_img,
                                              size_t px, size_t out, float* __restrict__ radiance,
                                              unsigned char* __restrict__ image) {
  const float inv = 1.0f / (float)(ssaa * ssaa);
  const float rest = 1.0f - (float)covered * inv;
  float bg0 = P.bg[0], bg1 = P.bg[1], bg2 = P.bg[2];
  if (bg_img) {
    const unsigned char* q = bg_img + px * 3;
    bg0 = (float)q[0] / 255.0f; bg1 = (float)q[1] / 255.0f; bg2 = (float)q[2] / 255.0f;
  }
  const float r0 = acc0 * inv + bg0 * rest, r1 = acc1 * inv + bg1 * rest, r2 = acc2 * inv + bg2 * rest;
  if (radiance) { radiance[out] = r0; radiance[out + 1] = r1; radiance[out + 2] = r2; }
  if (image) { image[out] = quantize(r0); image[out + 1] = quantize(r1); image[out + 2] = quantize(r2); }
}

// params: the 15 floats ka, kd, ks, light, bg
inline void unpack_render_params(const float* params, int log2_shininess, RenderParams& P) {
  for (int k = 0; k < 3; ++k) {
    P.ka[k] = params[k]; P.kd[k] = params[3 + k]; P.ks[k] = params[6 + k];
    P.light[k] = params[9 + k]; P.bg[k] = params[12 + k];
  }
  P.log2_shininess = log2_shininess;
}

// params: those 15 floats, then ambient and diffuse
inline void unpack_material_params(const float* params, int log2_shininess, MaterialParams& Q) {
  unpack_render_params(params, log2_shininess, Q.base);
  Q.ambient = params[15]; Q.diffuse = params[16];
}

}  // namespace fpsg
