// render_common.h -- what K27/K28 (mesh_render.hip) and K29 (points_render.hip) share: the camera projection with its
// snap to 1/256 sample pixel, the order-preserving depth key, and the shading parameters.  Definitions: include/fpsg_hip.h.
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

inline void unpack_render_params(const float* params, int log2_shininess, RenderParams& P) {
  for (int k = 0; k < 3; ++k) {
    P.ka[k] = params[k]; P.kd[k] = params[3 + k]; P.ks[k] = params[6 + k];
    P.light[k] = params[9 + k]; P.bg[k] = params[12 + k];
  }
  P.log2_shininess = log2_shininess;
}

}  // namespace fpsg
