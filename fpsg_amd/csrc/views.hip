// views.hip -- K30: the uint8 images of an episode -> the float32 [n,3,Ho,Wo] batch the image encoder reads, for gfx950.
// One launch selects (sel), resamples (geom: an integer bilinear blend on a 1/256-pixel grid, clamp to edge), colour-
// jitters (color: saturation, contrast and brightness in fp32) and normalises.  The definition is in include/fpsg_hip.h
// (K30) and DESIGN.md; tests/_views_ref.py restates it in numpy and the kernel equals that bit for bit.
//
// Structure: a streaming kernel, 3 to 12 source bytes read and 12 bytes written per output pixel.
//   * one thread owns all three channels of its pixels (the luma needs them);
//   * with Wo a multiple of 4 (and `out` 16-byte aligned) a thread takes four consecutive pixels of a row, so each of its
//     three plane stores is 16 bytes per lane and a wave's stores are contiguous; any other Wo runs the one-pixel form;
//   * a window whose x0, y0 and step are multiples of 256 (the identity among them) has fx = fy = 0 everywhere: a uniform
//     branch per image takes the one-tap form, 3 source bytes per pixel instead of 12 -- the blend is in integers, so
//     leaving the three zero products out changes nothing;
//   * the per-image tables are read through a wave-uniform index; no LDS, no atomics, plain vector stores.
#include "fpsg_common.h"

namespace fpsg {
namespace {

constexpr int kThreads = 256;
constexpr int kOffsetMax = 1 << 24;      // |x0|, |y0|, in 1/256 source pixel
constexpr int kStepMax = 1 << 16;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// The pixels (row j, columns i0 .. i0 + PX - 1) of one image.  WHOLE: x0, y0 and step are multiples of 256, so every fx and
// fy is zero and a pixel is one tap (the integer blend of the other three has weight zero: leaving it out changes nothing).
template <int PX, bool WHOLE>
__device__ __forceinline__ void view_pixels(const uint8_t* __restrict__ img, int Hs, int Ws, int x0, int y0, int step,
                                            const float* __restrict__ color, int j, int i0, float (&res)[3][PX]) {
  float br = 0.0f, ct = 1.0f, sa = 1.0f;
  if (color) { br = color[0]; ct = color[1]; sa = color[2]; }
  const int Y = y0 + j * step;                               // |Y| < 2^24 + 2^13 2^16
  const int iy = Y >> 8, fy = Y & 255;
  const uint8_t* r0 = img + (size_t)clampi(iy, 0, Hs - 1) * Ws * 3;
  const uint8_t* r1 = img + (size_t)clampi(iy + 1, 0, Hs - 1) * Ws * 3;
#pragma unroll
  for (int p = 0; p < PX; ++p) {
    const int X = x0 + (i0 + p) * step;
    const int ix = X >> 8, fx = X & 255;
    const int c0 = clampi(ix, 0, Ws - 1) * 3, c1 = clampi(ix + 1, 0, Ws - 1) * 3;     // + channel < 3 Ws
    float x[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int v;                                                 // 0 .. 255 * 65536 < 2^24: exact as a float
      if constexpr (WHOLE) {
        v = (int)r0[c0 + c] << 16;
      } else {
        const int a0 = (int)r0[c0 + c] * (256 - fx) + (int)r0[c1 + c] * fx;
        const int a1 = (int)r1[c0 + c] * (256 - fx) + (int)r1[c1 + c] * fx;
        v = a0 * (256 - fy) + a1 * fy;
      }
      x[c] = (float)v / 16711680.0f;
    }
    if (color) {
      const float l = (0.299f * x[0] + 0.587f * x[1]) + 0.114f * x[2];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float tt = l + sa * (x[c] - l);
        const float u = (tt - 0.5f) * ct + (0.5f + br);
        x[c] = __builtin_fminf(__builtin_fmaxf(u, 0.0f), 1.0f);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) res[c][p] = (x[c] - 0.5f) / 0.5f;
  }
}

template <int PX>
__global__ __launch_bounds__(kThreads) void episode_views_kernel(const uint8_t* __restrict__ src, int n_src, int Hs,
                                                                 int Ws, const int* __restrict__ sel,
                                                                 const int* __restrict__ geom,
                                                                 const float* __restrict__ color,
                                                                 float* __restrict__ out, int Ho, int Wo) {
  const int k = blockIdx.y;                                  // the grid's y is n: sel[k], geom[4k..], color[4k..] exist
  const int wq = Wo / PX;                                    // PX = 4 only when it divides Wo
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= Ho * wq) return;                                  // Ho wq <= 2^26
  const int j = t / wq, i0 = (t - j * wq) * PX;              // row j < Ho, columns i0 .. i0 + PX - 1 < Wo
  const size_t plane = (size_t)Ho * Wo;
  float* o = out + (size_t)k * 3 * plane + (size_t)j * Wo + i0;
  float res[3][PX];

  const int s = sel[k];
  if (s < 0 || s >= n_src) {                                 // no read of src for such an image
    const float q = __builtin_nanf("");
#pragma unroll
    for (int p = 0; p < PX; ++p) res[0][p] = res[1][p] = res[2][p] = q;
  } else {
    int x0 = 0, y0 = 0, step = 256;
    if (geom) {                                              // the wrapper checks the ranges; the clamp keeps X, Y in int32
      x0 = clampi(geom[4 * k], -kOffsetMax, kOffsetMax);
      y0 = clampi(geom[4 * k + 1], -kOffsetMax, kOffsetMax);
      step = clampi(geom[4 * k + 2], 1, kStepMax);
    }
    const uint8_t* img = src + (size_t)s * Hs * Ws * 3;      // s in [0, n_src)
    const float* col = color ? color + 4 * k : nullptr;
    if (((x0 | y0 | step) & 255) == 0)                       // per image: a uniform branch
      view_pixels<PX, true>(img, Hs, Ws, x0, y0, step, col, j, i0, res);
    else
      view_pixels<PX, false>(img, Hs, Ws, x0, y0, step, col, j, i0, res);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if constexpr (PX == 4) {
      // Wo % 4 == 0 and out 16-byte aligned: k 3 plane + c plane + j Wo + i0 is a multiple of four floats
      *reinterpret_cast<v4f*>(o + c * plane) = v4f{res[c][0], res[c][1], res[c][2], res[c][3]};
    } else {
      o[c * plane] = res[c][0];
    }
  }
}

}  // namespace
}  // namespace fpsg

extern "C" int fpsg_episode_views(const uint8_t* src, int n_src, int Hs, int Ws, const int32_t* sel, int n,
                                  const int32_t* geom, const float* color, float* out, int Ho, int Wo,
                                  fpsg_stream_t stream) {
  using namespace fpsg;
  static_assert(FPSG_VIEWS_MAX_OFFSET == kOffsetMax && FPSG_VIEWS_MAX_STEP == kStepMax, "the header states the clamps");
  FPSG_REQUIRE(n_src > 0 && Hs > 0 && Ws > 0 && n > 0 && Ho > 0 && Wo > 0, FPSG_E_SHAPE,
               "fpsg_episode_views: n_src,Hs,Ws,n,Ho,Wo must be positive (got %d,%d,%d,%d,%d,%d)", n_src, Hs, Ws, n, Ho,
               Wo);
  FPSG_REQUIRE(Hs <= FPSG_VIEWS_MAX_SIZE && Ws <= FPSG_VIEWS_MAX_SIZE && Ho <= FPSG_VIEWS_MAX_SIZE &&
               Wo <= FPSG_VIEWS_MAX_SIZE && n <= FPSG_VIEWS_MAX_IMAGES, FPSG_E_LIMIT,
               "fpsg_episode_views: Hs,Ws,Ho,Wo <= %d and n <= %d are supported (got %d,%d,%d,%d,%d)",
               FPSG_VIEWS_MAX_SIZE, FPSG_VIEWS_MAX_IMAGES, Hs, Ws, Ho, Wo, n);
  FPSG_REQUIRE(src != nullptr, FPSG_E_NULL, "fpsg_episode_views: null pointer 'src'");
  FPSG_REQUIRE_PTR(sel); FPSG_REQUIRE_PTR(out);
  FPSG_REQUIRE(!misaligned4(geom) && !misaligned4(color), FPSG_E_ALIGN,
               "fpsg_episode_views: 'geom' or 'color' not 4-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool wide = Wo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  const int per_image = Ho * (wide ? Wo / 4 : Wo);           // <= 2^26
  const dim3 grid((unsigned)((per_image + kThreads - 1) / kThreads), (unsigned)n);    // n <= 65535
  if (wide)
    hipLaunchKernelGGL(episode_views_kernel<4>, grid, dim3(kThreads), 0, st, src, n_src, Hs, Ws, sel, geom, color, out,
                       Ho, Wo);
  else
    hipLaunchKernelGGL(episode_views_kernel<1>, grid, dim3(kThreads), 0, st, src, n_src, Hs, Ws, sel, geom, color, out,
                       Ho, Wo);
  return launch_status("fpsg_episode_views");
}
