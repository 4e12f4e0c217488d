// fps.hip -- K16: farthest point sampling, for gfx950.  The definition is in include/fpsg_hip.h (K16) and DESIGN.md:
// per cloud, n dependent rounds; every round picks the lowest index at which D (the squared distance to the nearest
// pick so far, fpsg::sq_dist of chamfer_dist.h, the bits of K1 and K13) is largest.
//
// Structure:
//   * one workgroup per cloud, T threads chosen from N; thread `tid` owns the points tid, tid + T, ... (P of them):
//     their coordinates and their D stay in registers for the whole call, 4 P VGPRs;
//   * a round: D = min(D, d(., last pick)) and the thread's best key, the key being (bits(D) << 32) | ~index -- D >= 0,
//     so its bits order as an unsigned integer, and one 64-bit max gives "largest D, lowest index";
//   * the key is maximised over the wave in registers (DPP, swizzle, half-wave swap); the lane that owns the wave's best
//     publishes the key WITH that point's coordinates in the wave's LDS slot; one barrier; every wave reads the slots,
//     one per lane, maximises over them in registers again and takes the winner's coordinates from the winner's lane
//     with v_readlane: they arrive as scalars, which is what the next round's distances need;
//   * the slots are double-buffered, so a round has ONE barrier, and that barrier waits for LDS only: the stores of
//     idx and min_dist (lane 0 of wave 0, ordinary vector stores) are never waited for inside the loop;
//   * a cloud of at most 256 points is one wave: no LDS, no barrier.
//   The loop runs n - 1 times whatever the data; a padding slot (index >= N) has D = 0 and the lowest key of all.
#include "chamfer_dist.h"
#include "fpsg_common.h"

namespace fpsg {
namespace {

typedef unsigned v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float fps_readlane(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

constexpr int fps_log2(int v) { return v <= 1 ? 0 : 1 + fps_log2(v >> 1); }

template <int T, int P>
__global__ __launch_bounds__(T) void fps_kernel(const float* __restrict__ xyz, int N, int n,
                                                const int* __restrict__ start, int* __restrict__ idx,
                                                float* __restrict__ min_dist) {
  constexpr int W = T / 64;                            // waves, a power of two up to 16
  constexpr int LOG_T = fps_log2(T);
  __shared__ v4u slot_kxy[2][W];                       // per wave: key (low, high), x, y of its best point
  __shared__ float slot_z[2][W];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float* cloud = xyz + (size_t)blockIdx.x * (size_t)N * 3;
  int* out_idx = idx + (size_t)blockIdx.x * (size_t)n;
  float* out_md = min_dist ? min_dist + (size_t)blockIdx.x * (size_t)n : nullptr;

  float x[P], y[P], z[P], D[P];
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const int i = tid + k * T;
    const bool in = i < N;
    const float* p = cloud + (size_t)(in ? i : 0) * 3;
    x[k] = p[0]; y[k] = p[1]; z[k] = p[2];
    D[k] = in ? __builtin_inff() : 0.0f;               // min(+inf, d) = d: the first round sets D = d(., idx[0])
  }

  int s = start ? start[blockIdx.x] : 0;
  s = s < 0 ? 0 : s > N - 1 ? N - 1 : s;               // a start outside the cloud is clamped, never followed
  s = __builtin_amdgcn_readfirstlane(s);
  float sx = cloud[(size_t)s * 3], sy = cloud[(size_t)s * 3 + 1], sz = cloud[(size_t)s * 3 + 2];
  if (tid == 0) {
    out_idx[0] = s;
    if (out_md) out_md[0] = __builtin_inff();
  }

  const unsigned nbase = ~(unsigned)tid;               // ~(tid + k T) = nbase - k T
  for (int t = 1; t < n; ++t) {
    unsigned long long best = 0ull;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      D[k] = __builtin_fminf(D[k], sq_dist(sx, sy, sz, x[k], y[k], z[k]));
      const unsigned long long key = ((unsigned long long)__float_as_uint(D[k]) << 32) | (nbase - (unsigned)(k * T));
      best = key > best ? key : best;
    }
    const unsigned long long wbest = group_max_u64<64>(best);
    // the coordinates of this thread's best point (a select chain: a run-time register index would go to scratch)
    const int kb = (int)(~(unsigned)best >> LOG_T);
    float bx = x[0], by = y[0], bz = z[0];
#pragma unroll
    for (int k = 1; k < P; ++k) {
      const bool hit = kb == k;
      bx = hit ? x[k] : bx; by = hit ? y[k] : by; bz = hit ? z[k] : bz;
    }
    unsigned long long win;
    if (W == 1) {
      win = wbest;
      const int owner = __builtin_amdgcn_readfirstlane((int)(~(unsigned)win & 63u));
      sx = fps_readlane(bx, owner); sy = fps_readlane(by, owner); sz = fps_readlane(bz, owner);
    } else {
      const int buf = t & 1;
      if (best == wbest) {                             // one lane: the indices in the keys are distinct
        slot_kxy[buf][wave] = v4u{(unsigned)best, (unsigned)(best >> 32), __float_as_uint(bx), __float_as_uint(by)};
        slot_z[buf][wave] = bz;
      }
      // LDS only: the barrier must not wait for the stores of idx and min_dist below
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const v4u sl = slot_kxy[buf][lane & (W - 1)];
      const float slz = slot_z[buf][lane & (W - 1)];
      win = group_max_u64<W>(((unsigned long long)sl.y << 32) | sl.x);
      // index = tid + k T: the winner's wave, whose slot lane `owner` has just read
      const unsigned wi = (unsigned)__builtin_amdgcn_readfirstlane((int)~(unsigned)win);
      const int owner = (int)((wi & (unsigned)(T - 1)) >> 6);
      sx = fps_readlane(__uint_as_float(sl.z), owner);
      sy = fps_readlane(__uint_as_float(sl.w), owner);
      sz = fps_readlane(slz, owner);
    }
    if (tid == 0) {
      const int wi = (int)~(unsigned)win;
      out_idx[t] = wi < N ? wi : N - 1;                // always in range, whatever the coordinates hold
      if (out_md) out_md[t] = __uint_as_float((unsigned)(win >> 32));
    }
  }
}

template <int T, int P>
void fps_launch(const float* xyz, int B, int N, int n, const int* start, int* idx, float* min_dist,
                hipStream_t stream) {
  hipLaunchKernelGGL((fps_kernel<T, P>), dim3((unsigned)B), dim3(T), 0, stream, xyz, N, n, start, idx, min_dist);
}

}  // namespace
}  // namespace fpsg

extern "C" size_t fpsg_fps_workspace_bytes(int B, int N, int n) {
  return 0;                                            // registers and a few LDS slots: nothing in memory
}

extern "C" int fpsg_fps(const float* xyz, int B, int N, int n, const int32_t* start, int32_t* idx, float* min_dist,
                        void* ws, size_t ws_bytes, fpsg_stream_t stream) {
  using namespace fpsg;
  FPSG_REQUIRE(B > 0 && N > 0, FPSG_E_SHAPE, "fpsg_fps: B,N must be positive (got %d,%d)", B, N);
  FPSG_REQUIRE(n >= 1 && n <= N, FPSG_E_SHAPE, "fpsg_fps: n must be from 1 to N=%d (got %d)", N, n);
  FPSG_REQUIRE(N <= FPSG_FPS_MAX_N, FPSG_E_LIMIT, "fpsg_fps: N=%d exceeds the supported maximum of %d", N,
               FPSG_FPS_MAX_N);
  FPSG_REQUIRE_PTR(xyz); FPSG_REQUIRE_PTR(idx);
  FPSG_REQUIRE(!misaligned4(start), FPSG_E_ALIGN, "fpsg_fps: 'start' not 4-byte aligned");
  FPSG_REQUIRE(!misaligned4(min_dist), FPSG_E_ALIGN, "fpsg_fps: 'min_dist' not 4-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  // threads per cloud from N: T P >= N
  if (N <= 64) fps_launch<64, 1>(xyz, B, N, n, start, idx, min_dist, st);
  else if (N <= 256) fps_launch<64, 4>(xyz, B, N, n, start, idx, min_dist, st);
  else if (N <= 1024) fps_launch<256, 4>(xyz, B, N, n, start, idx, min_dist, st);
  else if (N <= 2048) fps_launch<512, 4>(xyz, B, N, n, start, idx, min_dist, st);
  else if (N <= 4096) fps_launch<1024, 4>(xyz, B, N, n, start, idx, min_dist, st);
  else if (N <= 8192) fps_launch<1024, 8>(xyz, B, N, n, start, idx, min_dist, st);
  else fps_launch<1024, 16>(xyz, B, N, n, start, idx, min_dist, st);
  return launch_status("fpsg_fps");
}
