// chamfer_cross.hip -- K13, the all-pairs Chamfer matrix between two sets of clouds: for xyz1 [Na,N,3] and
// xyz2 [Nb,M,3],  out[a][b] = mean_i min_j d(a_i, b_j) + mean_j min_i d(b_j, a_i)  (metrics.chamfer_distance of the
// pair, Kaolin 0.9.0's convention), for the set-level generation metrics (MMD, COV, 1-NNA; fpsg_amd/set_metrics.py).
// gfx950 (MI355X).  Forward only: no indices, no per-point outputs, no workspace.
//
// d is K1's (chamfer_dist.h, the same packed block), so every per-point minimum equals K1's dist1 / dist2 bit for bit.
//
//   chamfer_cross_kernel<R>: a workgroup of 256 lanes owns cloud a: lane t holds rows t*R .. t*R+R-1 in VGPRs
//     (R = rows_per_lane(N): 2, 4, 8, 16 for N up to 512, 1024, 2048, 4096; padded rows never win).  It walks a run
//     of TB pairs (below); each cloud b is staged in LDS as SoA (+inf padded to a multiple of 16) and scanned in
//     chunks of 16 candidates by all four waves:
//       rows:    each lane keeps its rows' running minima in registers (v_min3, 0.5 instructions per distance);
//       columns: each lane keeps the minimum over its R rows per candidate (v_min3, 0.5 per distance); a wave-private
//                LDS transpose and two lane swaps give the wave's minimum per candidate, and the four waves meet in
//                an LDS ds_min_u32 on the float bits (the values are >= 0, so the integer order is the float order;
//                a minimum does not depend on the order of its operands, so the integer atomic is deterministic).
//     Then both sums are formed by one canonical function of the per-point minima of a cloud of n points:
//     lane t adds the minima of points t*K .. t*K+K-1, K = rows_per_lane(n), in ascending order,
//     and the 256 partial sums meet in a fixed tree (the xor butterfly of wave_sum in each wave, then
//     (w0 + w1) + (w2 + w3)).  The row side already has that layout in registers; the column side reads its minima
//     from LDS in it.  out = S_rows / N + S_cols / M.
//
// Summation order (the only difference from chamfer_distance, which sums each direction in torch's mean): the
// canonical sum above.  Consequences, all bitwise: an entry does not depend on Na, Nb, the slice or the launch it was
// computed in (one workgroup forms it, with fixed functions of its two clouds); chamfer_matrix(B, A) equals
// chamfer_matrix(A, B)^T (d is bit-symmetric, the two terms are formed by the same function whichever argument their
// points came from, and the final fp32 addition commutes); the symmetric mode (xyz2 == NULL) evaluates each
// unordered pair a < b once, writes it to [a][b] and [b][a], and writes an exact 0 to [a][a] -- what the full mode
// computes for A against itself (d(p,p) = 0).
//
// Work: the pairs are numbered row-major, (a, b) for b in [0, Nb) (symmetric mode: the upper triangle a < b), and
// workgroup w takes pairs [w*TB, w*TB + TB), reloading cloud a's rows when its run crosses into the next row, so every
// workgroup has the same work (a symmetric grid of row chunks leaves whole XCDs idle at the end).  TB =
// clamp(ceil(pairs / 4096), 1, 16); launches are split at 2^22 workgroups, so any Na x Nb fits a one-dimensional grid.
// Symmetric mode: workgroup w also writes the diagonal entries w, w + W, w + 2W, ... (W workgroups in all).
#include "chamfer_dist.h"
#include "fpsg_common.h"

namespace fpsg {
namespace {

constexpr int kXThreads = 256;         // lanes per workgroup (the canonical sum's fixed width)
constexpr int kXWaves = kXThreads / kWave;
constexpr int kXChunk = 16;            // candidates per chunk
constexpr int kXTStride = 20;          // floats per lane in the transpose buffer (16 + pad, 16-B aligned)
constexpr float kXRowPad = 3.0e38f;    // coordinates of padded rows: every distance overflows to +inf
constexpr unsigned kInfBits = 0x7f800000u;
constexpr long long kXMaxGrid = 1ll << 22;

__host__ __device__ constexpr int rows_per_lane(int n) { return n <= 512 ? 2 : n <= 1024 ? 4 : n <= 2048 ? 8 : 16; }

// Sum over the workgroup of one value per lane in a fixed tree; the total is returned to thread 0.
__device__ __forceinline__ void block_sum2(float& s0, float& s1, float* red) {
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) { red[2 * (tid >> 6)] = s0; red[2 * (tid >> 6) + 1] = s1; }
  __syncthreads();
  if (tid == 0) {
    s0 = (red[0] + red[2]) + (red[4] + red[6]);
    s1 = (red[1] + red[3]) + (red[5] + red[7]);
  }
}

// LDS: [3][Mp] candidate SoA | [Mp] column minima (float bits) | [4][64][kXTStride] transpose buffers | [8] sums
template <int R>
__global__ __launch_bounds__(kXThreads) void chamfer_cross_kernel(
    const float* __restrict__ xyz1, const float* __restrict__ xyz2, int Na, int Nb, int N, int M, int TB,
    long long npairs, long long nwg, long long base, int sym, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const long long work = base + blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (sym && tid == 0)
    for (long long d = work; d < Na; d += nwg) out[(size_t)d * Na + d] = 0.0f;
  const long long p0 = work * TB;
  const long long p1 = p0 + TB < npairs ? p0 + TB : npairs;
  if (p0 >= p1) return;                                  // uniform: before any barrier
  // the first pair (a, b) of the run
  int a, b;
  if (!sym) {
    a = (int)(p0 / Nb);
    b = (int)(p0 - (long long)a * Nb);
  } else {                                               // row a starts at pair a * (2 Na - a - 1) / 2
    auto row_start = [Na](long long r) { return r * (2ll * Na - r - 1) / 2; };
    const double q = 2.0 * Na - 1.0;
    long long r = (long long)((q - sqrt(fmax(q * q - 8.0 * (double)p0, 0.0))) * 0.5);
    r = r < 0 ? 0 : (r > Na - 2 ? Na - 2 : r);
    while (r > 0 && row_start(r) > p0) --r;
    while (r < Na - 2 && row_start(r + 1) <= p0) ++r;
    a = (int)r;
    b = (int)(p0 - row_start(r)) + a + 1;
  }

  const int Mp = (M + kXChunk - 1) / kXChunk * kXChunk;
  float* lx = lds;
  float* ly = lds + Mp;
  float* lz = lds + 2 * Mp;
  unsigned* colmin = reinterpret_cast<unsigned*>(lds + 3 * Mp);
  float* tbuf = lds + 4 * Mp + wave * (kWave * kXTStride);
  float* red = lds + 4 * Mp + kXWaves * kWave * kXTStride;

  static_assert(R % 2 == 0, "rows are kept as register pairs");
  const int row0 = tid * R;
  v2f qx[R / 2], qy[R / 2], qz[R / 2];
  const int KM = rows_per_lane(M);
  const int seg = lane >> 4;                             // 16-lane segment whose partials this lane reduces
  const int cl = lane & 15;                              // candidate of the chunk this lane reduces
  const int row_end = sym ? Na : Nb;

  for (long long p = p0, loaded = -1; p < p1; ++p) {
    if (a != loaded) {                                   // this lane's R rows of cloud a (.x = row 2p, .y = row 2p + 1)
      loaded = a;
      const float* __restrict__ src = xyz1 + ((size_t)a * N + row0) * 3;
      float f[3 * R];
#pragma unroll
      for (int e = 0; e < 3 * R; ++e) f[e] = (row0 + e / 3 < N) ? src[e] : kXRowPad;
#pragma unroll
      for (int p2 = 0; p2 < R / 2; ++p2) {
        qx[p2].x = f[6 * p2 + 0]; qy[p2].x = f[6 * p2 + 1]; qz[p2].x = f[6 * p2 + 2];
        qx[p2].y = f[6 * p2 + 3]; qy[p2].y = f[6 * p2 + 4]; qz[p2].y = f[6 * p2 + 5];
      }
    }
    __syncthreads();                                     // the previous cloud's readers are done
    {
      const float* __restrict__ src = xyz2 + (size_t)b * M * 3;
      for (int e = tid; e < 3 * Mp; e += kXThreads) {
        const int j = e / 3;
        const int k = e - 3 * j;
        lds[k * Mp + j] = e < 3 * M ? src[e] : __builtin_inff();
      }
      for (int j = tid; j < Mp; j += kXThreads) colmin[j] = kInfBits;
    }
    __syncthreads();

    float best[R];
#pragma unroll
    for (int r = 0; r < R; ++r) best[r] = __builtin_inff();

    for (int cbase = 0; cbase < Mp; cbase += kXChunk) {
      float cp[kXChunk];
#pragma unroll
      for (int u = 0; u < kXChunk; ++u) cp[u] = __builtin_inff();
      const v4f* px = reinterpret_cast<const v4f*>(lx + cbase);
      const v4f* py = reinterpret_cast<const v4f*>(ly + cbase);
      const v4f* pz = reinterpret_cast<const v4f*>(lz + cbase);
#pragma unroll
      for (int g = 0; g < kXChunk / 4; ++g) {
        const v4f X = px[g], Y = py[g], Z = pz[g];
#pragma unroll
        for (int p2 = 0; p2 < R / 2; ++p2) {
          v2f a01, a23, b01, b23;
          dist_2rows_4cands(X, Y, Z, qx[p2], qy[p2], qz[p2], a01, a23, b01, b23);
          best[2 * p2] = __builtin_fminf(__builtin_fminf(best[2 * p2], a01.x), a01.y);
          best[2 * p2] = __builtin_fminf(__builtin_fminf(best[2 * p2], a23.x), a23.y);
          best[2 * p2 + 1] = __builtin_fminf(__builtin_fminf(best[2 * p2 + 1], b01.x), b01.y);
          best[2 * p2 + 1] = __builtin_fminf(__builtin_fminf(best[2 * p2 + 1], b23.x), b23.y);
          cp[4 * g + 0] = __builtin_fminf(__builtin_fminf(cp[4 * g + 0], a01.x), b01.x);
          cp[4 * g + 1] = __builtin_fminf(__builtin_fminf(cp[4 * g + 1], a01.y), b01.y);
          cp[4 * g + 2] = __builtin_fminf(__builtin_fminf(cp[4 * g + 2], a23.x), b23.x);
          cp[4 * g + 3] = __builtin_fminf(__builtin_fminf(cp[4 * g + 3], a23.y), b23.y);
        }
      }
      // ---- columns: transpose the 64 x 16 partial minima through the wave's LDS buffer (one wave's LDS operations
      // execute in order, so the reads see the stores without a barrier), then the segments meet by lane swaps
      {
        v4f* tw = reinterpret_cast<v4f*>(tbuf + lane * kXTStride);
#pragma unroll
        for (int u = 0; u < kXChunk / 4; ++u) {
          const v4f v = {cp[4 * u + 0], cp[4 * u + 1], cp[4 * u + 2], cp[4 * u + 3]};
          tw[u] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const float* tr = tbuf + (seg * 16) * kXTStride + cl;
        float vt[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) vt[t] = tr[t * kXTStride];
        __builtin_amdgcn_wave_barrier();                 // the next chunk's stores come after these reads
        float v = __builtin_inff();
#pragma unroll
        for (int t = 0; t < 16; t += 2) v = __builtin_fminf(__builtin_fminf(v, vt[t]), vt[t + 1]);
        v = __builtin_fminf(v, lane_xor_f<16>(v));
        v = __builtin_fminf(v, lane_xor_f<32>(v));
        if (lane < 16) atomicMin(&colmin[cbase + cl], __float_as_uint(v));
      }
    }
    __syncthreads();                                     // every wave's column minima are in

    // ---- the two canonical sums: lane t adds the minima of points t*K .. t*K+K-1 in ascending order
    float srow = 0.0f, scol = 0.0f;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (row0 + r < N) srow += best[r];
    for (int k = 0; k < KM; ++k) {
      const int j = tid * KM + k;
      if (j < M) scol += __uint_as_float(colmin[j]);
    }
    block_sum2(srow, scol, red);
    if (tid == 0) {
      const float v = srow / (float)N + scol / (float)M;
      out[(size_t)a * Nb + b] = v;
      if (sym) out[(size_t)b * Na + a] = v;
    }
    if (++b == row_end) {
      ++a;
      b = sym ? a + 1 : 0;
    }
  }
}

template <int R>
int launch_cross(const float* xyz1, const float* xyz2, int Na, int Nb, int N, int M, int sym, float* out,
                 hipStream_t s) {
  const long long pairs = sym ? (long long)Na * (Na - 1) / 2 : (long long)Na * Nb;
  const int TB = (int)(pairs <= 4096 ? 1 : pairs >= 16 * 4096 ? 16 : (pairs + 4095) / 4096);
  const long long total = pairs > 0 ? (pairs + TB - 1) / TB : 1;      // (Na = 1, symmetric: the diagonal alone)
  const int Mp = (M + kXChunk - 1) / kXChunk * kXChunk;
  const size_t lds = (size_t)(4 * Mp + kXWaves * kWave * kXTStride + 2 * kXWaves) * sizeof(float);
  if (lds > 65536) {                                   // dynamic LDS beyond 64 KiB has to be requested (M > 3072)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(chamfer_cross_kernel<R>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { set_error("fpsg_chamfer_cross: %s", hipGetErrorString(e)); return (int)e; }
  }
  for (long long base = 0; base < total; base += kXMaxGrid) {
    const long long n = total - base < kXMaxGrid ? total - base : kXMaxGrid;
    hipLaunchKernelGGL(chamfer_cross_kernel<R>, dim3((unsigned)n), dim3(kXThreads), lds, s, xyz1, xyz2, Na, Nb, N, M,
                       TB, pairs, total, base, sym, out);
    const int rc = launch_status("fpsg_chamfer_cross");
    if (rc) return rc;
  }
  return 0;
}

}  // namespace
}  // namespace fpsg

extern "C" int fpsg_chamfer_cross(const float* xyz1, const float* xyz2, int Na, int Nb, int N, int M, float* out,
                                  fpsg_stream_t stream) {
  using namespace fpsg;
  FPSG_REQUIRE_PTR(xyz1); FPSG_REQUIRE_PTR(out);
  const int sym = xyz2 == nullptr;
  if (!sym) FPSG_REQUIRE(!misaligned4(xyz2), FPSG_E_ALIGN, "fpsg_chamfer_cross: 'xyz2' not 4-byte aligned");
  FPSG_REQUIRE(Na > 0 && Nb > 0 && N > 0 && M > 0, FPSG_E_SHAPE,
               "fpsg_chamfer_cross: Na,Nb,N,M must be positive (got %d,%d,%d,%d)", Na, Nb, N, M);
  FPSG_REQUIRE(!sym || (Nb == Na && M == N), FPSG_E_SHAPE,
               "fpsg_chamfer_cross: symmetric mode (xyz2 = NULL) needs Nb = Na and M = N (got %d,%d and %d,%d)", Nb,
               Na, M, N);
  FPSG_REQUIRE(N <= FPSG_CHAMFER_CROSS_MAX_N && M <= FPSG_CHAMFER_CROSS_MAX_N, FPSG_E_LIMIT,
               "fpsg_chamfer_cross: clouds of %d and %d points exceed the limit of %d points", N, M,
               FPSG_CHAMFER_CROSS_MAX_N);
  if (sym) xyz2 = xyz1;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (rows_per_lane(N)) {
    case 2: return launch_cross<2>(xyz1, xyz2, Na, Nb, N, M, sym, out, s);
    case 4: return launch_cross<4>(xyz1, xyz2, Na, Nb, N, M, sym, out, s);
    case 8: return launch_cross<8>(xyz1, xyz2, Na, Nb, N, M, sym, out, s);
    default: return launch_cross<16>(xyz1, xyz2, Na, Nb, N, M, sym, out, s);
  }
}
