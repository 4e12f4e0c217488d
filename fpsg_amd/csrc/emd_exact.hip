// emd_exact.hip -- K12: exact Earth Mover's Distance between equal-size clouds (N == M) by a forward auction
// (Bertsekas) with eps-scaling, one workgroup per cloud pair, for gfx950.
// Computes min over permutations a of sum_i |xyz1_i - xyz2_a(i)| -- the quantity K2 (emd.hip, soft assignment) and K2b
// (sinkhorn.hip, entropic) approximate -- together with a certificate: the duality gap of the auction's final prices.
//
// Structure:
//   * bidders are the points of xyz1, objects the points of xyz2, c_ij = |x_i - y_j| (fp32, explicit fmas and
//     v_sqrt_f32); prices start at 0 and only rise;
//   * phases eps_k = eps_0 theta^k (eps_0 = a quarter of the bounding-box diagonal of both clouds, an upper bound of
//     every c_ij; theta = 1/4) down to eps_final; every phase keeps the prices and starts with no assignment;
//   * a round: the unassigned bidders are listed; one wave per listed bidder scans all N objects (lane-strided, one
//     ds_read_b128 per object: x, y, z, price), the best and second-best value c_ij + p_j are folded over the wave with
//     DPP / swizzle lane exchanges; lane 0 bids p_j + (second - best) + eps with a 64-bit LDS atomicMax on
//     (price bits << 32 | ~bidder) -- non-negative floats order as their bits, so the highest bid wins and ties go to
//     the lowest bidder id; then every object with a bid takes its winner and displaces its previous owner;
//   * equal values between objects go to the lowest (j - i) mod N, so that coincident or duplicated points spread their
//     bids over the tied objects instead of all bidding for object 0 (one round instead of N for an all-ties pair);
//   * the result does not depend on the order of the atomics (or of the bidder list): two runs are bit-identical;
//   * bounded work: an intermediate phase stops after kExPhaseRoundsPerPoint * N + 256 rounds and hands its prices to
//     the next one; the call stops after max_rounds rounds in all -- then the unassigned bidders take the free objects
//     in index order (still a permutation) and status = 1.  No spin-wait, no communication between workgroups;
//   * certificate: gap = sum_i [(c_i,a(i) + p_a(i)) - min_j (c_ij + p_j)], which equals cost - D for the LP dual
//     D = sum_i min_j (c_ij + p_j) - sum_j p_j (u_i = min_j (c_ij + p_j), v_j = -p_j: u_i + v_j <= c_ij) -- written
//     term by term it has no cancellation between two large sums, and every term is >= 0 in fp32 (the minimum is over
//     the same fp32 values).  D is a lower bound of the optimum for ANY prices, so cost - gap <= EMD <= cost holds for a
//     capped pair too; a converged pair has gap <= N eps_final (eps-complementary slackness).
// LDS: both clouds + prices (2 x 32 KB as float4 rows), owners, assignment, bidder list (3 x 8 KB), bids (16 KB) at
// N = 2048 = FPSG_EMD_EXACT_MAX_N: 104 KB of the CU's 160 KB, one workgroup of 16 waves per CU.
#include "emd_auction.h"

namespace fpsg {
namespace {

constexpr int kExThreads = 1024;
constexpr int kExWaves = kExThreads / 64;
constexpr int kExMaxN = FPSG_EMD_EXACT_MAX_N;
constexpr int kExStats = 4;                  // ints of per-pair statistics in the workspace

__global__ __launch_bounds__(kExThreads) void emd_exact_kernel(const float* __restrict__ xyz1,
                                                              const float* __restrict__ xyz2, int N, float eps_final,
                                                              int max_rounds, float* __restrict__ cost,
                                                              float* __restrict__ gap, int* __restrict__ assign,
                                                              int* __restrict__ status, float* __restrict__ g1,
                                                              float* __restrict__ g2, int* __restrict__ stats) {
  __shared__ float4 bidders[kExMaxN];                  // x_i (w unused)
  __shared__ float4 objects[kExMaxN];                  // y_j, price p_j in w
  __shared__ int owner[kExMaxN];                       // object -> bidder, -1 free
  __shared__ int asg[kExMaxN];                         // bidder -> object, -1 unassigned
  __shared__ int list[kExMaxN];                        // unassigned bidders of the round
  __shared__ unsigned long long bid[kExMaxN];          // best bid of the round per object, 0 = none
  __shared__ int cnt[2];
  __shared__ float wred[kExWaves][6];

  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float* __restrict__ p1 = xyz1 + (size_t)b * N * 3;
  const float* __restrict__ p2 = xyz2 + (size_t)b * N * 3;

  // stage both clouds, prices 0; bounding box of their union -> eps_0
  float lo[3], hi[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) { lo[d] = __builtin_inff(); hi[d] = -__builtin_inff(); }
  for (int i = tid; i < N; i += kExThreads) {
    const float ax = p1[i * 3], ay = p1[i * 3 + 1], az = p1[i * 3 + 2];
    const float bx = p2[i * 3], by = p2[i * 3 + 1], bz = p2[i * 3 + 2];
    bidders[i] = make_float4(ax, ay, az, 0.0f);
    objects[i] = make_float4(bx, by, bz, 0.0f);
    lo[0] = __builtin_fminf(lo[0], __builtin_fminf(ax, bx)); hi[0] = __builtin_fmaxf(hi[0], __builtin_fmaxf(ax, bx));
    lo[1] = __builtin_fminf(lo[1], __builtin_fminf(ay, by)); hi[1] = __builtin_fmaxf(hi[1], __builtin_fmaxf(ay, by));
    lo[2] = __builtin_fminf(lo[2], __builtin_fminf(az, bz)); hi[2] = __builtin_fmaxf(hi[2], __builtin_fmaxf(az, bz));
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    fold_minmax_wave(lo[d], hi[d]);
  }
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { wred[wave][d] = lo[d]; wred[wave][3 + d] = hi[d]; }
  }
  __syncthreads();
  float ext[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    float l = wred[0][d], h = wred[0][3 + d];
    for (int w = 1; w < kExWaves; ++w) { l = __builtin_fminf(l, wred[w][d]); h = __builtin_fmaxf(h, wred[w][3 + d]); }
    ext[d] = h - l;
  }
  const float eps0 = ex_eps0(ext, eps_final);
  const int phase_cap = ex_phase_cap(N);

  int rounds = 0, phases = 0, last_rounds = 0;
  bool capped = false;
  float eps = eps0;
  for (;;) {                                           // phases
    const bool final_phase = !(eps > eps_final);
    if (final_phase) eps = eps_final;
    for (int i = tid; i < N; i += kExThreads) { asg[i] = -1; owner[i] = -1; bid[i] = 0ull; }
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    __syncthreads();
    int r = 0;
    for (;;) {                                         // rounds; every thread takes the same branches
      int* c = &cnt[r & 1];
      for (int i = tid; i < N; i += kExThreads)
        if (asg[i] < 0) list[atomicAdd(c, 1)] = i;
      if (tid == 0) cnt[(r + 1) & 1] = 0;              // read last in the previous round, before two barriers
      __syncthreads();
      const int U = *c;
      if (U == 0) break;                               // every bidder holds an object: the phase is done
      if (rounds >= max_rounds) { capped = true; break; }
      if (!final_phase && r >= phase_cap) break;       // the next phase starts from these prices
      // bids: one wave per unassigned bidder
      for (int k = wave; k < U; k += kExWaves) {
        const int i = list[k];
        const float4 xi = bidders[i];
        float b1 = __builtin_inff(), b2 = __builtin_inff();
        int r1 = 0x7fffffff;
        for (int j = lane; j < N; j += 64) {
          const float4 o = objects[j];
          ex_scan(ex_cost(xi.x, xi.y, xi.z, o.x, o.y, o.z) + o.w, ex_rank(j, i, N), b1, r1, b2);
        }
        fold_best2<1>(b1, r1, b2); fold_best2<2>(b1, r1, b2); fold_best2<4>(b1, r1, b2);
        fold_best2<8>(b1, r1, b2); fold_best2<16>(b1, r1, b2); fold_best2<32>(b1, r1, b2);
        if (lane == 0) {
          const int j1 = ex_unrank(r1, i, N);
          if (N == 1) b2 = b1;                         // no second object
          const float pj = objects[j1].w;
          const unsigned bits = ex_bid_bits(pj, b1, b2, eps);
          atomicMax(&bid[j1], ex_bid_key(bits, i));
        }
      }
      __syncthreads();
      // assignment: winners (unassigned bidders) displace the owners (assigned bidders): disjoint sets, no race
      for (int j = tid; j < N; j += kExThreads) {
        const unsigned long long key = bid[j];
        if (key) {
          const int w = ex_key_bidder(key);
          const int o = owner[j];
          if (o >= 0) asg[o] = -1;
          owner[j] = w;
          asg[w] = j;
          objects[j].w = ex_key_price(key);
          bid[j] = 0ull;
        }
      }
      __syncthreads();
      ++r;
      ++rounds;
    }
    ++phases;
    last_rounds = r;
    if (final_phase || capped) break;
    eps = eps * kExTheta;
  }

  if (capped) {                                        // complete the permutation: free objects in index order
    if (tid == 0) ex_complete(owner, asg, N);
    __syncthreads();
  }

  // cost, certificate, assignment and gradients: one bidder per thread (the object reads are broadcasts)
  float csum = 0.0f, gsum = 0.0f;
  for (int i = tid; i < N; i += kExThreads) {
    const float4 xi = bidders[i];
    float u = __builtin_inff();
    for (int j = 0; j < N; ++j) {
      const float4 o = objects[j];
      u = __builtin_fminf(u, ex_cost(xi.x, xi.y, xi.z, o.x, o.y, o.z) + o.w);
    }
    const int j = asg[i];
    const float4 o = objects[j];
    const float cij = ex_cost(xi.x, xi.y, xi.z, o.x, o.y, o.z);
    csum += cij;
    gsum += (cij + o.w) - u;
    assign[(size_t)b * N + i] = j;
    if (g1 || g2) {
      float gx = 0.0f, gy = 0.0f, gz = 0.0f;
      if (cij > 0.0f) { gx = (xi.x - o.x) / cij; gy = (xi.y - o.y) / cij; gz = (xi.z - o.z) / cij; }
      if (g1) {
        float* q = g1 + ((size_t)b * N + i) * 3;
        q[0] = gx; q[1] = gy; q[2] = gz;
      }
      if (g2) {
        float* q = g2 + ((size_t)b * N + j) * 3;
        q[0] = -gx; q[1] = -gy; q[2] = -gz;
      }
    }
  }
  csum = wave_sum(csum);                               // fixed trees: deterministic
  gsum = wave_sum(gsum);
  __syncthreads();                                     // (wred was last read before the phases)
  if (lane == 0) { wred[wave][0] = csum; wred[wave][1] = gsum; }
  __syncthreads();
  if (tid == 0) {
    float ct = 0.0f, gt = 0.0f;
    for (int w = 0; w < kExWaves; ++w) { ct += wred[w][0]; gt += wred[w][1]; }
    cost[b] = ct;
    gap[b] = gt;
    status[b] = capped ? 1 : 0;
    int* s = stats + (size_t)b * kExStats;
    s[0] = rounds;
    s[1] = last_rounds;
    s[2] = phases;
    s[3] = (int)__float_as_uint(eps0);
  }
}

}  // namespace
}  // namespace fpsg

extern "C" size_t fpsg_emd_exact_workspace_floats(int B, int N) {
  if (B <= 0 || N <= 0 || N > FPSG_EMD_EXACT_MAX_N) return 0;
  return (size_t)B * fpsg::kExStats;
}

extern "C" int fpsg_emd_exact(const float* xyz1, const float* xyz2, int B, int N, float eps_final, int max_rounds,
                              float* cost, float* gap, int* assign, int* status, float* gxyz1, float* gxyz2, float* ws,
                              fpsg_stream_t stream) {
  using namespace fpsg;
  FPSG_REQUIRE_PTR(xyz1); FPSG_REQUIRE_PTR(xyz2); FPSG_REQUIRE_PTR(cost); FPSG_REQUIRE_PTR(gap);
  FPSG_REQUIRE_PTR(assign); FPSG_REQUIRE_PTR(status); FPSG_REQUIRE_PTR(ws);
  FPSG_REQUIRE(B > 0 && N > 0, FPSG_E_SHAPE, "fpsg_emd_exact: B,N must be positive (got %d,%d)", B, N);
  FPSG_REQUIRE(N <= FPSG_EMD_EXACT_MAX_N, FPSG_E_SHAPE,
               "fpsg_emd_exact: N=%d exceeds the supported maximum of %d points", N, FPSG_EMD_EXACT_MAX_N);
  FPSG_REQUIRE(B <= 2147483647 / N, FPSG_E_SHAPE, "fpsg_emd_exact: B*N=%d*%d overflows", B, N);
  FPSG_REQUIRE(eps_final > 0.0f && eps_final < __builtin_inff(), FPSG_E_SHAPE,
               "fpsg_emd_exact: eps_final must be positive and finite (got %g)", (double)eps_final);
  FPSG_REQUIRE(max_rounds >= 1, FPSG_E_SHAPE, "fpsg_emd_exact: max_rounds must be at least 1 (got %d)", max_rounds);
  FPSG_REQUIRE(!misaligned4(gxyz1) && !misaligned4(gxyz2), FPSG_E_ALIGN,
               "fpsg_emd_exact: gradient buffers must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(emd_exact_kernel, dim3(B), dim3(kExThreads), 0, s, xyz1, xyz2, N, eps_final, max_rounds, cost,
                     gap, assign, status, gxyz1, gxyz2, reinterpret_cast<int*>(ws));
  return launch_status("fpsg_emd_exact");
}
