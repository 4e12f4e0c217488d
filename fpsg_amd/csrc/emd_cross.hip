// emd_cross.hip -- K14: the all-pairs exact EMD matrix, out[a][b] = the exact EMD of (xyz1[a], xyz2[b]) for every
// pair in one call, shaped for throughput, for gfx950.  The auction is K12's (emd_auction.h): every bid is computed bit
// for bit as K12 computes it, and a Jacobi auction's trajectory does not depend on the number of waves that compute
// its bids nor on the order of the bidder list or of the atomics, so a pair ends with K12's rounds, status, prices and
// assignment; cost and gap are summed in K12's order and are bitwise K12's.
//
// Structure:
//   * one workgroup of 4 waves per pair (K12: 16); persistent workgroups take the next pair from a 64-bit counter in
//     the call's workspace (zeroed on the call's stream before the launch), so pairs of unequal length balance;
//   * the objects' coordinates live in registers: lane l of every wave holds objects l, l + 64, ... (T per lane), the
//     objects a lane scans in K12's lane-strided loop, in the same order; only the prices are in LDS.  The bidders'
//     coordinates are read from global memory (scalar loads, one bidder per wave);
//   * the bidder list of a round is built from the previous round: the bidders that lost and the owners displaced by
//     the winners (K12 rescans all N bidders).  After the bids, each listed bidder reads the key of the object it
//     bid on; the bidder it names takes the object.  Two barriers per round (K12: three), no pass over the N objects;
//   * bids are not cleared between rounds: a bid is always above its object's price and prices only rise, so a key
//     left by an earlier round never beats a new bid; and only the bidder a key names, which bid on that object in
//     this round, acts on it, so owners stay a partial matching whatever the input;
//   * the assignment is derived from the owners at the end; a capped pair is completed as in K12.
// LDS per pair: bids (8 B), prices, owners (4 B each), two bidder lists (8 B) per point: 24 N bytes, 48 KB at
// N = 2048 (K12: 104 KB).  The prices are padded to 64 T with +inf, so the scans need no bounds test.
#include "emd_auction.h"

namespace fpsg {
namespace {

constexpr int kEcThreads = 256;
constexpr int kEcWaves = kEcThreads / 64;
constexpr int kEcSumWaves = 16;                        // K12's waves: the cost and gap sums follow its order

// T objects per lane: N <= 64 T.
template <int T>
__global__ __launch_bounds__(kEcThreads) void emd_cross_kernel(const float* __restrict__ xyz1,
                                                              const float* __restrict__ xyz2, int Na, int Nb, int N,
                                                              float eps_final, int max_rounds, int sym,
                                                              long long pairs, float* __restrict__ cost,
                                                              float* __restrict__ gap, int* __restrict__ status,
                                                              int* __restrict__ rounds_out,
                                                              unsigned long long* __restrict__ counter) {
  extern __shared__ __align__(16) unsigned char ec_smem[];
  unsigned long long* bid = reinterpret_cast<unsigned long long*>(ec_smem);   // [N] best bid per object
  float* price = reinterpret_cast<float*>(bid + N);                          // [64 T], +inf beyond N
  int* owner = reinterpret_cast<int*>(price + 64 * T);                       // [N] object -> bidder, -1 free
  int* lists = owner + N;                                                    // [2][N] bidder lists
  __shared__ int cnt[2];
  __shared__ long long next_pair;
  __shared__ float wext[kEcWaves][6];
  __shared__ float wred[kEcSumWaves][2];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  if (sym) {                                           // the diagonal: exact zeros, not solved
    for (long long a = (long long)blockIdx.x * kEcThreads + tid; a < Na; a += (long long)gridDim.x * kEcThreads) {
      const size_t e = (size_t)a * Na + a;
      cost[e] = 0.0f;
      gap[e] = 0.0f;
      status[e] = 0;
      if (rounds_out) rounds_out[e] = 0;
    }
  }

  for (;;) {
    if (tid == 0) next_pair = (long long)atomicAdd(counter, 1ull);
    __syncthreads();                                   // (every thread passes barriers of the previous pair first)
    const long long p = next_pair;
    if (p >= pairs) break;
    long long a, b;
    if (sym) {                                         // upper triangle, row-major: row a starts at a (2 Na - a - 1) / 2
      const double m = 2.0 * Na - 1.0;
      a = (long long)((m - __builtin_sqrt(m * m - 8.0 * (double)p)) * 0.5);
      if (a < 0) a = 0;
      if (a > Na - 2) a = Na - 2;
      while (a > 0 && a * (2LL * Na - a - 1) / 2 > p) --a;
      while (a < Na - 2 && (a + 1) * (2LL * Na - a - 2) / 2 <= p) ++a;
      b = p - a * (2LL * Na - a - 1) / 2 + a + 1;
    } else {
      a = p / Nb;
      b = p - a * Nb;
    }
    const float* __restrict__ p1 = xyz1 + (size_t)a * N * 3;
    const float* __restrict__ p2 = xyz2 + (size_t)b * N * 3;

    // objects j = lane + 64 t in registers; prices 0; bounding box of both clouds -> eps_0
    float ox[T], oy[T], oz[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int j = lane + 64 * t;
      ox[t] = 0.0f; oy[t] = 0.0f; oz[t] = 0.0f;
      if (j < N) { ox[t] = p2[j * 3]; oy[t] = p2[j * 3 + 1]; oz[t] = p2[j * 3 + 2]; }
    }
    float lo[3], hi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { lo[d] = __builtin_inff(); hi[d] = -__builtin_inff(); }
    for (int j = N + tid; j < 64 * T; j += kEcThreads) price[j] = __builtin_inff();
    for (int i = tid; i < N; i += kEcThreads) {
      price[i] = 0.0f;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float u = p1[i * 3 + d], v = p2[i * 3 + d];
        lo[d] = __builtin_fminf(lo[d], __builtin_fminf(u, v));
        hi[d] = __builtin_fmaxf(hi[d], __builtin_fmaxf(u, v));
      }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) fold_minmax_wave(lo[d], hi[d]);
    if (lane == 0) {
#pragma unroll
      for (int d = 0; d < 3; ++d) { wext[wave][d] = lo[d]; wext[wave][3 + d] = hi[d]; }
    }
    __syncthreads();
    float ext[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      float l = wext[0][d], h = wext[0][3 + d];
      for (int w = 1; w < kEcWaves; ++w) { l = __builtin_fminf(l, wext[w][d]); h = __builtin_fmaxf(h, wext[w][3 + d]); }
      ext[d] = h - l;
    }
    const float eps0 = ex_eps0(ext, eps_final);
    const int phase_cap = ex_phase_cap(N);

    int rounds = 0;
    bool capped = false;
    float eps = eps0;
    for (;;) {                                         // phases
      const bool final_phase = !(eps > eps_final);
      if (final_phase) eps = eps_final;
      for (int i = tid; i < N; i += kEcThreads) { owner[i] = -1; bid[i] = 0ull; lists[i] = i; }
      if (tid == 0) { cnt[0] = N; cnt[1] = 0; }
      __syncthreads();
      int r = 0;
      for (;;) {                                       // rounds; every thread takes the same branches
        const int cur = r & 1;
        const int U = cnt[cur];
        if (U == 0) break;                             // every bidder holds an object: the phase is done
        if (rounds >= max_rounds) { capped = true; break; }
        if (!final_phase && r >= phase_cap) break;     // the next phase starts from these prices
        int* __restrict__ L = lists + cur * N;
        int* __restrict__ Ln = lists + (cur ^ 1) * N;
        if (tid == 0) cnt[cur ^ 1] = 0;                // read last at the top of the previous round
        // bids: one wave per listed bidder, K12's scan over the register-resident objects
        for (int k = wave; k < U; k += kEcWaves) {
          const int i = __builtin_amdgcn_readfirstlane(L[k]);
          const float xx = p1[i * 3], xy = p1[i * 3 + 1], xz = p1[i * 3 + 2];
          float b1 = __builtin_inff(), b2 = __builtin_inff();
          int r1 = 0x7fffffff;
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const int j = lane + 64 * t;               // j >= N: value +inf, never taken while a value is finite
            ex_scan(ex_cost(xx, xy, xz, ox[t], oy[t], oz[t]) + price[j], ex_rank(j, i, N), b1, r1, b2);
          }
          fold_best2<1>(b1, r1, b2); fold_best2<2>(b1, r1, b2); fold_best2<4>(b1, r1, b2);
          fold_best2<8>(b1, r1, b2); fold_best2<16>(b1, r1, b2); fold_best2<32>(b1, r1, b2);
          if (lane == 0) {
            if ((unsigned)r1 >= (unsigned)N) r1 = 0;   // no finite value (NaN input): keeps j1 in [0, N)
            const int j1 = ex_unrank(r1, i, N);
            if (N == 1) b2 = b1;                       // no second object
            const float pj = price[j1];
            const unsigned bits = ex_bid_bits(pj, b1, b2, eps);
            atomicMax(&bid[j1], ex_bid_key(bits, i));
            L[k] = i | (j1 << 16);                     // N <= 2048: both fit
          }
        }
        __syncthreads();
        // the bidder a key names takes its object and displaces the owner; the others stay unassigned
        for (int k = tid; k < U; k += kEcThreads) {
          const int e = L[k];
          const int i = e & 0xffff, j = e >> 16;
          const unsigned long long key = bid[j];
          if (ex_key_bidder(key) == i) {
            const int o = owner[j];
            if (o >= 0) Ln[atomicAdd(&cnt[cur ^ 1], 1)] = o;
            owner[j] = i;
            price[j] = ex_key_price(key);
          } else {
            Ln[atomicAdd(&cnt[cur ^ 1], 1)] = i;
          }
        }
        __syncthreads();
        ++r;
        ++rounds;
      }
      __syncthreads();                                 // every thread has read the count before the next phase resets it
      if (final_phase || capped) break;
      eps = eps * kExTheta;
    }

    // assignment from the owners (in the first list); a capped pair is completed as in K12
    int* asg = lists;
    for (int i = tid; i < N; i += kEcThreads) asg[i] = -1;
    __syncthreads();
    for (int j = tid; j < N; j += kEcThreads) {
      const int o = owner[j];
      if (o >= 0) asg[o] = j;
    }
    __syncthreads();
    if (capped) {
      if (tid == 0) ex_complete(owner, asg, N);
      __syncthreads();
    }

    // cost and certificate terms per bidder (one wave per bidder), into the bid array
    float* cterm = reinterpret_cast<float*>(bid);
    float* gterm = cterm + N;
    for (int i = wave; i < N; i += kEcWaves) {
      const float xx = p1[i * 3], xy = p1[i * 3 + 1], xz = p1[i * 3 + 2];
      float u = __builtin_inff();
#pragma unroll
      for (int t = 0; t < T; ++t) {
        u = __builtin_fminf(u, ex_cost(xx, xy, xz, ox[t], oy[t], oz[t]) + price[lane + 64 * t]);
      }
      u = wave_min(u);
      if (lane == 0) {
        int j = asg[i];
        if ((unsigned)j >= (unsigned)N) j = 0;         // never: the assignment is a permutation
        const float cij = ex_cost(xx, xy, xz, p2[j * 3], p2[j * 3 + 1], p2[j * 3 + 2]);
        cterm[i] = cij;
        gterm[i] = (cij + price[j]) - u;
      }
    }
    __syncthreads();
    // K12's sums: its thread t adds the terms of bidders t, t + 1024, ...; its wave w sums by wave_sum; then waves
    // 0..15 in order.  Here K12's thread t = tid + 256 q is in wave tid / 64 + 4 q at the same lane.
#pragma unroll
    for (int q = 0; q < kEcSumWaves / kEcWaves; ++q) {
      float csum = 0.0f, gsum = 0.0f;
      for (int i = tid + q * kEcThreads; i < N; i += kEcSumWaves * 64) { csum += cterm[i]; gsum += gterm[i]; }
      csum = wave_sum(csum);
      gsum = wave_sum(gsum);
      if (lane == 0) { wred[wave + q * kEcWaves][0] = csum; wred[wave + q * kEcWaves][1] = gsum; }
    }
    __syncthreads();
    if (tid == 0) {
      float ct = 0.0f, gt = 0.0f;
      for (int w = 0; w < kEcSumWaves; ++w) { ct += wred[w][0]; gt += wred[w][1]; }
      const size_t e = (size_t)a * Nb + b;
      cost[e] = ct;
      gap[e] = gt;
      status[e] = capped ? 1 : 0;
      if (rounds_out) rounds_out[e] = rounds;
      if (sym) {
        const size_t m = (size_t)b * Nb + a;
        cost[m] = ct;
        gap[m] = gt;
        status[m] = capped ? 1 : 0;
        if (rounds_out) rounds_out[m] = rounds;
      }
    }
  }
}

template <int T>
int launch_emd_cross(const float* xyz1, const float* xyz2, int Na, int Nb, int N, float eps_final, int max_rounds,
                     int sym, float* cost, float* gap, int* status, int* rounds, unsigned long long* counter,
                     hipStream_t s) {
  const long long pairs = sym ? (long long)Na * (Na - 1) / 2 : (long long)Na * Nb;
  const size_t lds = (size_t)N * 20 + (size_t)64 * T * 4;
  int dev = 0, cus = 0, per_cu = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e == hipSuccess)
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(emd_cross_kernel<T>),
                                                     kEcThreads, lds);
  if (e != hipSuccess) { set_error("fpsg_emd_cross: %s", hipGetErrorString(e)); return (int)e; }
  // persistent workgroups: at most as many as run at once (the grid stays far below 2^31); pairs are 64-bit
  const long long resident = (long long)(cus > 0 ? cus : 1) * (per_cu > 0 ? per_cu : 1);
  const long long grid = pairs < 1 ? 1 : pairs < resident ? pairs : resident;
  e = hipMemsetAsync(counter, 0, sizeof(unsigned long long), s);
  if (e != hipSuccess) { set_error("fpsg_emd_cross: %s", hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL(emd_cross_kernel<T>, dim3((unsigned)grid), dim3(kEcThreads), lds, s, xyz1, xyz2, Na, Nb, N,
                     eps_final, max_rounds, sym, pairs, cost, gap, status, rounds, counter);
  return launch_status("fpsg_emd_cross");
}

}  // namespace
}  // namespace fpsg

extern "C" size_t fpsg_emd_cross_workspace_bytes(int Na, int Nb, int N) {
  if (Na <= 0 || Nb <= 0 || N <= 0 || N > FPSG_EMD_EXACT_MAX_N) return 0;
  return 256;                                          // the pair counter (one 64-bit word, padded)
}

extern "C" int fpsg_emd_cross(const float* xyz1, const float* xyz2, int Na, int Nb, int N, float eps_final,
                              int max_rounds, float* cost, float* gap, int* status, int* rounds, void* ws,
                              size_t ws_bytes, fpsg_stream_t stream) {
  using namespace fpsg;
  FPSG_REQUIRE_PTR(xyz1); FPSG_REQUIRE_PTR(cost); FPSG_REQUIRE_PTR(gap); FPSG_REQUIRE_PTR(status);
  FPSG_REQUIRE_PTR(ws);
  const int sym = xyz2 == nullptr;
  if (!sym) FPSG_REQUIRE(!misaligned4(xyz2), FPSG_E_ALIGN, "fpsg_emd_cross: 'xyz2' not 4-byte aligned");
  FPSG_REQUIRE(!misaligned4(rounds), FPSG_E_ALIGN, "fpsg_emd_cross: 'rounds' not 4-byte aligned");
  FPSG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, FPSG_E_ALIGN,
               "fpsg_emd_cross: 'ws' not 8-byte aligned");
  FPSG_REQUIRE(Na > 0 && Nb > 0 && N > 0, FPSG_E_SHAPE, "fpsg_emd_cross: Na,Nb,N must be positive (got %d,%d,%d)", Na,
               Nb, N);
  FPSG_REQUIRE(!sym || Nb == Na, FPSG_E_SHAPE, "fpsg_emd_cross: symmetric mode (xyz2 = NULL) needs Nb = Na (got %d,%d)",
               Nb, Na);
  FPSG_REQUIRE(N <= FPSG_EMD_EXACT_MAX_N, FPSG_E_LIMIT,
               "fpsg_emd_cross: N=%d exceeds the supported maximum of %d points", N, FPSG_EMD_EXACT_MAX_N);
  FPSG_REQUIRE(eps_final > 0.0f && eps_final < __builtin_inff(), FPSG_E_SHAPE,
               "fpsg_emd_cross: eps_final must be positive and finite (got %g)", (double)eps_final);
  FPSG_REQUIRE(max_rounds >= 1, FPSG_E_SHAPE, "fpsg_emd_cross: max_rounds must be at least 1 (got %d)", max_rounds);
  FPSG_REQUIRE(ws_bytes >= fpsg_emd_cross_workspace_bytes(Na, Nb, N), FPSG_E_SHAPE,
               "fpsg_emd_cross: workspace of %zu bytes, %zu needed", ws_bytes,
               fpsg_emd_cross_workspace_bytes(Na, Nb, N));
  if (sym) xyz2 = xyz1;
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long* counter = static_cast<unsigned long long*>(ws);
  if (N <= 256) return launch_emd_cross<4>(xyz1, xyz2, Na, Nb, N, eps_final, max_rounds, sym, cost, gap, status,
                                           rounds, counter, s);
  if (N <= 512) return launch_emd_cross<8>(xyz1, xyz2, Na, Nb, N, eps_final, max_rounds, sym, cost, gap, status,
                                           rounds, counter, s);
  if (N <= 1024) return launch_emd_cross<16>(xyz1, xyz2, Na, Nb, N, eps_final, max_rounds, sym, cost, gap, status,
                                             rounds, counter, s);
  return launch_emd_cross<32>(xyz1, xyz2, Na, Nb, N, eps_final, max_rounds, sym, cost, gap, status, rounds, counter,
                              s);
}
