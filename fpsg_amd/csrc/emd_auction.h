// emd_auction.h -- the auction arithmetic of K12 (emd_exact.hip) and K14 (emd_cross.hip): cost, best / second-best
// fold, bid with its one-ulp floor, rotated tie-break, 64-bit bid key, eps schedule, caps and the completion of a
// capped pair.  Both kernels include this one definition, so a K14 pair computes every bid of K12 bit for bit and
// follows the same trajectory (same rounds, same status, same final prices and assignment).
#pragma once
#include "fpsg_common.h"

namespace fpsg {

constexpr float kExTheta = 0.25f;            // eps_{k+1} = eps_k / 4
constexpr int kExPhaseRoundsPerPoint = 16;   // round cap of an intermediate phase: 16 N + 256

__device__ __forceinline__ float ex_cost(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return __builtin_amdgcn_sqrtf(fma_rn(dz, dz, fma_rn(dy, dy, dx * dx)));
}

// (best value, its rank, second-best value) of two lanes: the lower (value, rank) wins; the second best is the smaller
// of the loser's best and the winner's second best.
template <int M>
__device__ __forceinline__ void fold_best2(float& b1, int& r1, float& b2) {
  const float o1 = lane_xor_f<M>(b1), o2 = lane_xor_f<M>(b2);
  const int orr = lane_xor_i<M>(r1);
  if (o1 < b1 || (o1 == b1 && orr < r1)) {
    b2 = __builtin_fminf(b1, o2);
    b1 = o1;
    r1 = orr;
  } else {
    b2 = __builtin_fminf(b2, o1);
  }
}

__device__ __forceinline__ void fold_minmax_wave(float& lo, float& hi) {
  lo = wave_min(lo);
  hi = wave_max(hi);
}

// rotated tie-break: equal values between objects go to the lowest (j - i) mod N
__device__ __forceinline__ int ex_rank(int j, int i, int N) {
  int rk = j - i;
  if (rk < 0) rk += N;
  return rk;
}

__device__ __forceinline__ int ex_unrank(int rk, int i, int N) {
  int j = rk + i;
  if (j >= N) j -= N;
  return j;
}

// one object's value v = c_ij + p_j (rank rk) into a lane's (best, rank, second best)
__device__ __forceinline__ void ex_scan(float v, int rk, float& b1, int& r1, float& b2) {
  if (v < b1 || (v == b1 && rk < r1)) { b2 = b1; b1 = v; r1 = rk; }
  else b2 = __builtin_fminf(b2, v);
}

// The bid on the best object (price pj): pj + (second - best) + eps, as price bits (b2 = b1 when N = 1: there is no
// second object); the increment is at least one ulp of the price, whatever eps is.
__device__ __forceinline__ unsigned ex_bid_bits(float pj, float b1, float b2, float eps) {
  const float nb = pj + ((b2 - b1) + eps);
  return nb > pj ? __float_as_uint(nb) : __float_as_uint(pj) + 1u;
}

// (price bits << 32 | ~bidder): non-negative floats order as their bits, so the highest bid wins an atomicMax and
// ties go to the lowest bidder id.
__device__ __forceinline__ unsigned long long ex_bid_key(unsigned bits, int i) {
  return ((unsigned long long)bits << 32) | (unsigned)(~i);
}

__device__ __forceinline__ int ex_key_bidder(unsigned long long key) { return (int)(~(unsigned)key); }

__device__ __forceinline__ float ex_key_price(unsigned long long key) { return __uint_as_float((unsigned)(key >> 32)); }

// eps_0: a quarter of the bounding-box diagonal of both clouds (extents ext), an upper bound of every c_ij
__device__ __forceinline__ float ex_eps0(const float ext[3], float eps_final) {
  const float diag = __builtin_amdgcn_sqrtf(fma_rn(ext[2], ext[2], fma_rn(ext[1], ext[1], ext[0] * ext[0])));
  return __builtin_fmaxf(diag * 0.25f, eps_final);
}

__device__ __forceinline__ int ex_phase_cap(int N) { return kExPhaseRoundsPerPoint * N + 256; }

// Completion of a capped pair (one thread): the unassigned bidders take the free objects in index order.
__device__ __forceinline__ void ex_complete(int* owner, int* asg, int N) {
  int i = 0;
  for (int j = 0; j < N; ++j) {
    if (owner[j] >= 0) continue;
    while (i < N && asg[i] >= 0) ++i;          // as many unassigned bidders as free objects
    if (i == N) break;
    asg[i] = j;
    owner[j] = i;
  }
}

}  // namespace fpsg
