// self_knn.h -- the self-neighbour sweep that K21 (repulsion.hip) and K33a (point_normals.hip) share: the k nearest
// neighbours of every point in its OWN cloud, as sorted register lists in the lexicographic (d2, j) order.  Both
// kernels include this one definition, so their lists are the same lists (tests/test_point_normals_gpu.py pins it).
#pragma once
#include <cmath>

#include "chamfer_dist.h"

namespace fpsg {

constexpr int kSelfKnnTile = 1024;                                // candidates per LDS tile

// Puts (c, j) into the sorted list; the caller has checked c < d[K - 1].  Branch-free: slot s becomes the median of
// (d[s - 1], d[s], c) -- d[s - 1] where c lands above it, c where it lands here, d[s] otherwise -- one v_med3_f32, and
// its index follows the same two comparisons (strict: on equal distances the resident, which has the lower index, stays).
template <int K>
__device__ __forceinline__ void topk_insert(float (&d)[K], int (&ix)[K], float c, int j) {
  bool lt[K];
#pragma unroll
  for (int s = 0; s < K; ++s) lt[s] = c < d[s];
#pragma unroll
  for (int s = K - 1; s >= 1; --s) {
    ix[s] = lt[s - 1] ? ix[s - 1] : (lt[s] ? j : ix[s]);
    d[s] = __builtin_amdgcn_fmed3f(d[s - 1], d[s], c);
  }
  ix[0] = lt[0] ? j : ix[0];
  d[0] = lt[0] ? c : d[0];
}

// Loads candidates j0 .. j0 + kSelfKnnTile of cloud `x` into the tile, THREADS threads together.  Past the end of the
// cloud the padding is NaN: every comparison with a NaN distance is false, so a padded candidate enters no list.
template <int THREADS>
__device__ __forceinline__ void stage_xyz_tile(const float* __restrict__ x, int N, int j0, float* sx, float* sy,
                                               float* sz) {
  static_assert(kSelfKnnTile % THREADS == 0, "every thread stages the same number of candidates");
#pragma unroll
  for (int u = 0; u < kSelfKnnTile / THREADS; ++u) {
    const int t = (int)threadIdx.x + u * THREADS;
    const int j = j0 + t;
    const bool ok = j < N;
    sx[t] = ok ? x[3 * (size_t)j + 0] : NAN;
    sy[t] = ok ? x[3 * (size_t)j + 1] : NAN;
    sz[t] = ok ? x[3 * (size_t)j + 2] : NAN;
  }
}

// The K nearest neighbours of query i = (qx, qy, qz) among the N points of its own cloud `x`, i itself excluded by
// index: d (ascending) and ix come back sorted, slots nobody entered hold +inf / -1.  sx, sy, sz are the workgroup's
// tile, kSelfKnnTile floats each, 16-byte aligned: every lane of a wave reads the same four candidates with one
// broadcast ds_read_b128 per coordinate.
// EVERY thread of the workgroup of THREADS calls this, dead lanes past N included (with any finite query): the trip
// count is uniform and the loop contains barriers.
// The sweep is ascending in j and a candidate enters only where d2 < d[K - 1] strictly, so an equal distance at a
// higher index loses the tie: the resulting order is lexicographic in (d2, j).
template <int K, int THREADS>
__device__ __forceinline__ void self_knn_sweep(const float* x, int N, int i, float qx, float qy, float qz,
                                               float (&d)[K], int (&ix)[K], float* sx, float* sy, float* sz) {
#pragma unroll
  for (int s = 0; s < K; ++s) {
    d[s] = INFINITY;
    ix[s] = -1;
  }
  for (int j0 = 0; j0 < N; j0 += kSelfKnnTile) {
    __syncthreads();                                              // the previous tile has been read
    stage_xyz_tile<THREADS>(x, N, j0, sx, sy, sz);
    __syncthreads();
    const int groups = (min(kSelfKnnTile, N - j0) + 3) >> 2;
    for (int g = 0; g < groups; ++g) {
      const v4f X = *reinterpret_cast<const v4f*>(sx + 4 * g);
      const v4f Y = *reinterpret_cast<const v4f*>(sy + 4 * g);
      const v4f Z = *reinterpret_cast<const v4f*>(sz + 4 * g);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + 4 * g + c;
        const float d2 = sq_dist(qx, qy, qz, X[c], Y[c], Z[c]);
        if ((d2 < d[K - 1]) & (j != i)) topk_insert<K>(d, ix, d2, j);
      }
    }
  }
}

}  // namespace fpsg
