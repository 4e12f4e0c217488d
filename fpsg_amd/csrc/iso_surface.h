// iso_surface.h -- K34: a signed implicit field of an oriented point cloud on a regular grid (K34a) and the marching-
// tetrahedra extraction of its zero level set as an indexed mesh (K34b), for gfx950.  The definition is in
// include/fpsg_hip.h (K34) and DESIGN.md; tests/_iso_ref.py restates it in numpy.  The entries are in mesh_normals.hip.
//
// K34a.  One workgroup of 256 threads owns a brick of 8 x 8 x 8 nodes, two nodes per thread: the nodes (i, j, k) and
// (i, j, k + 4), which share dx, dy and with them the first halves of d2 and of s (the header's operation order puts x
// and y first, so the shared prefixes are the very operations of the definition).  The cloud streams through LDS in
// tiles of 256 points, one point per thread.  A point is kept when its ball can reach the brick; the kept points are
// compacted by ballot in ascending point order (wave by wave, lane by lane) into records of eight floats that the inner
// loop reads by broadcast, so every node sums its points in ascending order whatever the cull drops.
//
// The cull is conservative in floating point.  Along one axis let lo and hi be the brick's first and last node
// coordinates, computed with the node formula itself (min and max of the two, whatever the sign of cell).  Rounding is
// monotone, so every node coordinate x of the brick has lo <= x <= hi, and with the kernel's own subtraction
// fl(x - p) >= fl(lo - p) =: a and fl(x - p) <= fl(hi - p) =: -c.  A point is dropped only when a > Rm or c > Rm on
// some axis, Rm = fl(|radius| * (1 + 2^-20)).  Then |dx| >= Rm for every node of the brick, d2 >= fl(dx dx) (adding
// non-negative terms and rounding never goes below a representable addend), and with u = 2^-24, each of fl(dx dx),
// fl(r r), fl(1 / .), fl(d2 inv) and Rm itself off by at most a factor 1 +- u:
//     fl(d2 inv) >= (1 + 2^-20)^2 (1 - u)^5 / (1 + u) > (1 + 2^-19) (1 - 7 u) > 1       (2^-19 = 32 u),
// so t = max(1 - fl(d2 inv), 0) is exactly +0, w = +0, and w s = +-0 leaves num (never -0: it starts at +0) and den
// unchanged bit for bit.  A NaN or infinite radius, origin or cell makes every comparison false: nothing is dropped.
// The argument needs r r and its reciprocal in the normal range, as the header states.
//
// K34b.  One thread per node, two launches (count, emit); the case table of the six Kuhn tetrahedra is generated at
// compile time from the header's rule (make_iso_table below), never typed in.
#pragma once
#include "fpsg_common.h"

namespace fpsg {
namespace iso {

constexpr int kBrick = FPSG_FIELD_BRICK;   // nodes per brick side: 8, two nodes per thread
constexpr int kTile = FPSG_FIELD_TILE;     // points per LDS tile: 256, one per thread
static_assert(kBrick == 8 && kTile == 256, "the thread layout below is written for these");

__device__ __forceinline__ bool finite3(float a, float b, float c) {
  return (__builtin_fabsf(a) < __builtin_inff()) && (__builtin_fabsf(b) < __builtin_inff()) &&
         (__builtin_fabsf(c) < __builtin_inff());
}

// the node formula: a multiply, then an add (the build forbids contraction)
__device__ __forceinline__ float node_coord(float origin, float cell, int i) { return origin + (float)i * cell; }

__global__ __launch_bounds__(256) void implicit_field_kernel(const float* __restrict__ points,
                                                             const float* __restrict__ normals, int N,
                                                             const float* __restrict__ origin,
                                                             const float* __restrict__ cell,
                                                             const float* __restrict__ radius, int G, int bricks_side,
                                                             float* __restrict__ field, float* __restrict__ weight) {
  __shared__ v4f rec[kTile * 2];               // (px, py, pz, nx) (ny, nz, -, -) per kept point
  __shared__ int wave_count[4];

  const int bricks = bricks_side * bricks_side * bricks_side;
  const int b = (int)(blockIdx.x / (unsigned)bricks);
  int br = (int)(blockIdx.x - (unsigned)b * (unsigned)bricks);
  const int bk = br % bricks_side; br /= bricks_side;
  const int bj = br % bricks_side;
  const int bi = br / bricks_side;
  const int i0 = bi * kBrick, j0 = bj * kBrick, k0 = bk * kBrick;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float ox = origin[b * 3], oy = origin[b * 3 + 1], oz = origin[b * 3 + 2];
  const float h = cell[b], r = radius[b];
  const float inv = 1.0f / (r * r);
  const float rm = __builtin_fabsf(r) * 1.00000095367431640625f;         // 1 + 2^-20

  // the brick's box, from the node formula at its first and last node of the grid
  const int i1 = min(i0 + kBrick - 1, G - 1), j1 = min(j0 + kBrick - 1, G - 1), k1 = min(k0 + kBrick - 1, G - 1);
  const float ax = node_coord(ox, h, i0), bx = node_coord(ox, h, i1);
  const float ay = node_coord(oy, h, j0), by = node_coord(oy, h, j1);
  const float az = node_coord(oz, h, k0), bz = node_coord(oz, h, k1);
  const float lox = __builtin_fminf(ax, bx), hix = __builtin_fmaxf(ax, bx);
  const float loy = __builtin_fminf(ay, by), hiy = __builtin_fmaxf(ay, by);
  const float loz = __builtin_fminf(az, bz), hiz = __builtin_fmaxf(az, bz);
  const bool box_ok = (ax == ax) && (bx == bx) && (ay == ay) && (by == by) && (az == az) && (bz == bz);

  // this thread's two nodes: (i, j, k) and (i, j, k + 4)
  const int ni = i0 + (tid >> 5), nj = j0 + ((tid >> 2) & 7), nk = k0 + (tid & 3);
  const float x = node_coord(ox, h, ni), y = node_coord(oy, h, nj);
  const float z0 = node_coord(oz, h, nk), z1 = node_coord(oz, h, nk + 4);
  float num0 = 0.0f, den0 = 0.0f, num1 = 0.0f, den1 = 0.0f;

  const float* P = points + (size_t)b * N * 3;
  const float* Q = normals + (size_t)b * N * 3;
  for (int base = 0; base < N; base += kTile) {
    const int j = base + tid;
    bool keep = false;
    float px = 0.0f, py = 0.0f, pz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (j < N) {
      px = P[(size_t)j * 3]; py = P[(size_t)j * 3 + 1]; pz = P[(size_t)j * 3 + 2];
      nx = Q[(size_t)j * 3]; ny = Q[(size_t)j * 3 + 1]; nz = Q[(size_t)j * 3 + 2];
      keep = finite3(px, py, pz) && finite3(nx, ny, nz);
      if (box_ok) {   // the comparisons are false on NaN: only a proven +0 is dropped
        const bool out = (lox - px > rm) || (px - hix > rm) || (loy - py > rm) || (py - hiy > rm) ||
                         (loz - pz > rm) || (pz - hiz > rm);
        keep = keep && !out;
      }
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    int first = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = wave_count[w];
      if (w < wave) first += c;
      total += c;
    }
    if (keep) {
      const int slot = first + __popcll(mask & ((1ull << lane) - 1ull));
      rec[slot * 2] = v4f{px, py, pz, nx};
      rec[slot * 2 + 1] = v4f{ny, nz, 0.0f, 0.0f};
    }
    __syncthreads();
    for (int s = 0; s < total; ++s) {
      const v4f a = rec[s * 2], c = rec[s * 2 + 1];
      const float dx = x - a.x, dy = y - a.y;
      const float dxy = dx * dx + dy * dy;
      const float sxy = dx * a.w + dy * c.x;
      {
        const float dz = z0 - a.z;
        const float d2 = dxy + dz * dz;
        const float t = __builtin_fmaxf(1.0f - d2 * inv, 0.0f);
        const float w = (t * t) * t;
        const float sd = sxy + dz * c.y;
        num0 = num0 + w * sd;
        den0 = den0 + w;
      }
      {
        const float dz = z1 - a.z;
        const float d2 = dxy + dz * dz;
        const float t = __builtin_fmaxf(1.0f - d2 * inv, 0.0f);
        const float w = (t * t) * t;
        const float sd = sxy + dz * c.y;
        num1 = num1 + w * sd;
        den1 = den1 + w;
      }
    }
    __syncthreads();                              // the records and counts are rewritten by the next tile
  }

  if (ni < G && nj < G) {
    const size_t row = (((size_t)b * G + ni) * G + nj) * G;
    if (nk < G) {
      field[row + nk] = den0 > 0.0f ? num0 / den0 : __builtin_nanf("");
      if (weight) weight[row + nk] = den0;
    }
    if (nk + 4 < G) {
      field[row + nk + 4] = den1 > 0.0f ? num1 / den1 : __builtin_nanf("");
      if (weight) weight[row + nk + 4] = den1;
    }
  }
}

// ---- K34b ---------------------------------------------------------------------------------------------------------------
// The six Kuhn tetrahedra of a cell: for the permutations (a, b, c) of the axes (0 = i, 1 = j, 2 = k) in lexicographic
// order the path 000, +e_a, +e_a+e_b, 111.  A corner is three bits, bit 2 = i, bit 1 = j, bit 0 = k (as the edge
// classes are written: 100 steps along i).  A mesh vertex is a grid edge: (owner corner, class).
struct IsoTable {
  unsigned char corner[6][4];        // path corner p of tetrahedron t, as three bits
  unsigned char count[6][16];        // triangles of case m (bit p set: path corner p inside)
  unsigned char owner[6][16][2][3];  // per triangle vertex: the edge's lower corner, three bits
  unsigned char cls[6][16][2][3];    // and its class 0..6 in the order 100 010 001 110 101 011 111
};

constexpr int iso_class_of(int step) {         // step: three bits, never 0
  constexpr int order[7] = {4, 2, 1, 6, 5, 3, 7};
  for (int c = 0; c < 7; ++c)
    if (order[c] == step) return c;
  return -1;
}

constexpr IsoTable make_iso_table() {
  IsoTable T{};
  constexpr int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (int t = 0; t < 6; ++t) {
    const int ea = 4 >> perms[t][0], eb = 4 >> perms[t][1];
    T.corner[t][0] = 0; T.corner[t][1] = (unsigned char)ea; T.corner[t][2] = (unsigned char)(ea | eb); T.corner[t][3] = 7;
    for (int m = 0; m < 16; ++m) {
      int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, n_in = 0, n_out = 0;
      for (int p = 0; p < 4; ++p) {
        if (m >> p & 1) in[n_in++] = p;
        else out[n_out++] = p;
      }
      int e[2][3][2] = {};             // triangles as edges (inside corner, outside corner)
      int n = 0;
      if (n_in == 1) {
        n = 1;
        for (int q = 0; q < 3; ++q) { e[0][q][0] = in[0]; e[0][q][1] = out[q]; }
      } else if (n_in == 3) {
        n = 1;
        for (int q = 0; q < 3; ++q) { e[0][q][0] = in[q]; e[0][q][1] = out[0]; }
      } else if (n_in == 2) {
        n = 2;
        const int i = in[0], j = in[1], k = out[0], l = out[1];
        e[0][0][0] = i; e[0][0][1] = k; e[0][1][0] = i; e[0][1][1] = l; e[0][2][0] = j; e[0][2][1] = l;
        e[1][0][0] = i; e[1][0][1] = k; e[1][1][0] = j; e[1][1][1] = l; e[1][2][0] = j; e[1][2][1] = k;
      }
      // orientation at the edge midpoints (doubled, so integers): the normal must look from the inside corners'
      // centroid to the outside corners'
      int dir[3] = {0, 0, 0};
      for (int ax = 0; ax < 3; ++ax) {
        int so = 0, si = 0;
        for (int q = 0; q < n_out; ++q) so += T.corner[t][out[q]] >> (2 - ax) & 1;
        for (int q = 0; q < n_in; ++q) si += T.corner[t][in[q]] >> (2 - ax) & 1;
        dir[ax] = n_in * so - n_out * si;
      }
      bool flip = false;
      if (n > 0) {
        int mid[3][3] = {};
        for (int q = 0; q < 3; ++q)
          for (int ax = 0; ax < 3; ++ax)
            mid[q][ax] = (T.corner[t][e[0][q][0]] >> (2 - ax) & 1) + (T.corner[t][e[0][q][1]] >> (2 - ax) & 1);
        const int ux = mid[1][0] - mid[0][0], uy = mid[1][1] - mid[0][1], uz = mid[1][2] - mid[0][2];
        const int vx = mid[2][0] - mid[0][0], vy = mid[2][1] - mid[0][1], vz = mid[2][2] - mid[0][2];
        const int d = (uy * vz - uz * vy) * dir[0] + (uz * vx - ux * vz) * dir[1] + (ux * vy - uy * vx) * dir[2];
        flip = d < 0;
      }
      T.count[t][m] = (unsigned char)n;
      for (int f = 0; f < n; ++f)
        for (int q = 0; q < 3; ++q) {
          const int src = (flip && q > 0) ? 3 - q : q;           // the last two exchanged
          const int p0 = e[f][src][0] < e[f][src][1] ? e[f][src][0] : e[f][src][1];
          const int p1 = e[f][src][0] < e[f][src][1] ? e[f][src][1] : e[f][src][0];
          const int c0 = T.corner[t][p0], c1 = T.corner[t][p1];  // c0 is a subset of c1: the path only adds axes
          T.owner[t][m][f][q] = (unsigned char)c0;
          T.cls[t][m][f][q] = (unsigned char)iso_class_of(c1 & ~c0);
        }
    }
  }
  return T;
}

__constant__ IsoTable kIsoTable = make_iso_table();

__device__ __forceinline__ bool iso_finite(float f) { return __builtin_fabsf(f) < __builtin_inff(); }
__device__ __forceinline__ bool iso_inside(float f) { return f < 0.0f; }       // 0, -0 and NaN are not inside

// the active owned edges of node (i, j, k) of the grid F [G,G,G]: bit c for class c
__device__ __forceinline__ unsigned iso_edge_flags(const float* __restrict__ F, int G, int i, int j, int k) {
  const float f0 = F[((size_t)i * G + j) * G + k];
  if (!iso_finite(f0)) return 0u;
  const bool in0 = iso_inside(f0);
  unsigned flags = 0u;
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    constexpr int order[7] = {4, 2, 1, 6, 5, 3, 7};
    const int ii = i + (order[c] >> 2 & 1), jj = j + (order[c] >> 1 & 1), kk = k + (order[c] & 1);
    if (ii < G && jj < G && kk < G) {
      const float f1 = F[((size_t)ii * G + jj) * G + kk];
      if (iso_finite(f1) && iso_inside(f1) != in0) flags |= 1u << c;
    }
  }
  return flags;
}

// the cell's eight corners (index: three bits i j k) -> false when the cell is outside the grid
__device__ __forceinline__ bool iso_cell_corners(const float* __restrict__ F, int G, int i, int j, int k, float f[8]) {
  if (i >= G - 1 || j >= G - 1 || k >= G - 1) return false;
#pragma unroll
  for (int c = 0; c < 8; ++c) f[c] = F[((size_t)(i + (c >> 2 & 1)) * G + (j + (c >> 1 & 1))) * G + (k + (c & 1))];
  return true;
}

// case of tetrahedron t, or -1 when one of its corners is not finite
__device__ __forceinline__ int iso_tet_case(const float f[8], int t) {
  int m = 0;
  bool ok = true;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float v = f[kIsoTable.corner[t][p]];
    ok = ok && iso_finite(v);
    m |= (int)iso_inside(v) << p;
  }
  return ok ? m : -1;
}

__global__ __launch_bounds__(256) void iso_classify_kernel(const float* __restrict__ field, int G, long long nodes,
                                                           long long total, int* __restrict__ node_edges,
                                                           int* __restrict__ cell_tris) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= total) return;
  const long long b = n / nodes;
  int local = (int)(n - b * nodes);
  const int k = local % G; local /= G;
  const int j = local % G;
  const int i = local / G;
  const float* F = field + (size_t)b * nodes;
  node_edges[n] = __popc(iso_edge_flags(F, G, i, j, k));
  float f[8];
  int tris = 0;
  if (iso_cell_corners(F, G, i, j, k, f)) {
    for (int t = 0; t < 6; ++t) {
      const int m = iso_tet_case(f, t);
      if (m >= 0) tris += kIsoTable.count[t][m];
    }
  }
  cell_tris[n] = tris;
}

__global__ __launch_bounds__(256) void iso_emit_kernel(const float* __restrict__ field,
                                                       const float* __restrict__ origin,
                                                       const float* __restrict__ cell, int B, int G, long long nodes,
                                                       long long total, const long long* __restrict__ edge_offset,
                                                       const long long* __restrict__ tri_offset, long long n_verts,
                                                       long long n_faces, float* __restrict__ verts,
                                                       int* __restrict__ faces, long long* __restrict__ vert_range,
                                                       long long* __restrict__ face_range) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= total) return;
  const long long b = n / nodes;
  int local = (int)(n - b * nodes);
  const int k = local % G; local /= G;
  const int j = local % G;
  const int i = local / G;
  const float* F = field + (size_t)b * nodes;
  const long long vert_first = edge_offset[b * nodes];           // the cloud's own first vertex
  if (i == 0 && j == 0 && k == 0) {
    if (vert_range) vert_range[b] = vert_first;
    if (face_range) face_range[b] = tri_offset[b * nodes];
    if (b == B - 1) {
      if (vert_range) vert_range[B] = n_verts;
      if (face_range) face_range[B] = n_faces;
    }
  }
  // vertices: this node's active edges in class order
  const unsigned flags = iso_edge_flags(F, G, i, j, k);
  if (flags) {
    const float h = cell[b];
    const float x0 = node_coord(origin[b * 3], h, i), y0 = node_coord(origin[b * 3 + 1], h, j);
    const float z0 = node_coord(origin[b * 3 + 2], h, k);
    const float f0 = F[((size_t)i * G + j) * G + k];
    long long at = edge_offset[n];
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      constexpr int order[7] = {4, 2, 1, 6, 5, 3, 7};
      if (!(flags >> c & 1u)) continue;
      const int di = order[c] >> 2 & 1, dj = order[c] >> 1 & 1, dk = order[c] & 1;
      const float f1 = F[((size_t)(i + di) * G + (j + dj)) * G + (k + dk)];
      const float t = f0 / (f0 - f1);
      if (at >= 0 && at < n_verts) {
        verts[at * 3] = di ? x0 + t * h : x0;
        verts[at * 3 + 1] = dj ? y0 + t * h : y0;
        verts[at * 3 + 2] = dk ? z0 + t * h : z0;
      }
      ++at;
    }
  }
  // triangles: the cell's tetrahedra in order, each in table order
  float f[8];
  if (!iso_cell_corners(F, G, i, j, k, f)) return;
  long long at = tri_offset[n];
  for (int t = 0; t < 6; ++t) {
    const int m = iso_tet_case(f, t);
    if (m < 0) continue;
    const int cnt = kIsoTable.count[t][m];
    for (int q = 0; q < cnt; ++q) {
      int id[3];
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const int o = kIsoTable.owner[t][m][q][v], c = kIsoTable.cls[t][m][q][v];
        const int oi = i + (o >> 2 & 1), oj = j + (o >> 1 & 1), ok = k + (o & 1);
        const unsigned fl = iso_edge_flags(F, G, oi, oj, ok);
        const long long own = b * nodes + ((long long)oi * G + oj) * G + ok;
        id[v] = (int)(edge_offset[own] + __popc(fl & ((1u << c) - 1u)) - vert_first);
      }
      if (at >= 0 && at < n_faces) {
        faces[at * 3] = id[0]; faces[at * 3 + 1] = id[1]; faces[at * 3 + 2] = id[2];
      }
      ++at;
    }
  }
}

}  // namespace iso
}  // namespace fpsg
