// mesh_normals.hip -- mesh construction for gfx950: K31a, area-weighted vertex normals of B meshes that share their
// faces, and the entries of K34 (implicit field of an oriented cloud, marching-tetrahedra isosurface; the kernels are in
// iso_surface.h).  K31a's definition
// is in include/fpsg_hip.h (K31) and DESIGN.md: the un-normalised cross products of the faces around a vertex, summed in
// ascending face order and divided by the sum's length.
//
// Gather form: one thread per (mesh, vertex) walks the vertex's slice of the corner table (offsets, corner_faces) that
// the host built once for the topology.  No atomics, no order left to the launch: the bits are the same on every run.
// The table is device memory that the entry cannot read, so the kernel trusts none of it: a slice is clamped into
// [0, n], a face id outside [0, F) or a face with an index outside [0, V) is skipped.  A table that lies gives wrong
// normals and never an access outside the arrays.
#include "iso_surface.h"
#include "render_common.h"

namespace fpsg {
namespace {

__global__ __launch_bounds__(256) void mesh_vertex_normals_kernel(const float* __restrict__ verts, int V,
                                                                  const int* __restrict__ faces, int F,
                                                                  const int* __restrict__ offsets,
                                                                  const int* __restrict__ corner_faces, int n,
                                                                  float* __restrict__ normals) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const float* P = verts + (size_t)blockIdx.y * V * 3;
  int k0 = offsets[v], k1 = offsets[v + 1];              // offsets has V + 1 entries
  k0 = min(max(k0, 0), n);
  k1 = min(max(k1, k0), n);
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  for (int k = k0; k < k1; ++k) {
    const int f = corner_faces[k];
    if ((unsigned)f >= (unsigned)F) continue;
    const int ia = faces[(size_t)f * 3], ib = faces[(size_t)f * 3 + 1], ic = faces[(size_t)f * 3 + 2];
    if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) continue;
    const float* a = P + (size_t)ia * 3;
    const float* b = P + (size_t)ib * 3;
    const float* c = P + (size_t)ic * 3;
    const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    sx = sx + (e1y * e2z - e1z * e2y);
    sy = sy + (e1z * e2x - e1x * e2z);
    sz = sz + (e1x * e2y - e1y * e2x);
  }
  const float len = __builtin_sqrtf((sx * sx + sy * sy) + sz * sz);
  float* o = normals + ((size_t)blockIdx.y * V + v) * 3;
  if (len > 0.0f && finite_f(len)) { o[0] = sx / len; o[1] = sy / len; o[2] = sz / len; }
  else { o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f; }
}

}  // namespace
}  // namespace fpsg

extern "C" int fpsg_mesh_vertex_normals(const float* verts, int B, int V, const int32_t* faces, int F,
                                        const int32_t* offsets, const int32_t* corner_faces, int n, float* normals,
                                        fpsg_stream_t stream) {
  using namespace fpsg;
  FPSG_REQUIRE(B > 0 && V > 0 && F > 0 && n >= 0 && (long long)n <= 3ll * F, FPSG_E_SHAPE,
               "fpsg_mesh_vertex_normals: B,V,F must be positive and n from 0 to 3 F (got %d,%d,%d,%d)", B, V, F, n);
  FPSG_REQUIRE(B <= FPSG_NORMALS_MAX_MESHES && V <= FPSG_MESH_MAX_FACES && F <= FPSG_MESH_MAX_FACES, FPSG_E_LIMIT,
               "fpsg_mesh_vertex_normals: B <= %d and V,F <= %d are supported (got %d,%d,%d)", FPSG_NORMALS_MAX_MESHES,
               FPSG_MESH_MAX_FACES, B, V, F);
  FPSG_REQUIRE_PTR(verts); FPSG_REQUIRE_PTR(faces); FPSG_REQUIRE_PTR(offsets); FPSG_REQUIRE_PTR(normals);
  if (n > 0) FPSG_REQUIRE_PTR(corner_faces);
  FPSG_REQUIRE(!misaligned4(corner_faces), FPSG_E_ALIGN, "fpsg_mesh_vertex_normals: 'corner_faces' not 4-byte aligned");
  hipLaunchKernelGGL(mesh_vertex_normals_kernel, dim3((unsigned)((V + 255) / 256), (unsigned)B), dim3(256), 0,
                     static_cast<hipStream_t>(stream), verts, V, faces, F, offsets, corner_faces, n, normals);
  return launch_status("fpsg_mesh_vertex_normals");
}

// ---- K34 ----------------------------------------------------------------------------------------------------------------
namespace fpsg {
namespace {

// K34's shape and limit checks, in the header's order; 0 when B clouds on G nodes per side pass
int iso_grid_status(const char* who, int B, int G) {
  FPSG_REQUIRE(B > 0 && G >= FPSG_ISO_MIN_GRID, FPSG_E_SHAPE, "%s: B must be positive and G at least %d (got %d,%d)", who,
               FPSG_ISO_MIN_GRID, B, G);
  FPSG_REQUIRE(G <= FPSG_ISO_MAX_GRID, FPSG_E_LIMIT, "%s: G <= %d is supported (got %d)", who, FPSG_ISO_MAX_GRID, G);
  FPSG_REQUIRE((long long)B * G * G * G <= (long long)FPSG_ISO_MAX_NODES, FPSG_E_LIMIT,
               "%s: B G^3 <= %d nodes are supported (got %d x %d^3)", who, FPSG_ISO_MAX_NODES, B, G);
  return 0;
}

}  // namespace
}  // namespace fpsg

extern "C" int fpsg_implicit_field(const float* points, const float* normals, int B, int N, const float* origin,
                                   const float* cell, const float* radius, int G, float* field, float* weight,
                                   fpsg_stream_t stream) {
  using namespace fpsg;
  FPSG_REQUIRE(N > 0, FPSG_E_SHAPE, "fpsg_implicit_field: N must be positive (got %d)", N);
  if (const int rc = iso_grid_status("fpsg_implicit_field", B, G)) return rc;
  FPSG_REQUIRE(N <= FPSG_NORMALS_POINTS_MAX_N, FPSG_E_LIMIT, "fpsg_implicit_field: N <= %d is supported (got %d)",
               FPSG_NORMALS_POINTS_MAX_N, N);
  FPSG_REQUIRE_PTR(points); FPSG_REQUIRE_PTR(normals); FPSG_REQUIRE_PTR(origin); FPSG_REQUIRE_PTR(cell);
  FPSG_REQUIRE_PTR(radius); FPSG_REQUIRE_PTR(field);
  FPSG_REQUIRE(!misaligned4(weight), FPSG_E_ALIGN, "fpsg_implicit_field: 'weight' not 4-byte aligned");
  const int side = (G + iso::kBrick - 1) / iso::kBrick;
  hipLaunchKernelGGL(iso::implicit_field_kernel, dim3((unsigned)B * (unsigned)(side * side * side)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), points, normals, N, origin, cell, radius, G, side, field, weight);
  return launch_status("fpsg_implicit_field");
}

extern "C" int fpsg_iso_classify(const float* field, int B, int G, int32_t* node_edges, int32_t* cell_tris,
                                 fpsg_stream_t stream) {
  using namespace fpsg;
  if (const int rc = iso_grid_status("fpsg_iso_classify", B, G)) return rc;
  FPSG_REQUIRE_PTR(field); FPSG_REQUIRE_PTR(node_edges); FPSG_REQUIRE_PTR(cell_tris);
  const long long nodes = (long long)G * G * G, total = nodes * B;
  hipLaunchKernelGGL(iso::iso_classify_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), field, G, nodes, total, node_edges, cell_tris);
  return launch_status("fpsg_iso_classify");
}

extern "C" int fpsg_iso_emit(const float* field, const float* origin, const float* cell, int B, int G,
                             const int64_t* edge_offset, const int64_t* tri_offset, long long n_verts, long long n_faces,
                             float* verts, int32_t* faces, int64_t* vert_range, int64_t* face_range,
                             fpsg_stream_t stream) {
  using namespace fpsg;
  FPSG_REQUIRE(n_verts >= 0 && n_faces >= 0, FPSG_E_SHAPE, "fpsg_iso_emit: n_verts and n_faces must not be negative "
               "(got %lld,%lld)", n_verts, n_faces);
  if (const int rc = iso_grid_status("fpsg_iso_emit", B, G)) return rc;
  const long long nodes = (long long)G * G * G, total = nodes * B;
  FPSG_REQUIRE_PTR(field); FPSG_REQUIRE_PTR(origin); FPSG_REQUIRE_PTR(cell); FPSG_REQUIRE_PTR(edge_offset);
  FPSG_REQUIRE_PTR(tri_offset);
  if (n_verts > 0) FPSG_REQUIRE_PTR(verts);
  if (n_faces > 0) FPSG_REQUIRE_PTR(faces);
  FPSG_REQUIRE(!misaligned4(verts) && !misaligned4(faces), FPSG_E_ALIGN, "fpsg_iso_emit: 'verts' or 'faces' not 4-byte aligned");
  FPSG_REQUIRE(((reinterpret_cast<uintptr_t>(edge_offset) | reinterpret_cast<uintptr_t>(tri_offset) |
                 reinterpret_cast<uintptr_t>(vert_range) | reinterpret_cast<uintptr_t>(face_range)) & 7u) == 0,
               FPSG_E_ALIGN, "fpsg_iso_emit: the 64-bit arrays must be 8-byte aligned");
  hipLaunchKernelGGL(iso::iso_emit_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), field, origin, cell, B, G, nodes, total,
                     reinterpret_cast<const long long*>(edge_offset), reinterpret_cast<const long long*>(tri_offset),
                     n_verts, n_faces, verts, faces, reinterpret_cast<long long*>(vert_range),
                     reinterpret_cast<long long*>(face_range));
  return launch_status("fpsg_iso_emit");
}
