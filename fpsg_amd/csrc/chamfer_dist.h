// chamfer_dist.h -- the squared point distance of K1 (chamfer_tiled.hip) and K13 (chamfer_cross.hip), scalar and
// packed.  Both kernels include this one definition, so every per-point minimum of K13 is bit-identical to K1's.
#pragma once
#include "fpsg_common.h"

namespace fpsg {

__device__ __forceinline__ float sq_dist(float qx, float qy, float qz, float cx, float cy, float cz) {
  float dx = cx - qx, dy = cy - qy, dz = cz - qz;
  return fma_rn(dz, dz, fma_rn(dy, dy, dx * dx));
}

// Squared distances of TWO rows (their coordinates share register pairs: q?.x = row a, q?.y = row b) to
// FOUR candidates (X, Y, Z = x, y, z of candidates 0..3): d = fma(dz,dz, fma(dy,dy, dx*dx)), dx = c - q,
// two candidates per packed instruction -- bit-identical to the scalar form.  Written out as one block:
//   * the row coordinate is splatted by op_sel from the shared pair (the compiler materialises {q,q} pairs:
//     48 VGPRs at R = 8) -- low half for row a, high half for row b;
//   * the four dependent chains (row a / b x candidates 01 / 23) are interleaved, so no packed operation
//     follows its producer (hipcc schedules the chains depth-first under register pressure and pads every
//     dependent pair with s_nop).  Outputs are early-clobber: they are written before the last input is read.
__device__ __forceinline__ void dist_2rows_4cands(v4f X, v4f Y, v4f Z, v2f qx, v2f qy, v2f qz,
                                                  v2f& a01, v2f& a23, v2f& b01, v2f& b23) {
  v2f t0, t1, t2, t3;
  const v2f x01 = X.xy, x23 = X.zw, y01 = Y.xy, y23 = Y.zw, z01 = Z.xy, z23 = Z.zw;
  asm volatile(
      "v_pk_add_f32 %0, %8, %14 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"     // a01 = x01 - qx.a
      "v_pk_add_f32 %1, %9, %14 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"     // a23 = x23 - qx.a
      "v_pk_add_f32 %2, %8, %14 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]\n\t"     // b01 = x01 - qx.b
      "v_pk_add_f32 %3, %9, %14 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]\n\t"     // b23 = x23 - qx.b
      "v_pk_add_f32 %4, %10, %15 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"    // t0 = y01 - qy.a
      "v_pk_add_f32 %5, %11, %15 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"    // t1 = y23 - qy.a
      "v_pk_add_f32 %6, %10, %15 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]\n\t"    // t2 = y01 - qy.b
      "v_pk_add_f32 %7, %11, %15 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]\n\t"    // t3 = y23 - qy.b
      "v_pk_mul_f32 %0, %0, %0\n\t"                                                              // dx*dx
      "v_pk_mul_f32 %1, %1, %1\n\t"
      "v_pk_mul_f32 %2, %2, %2\n\t"
      "v_pk_mul_f32 %3, %3, %3\n\t"
      "v_pk_fma_f32 %0, %4, %4, %0\n\t"                                                          // fma(dy,dy,.)
      "v_pk_fma_f32 %1, %5, %5, %1\n\t"
      "v_pk_fma_f32 %2, %6, %6, %2\n\t"
      "v_pk_fma_f32 %3, %7, %7, %3\n\t"
      "v_pk_add_f32 %4, %12, %16 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"    // t0 = z01 - qz.a
      "v_pk_add_f32 %5, %13, %16 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"
      "v_pk_add_f32 %6, %12, %16 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]\n\t"
      "v_pk_add_f32 %7, %13, %16 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]\n\t"
      "v_pk_fma_f32 %0, %4, %4, %0\n\t"                                                          // fma(dz,dz,.)
      "v_pk_fma_f32 %1, %5, %5, %1\n\t"
      "v_pk_fma_f32 %2, %6, %6, %2\n\t"
      "v_pk_fma_f32 %3, %7, %7, %3"
      : "=&v"(a01), "=&v"(a23), "=&v"(b01), "=&v"(b23), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
      : "v"(x01), "v"(x23), "v"(y01), "v"(y23), "v"(z01), "v"(z23), "v"(qx), "v"(qy), "v"(qz));
}

}  // namespace fpsg
