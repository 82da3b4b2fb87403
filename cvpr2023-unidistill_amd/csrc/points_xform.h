// Point transform arithmetic shared by ud_points_transform and the fused LiDAR input chain (ud_lidar_prep_*), so the
// two paths cannot drift.  numpy's (m @ [x y z 1]^T)[:3] on float64, stored into a float32 cloud: per output
// coordinate ((m0 x + m1 y) + m2 z) + m3 in float64 (no contraction: the library builds with -ffp-contract=off),
// rounded once to float32.  m: row-major 4x4 float64.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void ud_points_xform(const double* m, float x, float y, float z, float r[3]) {
  const double dx = x, dy = y, dz = z;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    r[k] = (float)(((m[4 * k] * dx + m[4 * k + 1] * dy) + m[4 * k + 2] * dz) + m[4 * k + 3]);
}
