// The point-in-rotated-box test of the LiDAR input side: OpenPCDet's check_pt_in_box3d in float32,
//   sx = x - cx, sy = y - cy;  |z - cz| <= dz / 2;
//   lx = sx * cos(yaw) + sy * sin(yaw),  ly = -sx * sin(yaw) + sy * cos(yaw);  |lx| < dx / 2 + 1e-5, |ly| < dy / 2 + 1e-5.
// Shared by the paste's point removal (lidar_prep.hip) and the database build (gt_database.hip), so both decide alike.
#pragma once
#include "ud_common.h"

namespace {

// A box as the inside test reads it: centre, half extents (+1e-5 on x / y), sin / cos of the yaw.
struct RmBox {
  float cx, cy, cz, hx, hy, hz, sn, cs;
};

__device__ __forceinline__ bool in_rm_box(const RmBox& r, const float xyz[3]) {
  const float sx = xyz[0] - r.cx, sy = xyz[1] - r.cy;
  if (!(fabsf(xyz[2] - r.cz) <= r.hz)) return false;
  const float lx = sx * r.cs + sy * r.sn, ly = -sx * r.sn + sy * r.cs;
  return fabsf(lx) < r.hx && fabsf(ly) < r.hy;
}

}  // namespace
