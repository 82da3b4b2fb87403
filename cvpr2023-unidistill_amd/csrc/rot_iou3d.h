// Rotated 3-D IoU of two boxes (x, y, z, dx, dy, dz, yaw) and its derivative with respect to the first box
// (det_loss.hip: the opt-in "rotated3d" IoU loss / IoU-aware target, and the pairwise op ud_rot_iou3d_pairs).
//
//   inter_bev = area of the intersection of the two rotated rectangles (Sutherland-Hodgman + shoelace, as bev_iou.h)
//   oz        = max(min(z_a + dz_a/2, z_b + dz_b/2) - max(z_a - dz_a/2, z_b - dz_b/2), 0)
//   IoU       = inter_bev oz / max(dx_a dy_a dz_a + dx_b dy_b dz_b - inter_bev oz, 1e-8)
//
// Box a is moved into the frame of box b first, so that the clip runs against the four axis-aligned half-planes
// |X| <= dx_b/2, |Y| <= dy_b/2: the inside tests are single subtractions, a clipped coordinate IS the bound, and the
// shoelace sums products of offsets from b's centre instead of map coordinates.  The derivative is forward mode: every
// vertex coordinate carries five tangents (x, y, dx, dy, yaw of a) through the very same clip, so value and derivative
// take the same branches by construction.  Where a vertex of one rectangle lies on an edge of the other, where the
// z-intervals touch or an end of one coincides with an end of the other, the derivative is one-sided (the branch the
// value took).  A quadrilateral cut by four half-planes has at most 8 vertices; every store into the vertex buffers is
// guarded by that bound, so no input (NaN included: a NaN compares false, and flows through to the result) can index
// past them.
#pragma once
#include "ud_common.h"

namespace ud_riou {

constexpr int kTan = 5;           // tangents of the BEV part: x, y, dx, dy, yaw of box a
constexpr int kMaxVerts = 8;

// value + N tangents; N = 0 is the plain value (same operations on .v in the same order: bitwise the same number)
template <int N>
struct Jet {
  float v;
  float d[N > 0 ? N : 1];
};

template <int N>
__host__ __device__ __forceinline__ Jet<N> jconst(float v) {
  Jet<N> r;
  r.v = v;
  r.d[0] = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = 0.f;
  return r;
}
template <int N>
__host__ __device__ __forceinline__ Jet<N> operator+(const Jet<N>& a, const Jet<N>& b) {
  Jet<N> r = jconst<N>(a.v + b.v);
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] + b.d[i];
  return r;
}
template <int N>
__host__ __device__ __forceinline__ Jet<N> operator-(const Jet<N>& a, const Jet<N>& b) {
  Jet<N> r = jconst<N>(a.v - b.v);
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] - b.d[i];
  return r;
}
template <int N>
__host__ __device__ __forceinline__ Jet<N> operator*(const Jet<N>& a, const Jet<N>& b) {
  Jet<N> r = jconst<N>(a.v * b.v);
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
  return r;
}
template <int N>
__host__ __device__ __forceinline__ Jet<N> operator/(const Jet<N>& a, const Jet<N>& b) {
  Jet<N> r = jconst<N>(a.v / b.v);
  const float inv = 1.f / b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * inv;
  return r;
}

template <int N>
struct Vert {
  Jet<N> c[2];      // X, Y in the frame of box b
};

// Area of (rectangle a) ∩ (rectangle b); with N = kTan also its derivative by (x, y, dx, dy, yaw) of a.
template <int N>
__host__ __device__ __forceinline__ Jet<N> inter_bev(const float* a, const float* b) {
  // a in b's frame: centre (cx, cy), heading yr
  const float cb = cosf(b[6]), sb = sinf(b[6]);
  const float ex = a[0] - b[0], ey = a[1] - b[1];
  const float cx = cb * ex + sb * ey, cy = cb * ey - sb * ex;
  const float yr = a[6] - b[6];
  const float cr = cosf(yr), sr = sinf(yr);
  const float hx = 0.5f * a[3], hy = 0.5f * a[4];
  Vert<N> poly[kMaxVerts], tmp[kMaxVerts];
  const float sgx[4] = {-1.f, 1.f, 1.f, -1.f}, sgy[4] = {-1.f, -1.f, 1.f, 1.f};      // counter-clockwise
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float lx = sgx[k] * hx, ly = sgy[k] * hy;
    Jet<N> X = jconst<N>(cx + (lx * cr - ly * sr)), Y = jconst<N>(cy + (lx * sr + ly * cr));
    if constexpr (N == kTan) {
      X.d[0] = cb;                    Y.d[0] = -sb;                  // d / d x_a
      X.d[1] = sb;                    Y.d[1] = cb;                   // d / d y_a
      X.d[2] = 0.5f * sgx[k] * cr;    Y.d[2] = 0.5f * sgx[k] * sr;   // d / d dx_a
      X.d[3] = -0.5f * sgy[k] * sr;   Y.d[3] = 0.5f * sgy[k] * cr;   // d / d dy_a
      X.d[4] = -(lx * sr + ly * cr);  Y.d[4] = lx * cr - ly * sr;    // d / d yaw_a
    }
    poly[k].c[0] = X;
    poly[k].c[1] = Y;
  }
  int n = 4;
  const float bound[2] = {0.5f * b[3], 0.5f * b[4]};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int ax = e >> 1;                       // half-plane e: sg * c[ax] <= bound[ax]
    const float sg = (e & 1) ? -1.f : 1.f;
    const float h = bound[ax];
    int m = 0;
    for (int k = 0; k < n; ++k) {
      const Vert<N> s = poly[k], t = poly[(k + 1 == n) ? 0 : k + 1];
      const float ds = h - sg * s.c[ax].v, dt = h - sg * t.c[ax].v;       // >= 0: inside
      const bool is = ds >= 0.f, it = dt >= 0.f;
      if (is && m < kMaxVerts) tmp[m++] = s;
      if (is != it && m < kMaxVerts) {
        // crossing: the clipped coordinate is the bound itself, the other one is interpolated
        const Jet<N> js = jconst<N>(h) - jconst<N>(sg) * s.c[ax], jt = jconst<N>(h) - jconst<N>(sg) * t.c[ax];
        const Jet<N> u = js / (js - jt);
        tmp[m].c[ax] = jconst<N>(sg * h);
        tmp[m].c[1 - ax] = s.c[1 - ax] + u * (t.c[1 - ax] - s.c[1 - ax]);
        ++m;
      }
    }
    n = m;
    for (int k = 0; k < n; ++k) poly[k] = tmp[k];
  }
  if (n < 3) {
    // empty (or NaN corners: nothing compared inside): 0, unless a NaN has to flow through
    const float q = (cx + cy) + (cr + sr) + (hx + hy) + (bound[0] + bound[1]);
    return jconst<N>(q != q ? q : 0.f);
  }
  Jet<N> a2 = jconst<N>(0.f);
  for (int k = 0; k < n; ++k) {
    const Vert<N> s = poly[k], t = poly[(k + 1 == n) ? 0 : k + 1];
    a2 = a2 + (s.c[0] * t.c[1] - t.c[0] * s.c[1]);
  }
  const Jet<N> half = jconst<N>(a2.v < 0.f ? -0.5f : 0.5f);
  return half * a2;
}

// IoU3D_rot(a, b); with D also d[0..7) = d IoU / d (x, y, z, dx, dy, dz, yaw) of a (b is a constant; 0 where the IoU is NaN).
template <bool D>
__host__ __device__ __forceinline__ float iou3d(const float* a, const float* b, float* d) {
  const Jet<D ? kTan : 0> ib = inter_bev<D ? kTan : 0>(a, b);
  const float A = a[2] + 0.5f * a[5], B = b[2] + 0.5f * b[5], C = a[2] - 0.5f * a[5], E = b[2] - 0.5f * b[5];
  const float raw = fminf(A, B) - fmaxf(C, E);
  // fmaxf(NaN, 0) is 0: keep the NaN
  const float oz = raw != raw ? raw : fmaxf(raw, 0.f);
  const float inter = ib.v * oz;
  const float vb = b[3] * b[4] * b[5];
  const float U = a[3] * a[4] * a[5] + vb - inter;
  const float Uc = U != U ? U : fmaxf(U, 1e-8f);
  const float iou = inter / Uc;
  if constexpr (D) {
    const float on = raw > 0.f ? 1.f : 0.f;
    const float hi = A <= B ? 1.f : 0.f, lo = C >= E ? 1.f : 0.f;
    const float doz_dz = on * (hi - lo), doz_ddz = on * (0.5f * hi + 0.5f * lo);
    const bool free_u = U >= 1e-8f;
    const float di_dinter = free_u ? (Uc + inter) / (Uc * Uc) : 1.f / Uc;
    const float di_dva = free_u ? -inter / (Uc * Uc) : 0.f;
    d[0] = di_dinter * (oz * ib.d[0]);
    d[1] = di_dinter * (oz * ib.d[1]);
    d[2] = di_dinter * (ib.v * doz_dz);
    d[3] = di_dinter * (oz * ib.d[2]) + di_dva * (a[4] * a[5]);
    d[4] = di_dinter * (oz * ib.d[3]) + di_dva * (a[3] * a[5]);
    d[5] = di_dinter * (ib.v * doz_ddz) + di_dva * (a[3] * a[4]);
    d[6] = di_dinter * (oz * ib.d[4]);
    if (iou != iou)                      // a NaN IoU has no derivative: report 0, not NaN
#pragma unroll
      for (int i = 0; i < 7; ++i) d[i] = 0.f;
  }
  return iou;
}

}  // namespace ud_riou
