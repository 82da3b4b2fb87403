// LiDAR depth supervision of the camera student's LSS lift (the BEVDepth recipe) for MI355X / gfx950:
//   ud_depth_labels    the collated cloud projected into every key-frame image -> per-cell minimum depth and depth-bin label
//   ud_depth_loss_fwd  softmax over the D depth logits + binary cross entropy against the one-hot label, mean over the
//                      labelled pixels, bitwise reproducible
//   ud_depth_loss_bwd  its gradient with respect to the logits, one launch
//
// The projection is the inverse of the chain LSSFPN.get_geometry runs forward (lss_geom.h): per sample b and camera c
//   q = (bda_b . sensor2ego_bc)^-1 . (x, y, z, 1)        camera frame
//   (x', y', w) = K_bc . q  (upper 3x3 of intrin)         u0 = x' / w, v0 = y' / w
//   (u, v, d, 1) = ida_bc . (u0, v0, q.z, 1)
// evaluated in fp64 with separately rounded products and sums in the order written below (the build sets -ffp-contract=off),
// so that a float64 restatement on the host reproduces every comparison (tests/depth_sup_ref.py).  d is rounded to fp32 once;
// positive floats order like their bit patterns, so an unsigned atomicMin on the bits gives the minimum whatever the order of
// the points: the result is bitwise reproducible.
#include "ud_common.h"
#include "ud_prof.h"
#include "lss_geom.h"
#include "ud_reduce.h"

namespace {

// per (b, c): P = K3 . Minv[0:3] (3 x 4), row z of Minv (4), rows 0..2 of ida (3 x 4); Minv = (bda . sensor2ego)^-1
constexpr int DS_CAM_DOUBLES = 28;
constexpr unsigned DS_EMPTY = 0xFFFFFFFFu;
constexpr int DS_PIX_PER_WAVE = 4;          // pixels a wave of the loss kernels walks; 4 waves per workgroup

__device__ __forceinline__ double ds_row4(const double* __restrict__ m, double x, double y, double z) {
  return ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
}

// Two independent jobs in one launch (neither is worth a launch of its own): every thread fills the depth cells with all-ones
// (a kernel, not a memset node: see k_ud_zero_f32 in ud_common.h), the first B * ncam threads build the projections.
__global__ __launch_bounds__(256) void k_depth_setup(const float* __restrict__ s2e, const float* __restrict__ intrin,
                                                     const float* __restrict__ ida, const float* __restrict__ bda,
                                                     double* __restrict__ proj, int B, int ncam,
                                                     unsigned* __restrict__ cells, size_t ncells) {
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (size_t i = gid; i < ncells; i += (size_t)gridDim.x * 256) cells[i] = DS_EMPTY;
  if (gid >= (size_t)B * ncam) return;
  const int b = (int)gid / ncam;
  const float* s = s2e + gid * 16;
  double m[16], minv[16];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      if (bda) {
        const float* a = bda + (size_t)b * 16 + r * 4;
        double acc = (double)a[0] * (double)s[c];
        for (int k = 1; k < 4; ++k) acc += (double)a[k] * (double)s[k * 4 + c];
        m[r * 4 + c] = acc;
      } else {
        m[r * 4 + c] = (double)s[r * 4 + c];
      }
    }
  if (!ud_inv4x4(m, minv))
    for (int k = 0; k < 16; ++k) minv[k] = __builtin_nan("");      // a singular rig labels nothing
  double* o = proj + gid * DS_CAM_DOUBLES;
  const float* K = intrin + gid * 16;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) {
      double acc = (double)K[r * 4 + 0] * minv[c];
      acc += (double)K[r * 4 + 1] * minv[4 + c];
      acc += (double)K[r * 4 + 2] * minv[8 + c];
      o[r * 4 + c] = acc;
    }
  for (int c = 0; c < 4; ++c) o[12 + c] = minv[8 + c];
  for (int k = 0; k < 12; ++k) o[16 + k] = (double)ida[gid * 16 + k];
}

// One point per lane, the cameras in a loop (their 28 doubles are wave-uniform loads).  A plain load skips the atomic when the
// cell already holds a smaller depth: a few thousand cells take hundreds of thousands of candidates, and a stale larger value
// only costs the atomic it would have saved.
__global__ __launch_bounds__(256) void k_depth_project(const float* __restrict__ pts, long long sb, long long sn, int Nmax,
                                                       const double* __restrict__ proj, int ncam, int fH, int fW, double H,
                                                       double W, double ds, double d_lo, double d_hi,
                                                       unsigned* __restrict__ cells) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Nmax) return;
  const float* p = pts + b * sb + i * sn;
  const float xf = p[0], yf = p[1], zf = p[2];
  if (xf == 0.f && yf == 0.f && zf == 0.f) return;                 // collate padding
  if (!(isfinite(xf) && isfinite(yf) && isfinite(zf))) return;
  const double x = xf, y = yf, z = zf;
  for (int c = 0; c < ncam; ++c) {
    const double* m = proj + (size_t)(b * ncam + c) * DS_CAM_DOUBLES;
    const double xp = ds_row4(m, x, y, z), yp = ds_row4(m + 4, x, y, z), w = ds_row4(m + 8, x, y, z);
    const double qz = ds_row4(m + 12, x, y, z);
    const double u0 = xp / w, v0 = yp / w;
    const double u = ((m[16] * u0 + m[17] * v0) + m[18] * qz) + m[19];
    const double v = ((m[20] * u0 + m[21] * v0) + m[22] * qz) + m[23];
    const double d = ((m[24] * u0 + m[25] * v0) + m[26] * qz) + m[27];
    if (!(isfinite(u) && isfinite(v) && isfinite(d))) continue;
    if (!(d >= d_lo && d < d_hi && u >= 0.0 && u < W && v >= 0.0 && v < H)) continue;
    const int fh = (int)floor(v / ds), fw = (int)floor(u / ds);
    if (fh >= fH || fw >= fW) continue;                            // final_dim not a multiple of the downsample factor
    const unsigned bits = __float_as_uint((float)d);
    unsigned* cell = cells + ((size_t)(b * ncam + c) * fH + fh) * fW + fw;
    if (__hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > bits) atomicMin(cell, bits);
  }
}

// cells (bit patterns) -> dmin in place (+inf where no point fell) and the bin label, -1 where empty or outside [0, D)
__global__ __launch_bounds__(256) void k_depth_convert(unsigned* __restrict__ cells, int32_t* __restrict__ label, size_t n,
                                                       double d_lo, double d_step, int D) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned v = cells[i];
  if (v == DS_EMPTY) {
    cells[i] = 0x7F800000u;
    label[i] = -1;
    return;
  }
  const double k = floor(((double)__uint_as_float(v) - d_lo) / d_step);
  label[i] = (k >= 0.0 && k < (double)D) ? (int32_t)k : -1;
}

__device__ __forceinline__ float ds_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// softmax over the D logits of one pixel, spread over the lanes of a wave: pr[s] = p[lane + 64 s] (0 beyond D)
__device__ __forceinline__ void ds_pixel_softmax(const float* __restrict__ px, long long sc, int D, int lane, float* pr) {
  float v[4], mx = -INFINITY;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int d = lane + 64 * s;
    v[s] = d < D ? px[d * sc] : -INFINITY;
    mx = fmaxf(mx, v[s]);
  }
  mx = ds_wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    pr[s] = (lane + 64 * s) < D ? expf(v[s] - mx) : 0.f;
    sum += pr[s];
  }
  sum = ud_wave_sum(sum);
#pragma unroll
  for (int s = 0; s < 4; ++s) pr[s] = __fdiv_rn(pr[s], sum);
}

// A wave per pixel (channels-last logits: one coalesced row of D floats; NCHW: a strided gather, correct but not the fast case),
// DS_PIX_PER_WAVE pixels per wave.  partial[block] = (sum of the labelled pixels' BCE sums, number of labelled pixels); the
// pixels' fp32 sums are added in fp64 in a fixed order and rounded once per block.
__global__ __launch_bounds__(256) void k_depth_loss_fwd(const float* __restrict__ x, long long sn, long long sc, long long sh,
                                                        long long sw, const int32_t* __restrict__ label, long long npix, int D,
                                                        int fH, int fW, float* __restrict__ partial) {
  __shared__ double red[4][2];
  const int lane = ud_lane(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long pix0 = ((long long)blockIdx.x * 4 + wave) * DS_PIX_PER_WAVE;
  const int HW = fH * fW;
  double acc = 0.0, cnt = 0.0;
  for (int k = 0; k < DS_PIX_PER_WAVE; ++k) {
    const long long pix = pix0 + k;
    if (pix >= npix) break;
    const int l = __builtin_amdgcn_readfirstlane(label[pix]);     // one label per wave
    if (l < 0 || l >= D) continue;
    const int bn = (int)(pix / HW), r = (int)(pix - (long long)bn * HW), h = r / fW, w = r - h * fW;
    float pr[4];
    ds_pixel_softmax(x + bn * sn + h * sh + w * sw, sc, D, lane, pr);
    float part = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int d = lane + 64 * s;
      if (d < D) part -= fmaxf(d == l ? logf(pr[s]) : logf(1.0f - pr[s]), -100.0f);   // binary_cross_entropy's clamp
    }
    acc += (double)ud_wave_sum(part);
    cnt += 1.0;
  }
  if (lane == 0) { red[wave][0] = acc; red[wave][1] = cnt; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  acc = red[0][0], cnt = red[0][1];
#pragma unroll
  for (int wv = 1; wv < 4; ++wv) { acc += red[wv][0]; cnt += red[wv][1]; }
  partial[(size_t)blockIdx.x * 2 + 0] = (float)acc;
  partial[(size_t)blockIdx.x * 2 + 1] = (float)cnt;
}

// dL/dp_j = (p_j - t_j) / max((1 - p_j) p_j, 1e-12) * (grad_out / max(1, |fg|)), pushed through the softmax:
// dx_j = p_j (g_j - sum_k p_k g_k); exact zeros where the pixel has no label.
__global__ __launch_bounds__(256) void k_depth_loss_bwd(const float* __restrict__ x, long long sn, long long sc, long long sh,
                                                        long long sw, const int32_t* __restrict__ label,
                                                        const float* __restrict__ result, const float* __restrict__ grad_out,
                                                        float* __restrict__ dx, long long dn, long long dc, long long dh,
                                                        long long dw, long long npix, int D, int fH, int fW) {
  const int lane = ud_lane(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long pix0 = ((long long)blockIdx.x * 4 + wave) * DS_PIX_PER_WAVE;
  const int HW = fH * fW;
  const float gs = __fdiv_rn(grad_out[0], fmaxf(result[1], 1.0f));
  for (int k = 0; k < DS_PIX_PER_WAVE; ++k) {
    const long long pix = pix0 + k;
    if (pix >= npix) break;
    const int l = __builtin_amdgcn_readfirstlane(label[pix]);     // one label per wave
    const int bn = (int)(pix / HW), r = (int)(pix - (long long)bn * HW), h = r / fW, w = r - h * fW;
    float* po = dx + bn * dn + h * dh + w * dw;
    if (l < 0 || l >= D) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (lane + 64 * s < D) po[(lane + 64 * s) * dc] = 0.f;
      continue;
    }
    float pr[4], g[4];
    ds_pixel_softmax(x + bn * sn + h * sh + w * sw, sc, D, lane, pr);
    float dot = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int d = lane + 64 * s;
      const float t = d == l ? 1.0f : 0.0f;
      g[s] = d < D ? __fdiv_rn(pr[s] - t, fmaxf((1.0f - pr[s]) * pr[s], 1e-12f)) * gs : 0.f;
      dot += pr[s] * g[s];
    }
    dot = ud_wave_sum(dot);
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (lane + 64 * s < D) po[(lane + 64 * s) * dc] = pr[s] * (g[s] - dot);
  }
}

bool labels_ok(int B, int Nmax, int ncam, int H, int W, int ds, double d_lo, double d_hi, double d_step, int D) {
  return B > 0 && B <= 65535 && Nmax >= 0 && ncam > 0 && H > 0 && W > 0 && ds > 0 && H / ds > 0 && W / ds > 0 && D > 0 &&
         d_lo >= 0.0 && d_hi > d_lo && d_step > 0.0 && (long long)B * ncam * (H / ds) * (W / ds) < (1ll << 31);
}

bool loss_ok(int BN, int D, int fH, int fW) {
  return BN > 0 && D > 0 && D <= 256 && fH > 0 && fW > 0 && (long long)BN * fH * fW < (1ll << 31);
}

int loss_blocks(int BN, int fH, int fW) { return ud_div_up((long long)BN * fH * fW, 4 * DS_PIX_PER_WAVE); }

}  // namespace

extern "C" size_t ud_depth_labels_workspace_bytes(int B, int ncam) {
  if (B <= 0 || ncam <= 0) return 0;
  return ud_align_up((size_t)B * ncam * DS_CAM_DOUBLES * sizeof(double));
}

extern "C" int ud_depth_labels(const float* points, int64_t stride_b, int64_t stride_n, int B, int Nmax,
                               const float* sensor2ego, const float* intrin, const float* ida, const float* bda, int ncam,
                               int H, int W, int downsample, double d_lo, double d_hi, double d_step, int D, float* dmin,
                               int32_t* label, void* workspace, size_t workspace_bytes, ud_stream_t stream_) {
  if (!sensor2ego || !intrin || !ida || !dmin || !label || !labels_ok(B, Nmax, ncam, H, W, downsample, d_lo, d_hi, d_step, D))
    return UD_ERR_INVALID_ARG;
  if (Nmax > 0 && !points) return UD_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < ud_depth_labels_workspace_bytes(B, ncam)) return UD_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int fH = H / downsample, fW = W / downsample;
  const size_t ncells = (size_t)B * ncam * fH * fW;
  double* proj = (double*)workspace;
  unsigned* cells = reinterpret_cast<unsigned*>(dmin);
  const int setup_blocks = ud_div_up((long long)(ncells > (size_t)B * ncam ? ncells : (size_t)B * ncam), 256);
  k_depth_setup<<<setup_blocks < 1024 ? setup_blocks : 1024, 256, 0, stream>>>(sensor2ego, intrin, ida, bda, proj, B, ncam,
                                                                                cells, ncells);
  UD_LAUNCH_CHECK();
  if (Nmax > 0) {
    UdProfScope prof("depth_sup.k_depth_project", stream);
    k_depth_project<<<dim3(ud_div_up(Nmax, 256), B), 256, 0, stream>>>(points, stride_b, stride_n, Nmax, proj, ncam, fH, fW,
                                                                       (double)H, (double)W, (double)downsample, d_lo, d_hi,
                                                                       cells);
    UD_LAUNCH_CHECK();
  }
  k_depth_convert<<<ud_div_up((long long)ncells, 256), 256, 0, stream>>>(cells, label, ncells, d_lo, d_step, D);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

extern "C" size_t ud_depth_loss_workspace_bytes(int BN, int fH, int fW) {
  if (BN <= 0 || fH <= 0 || fW <= 0) return 0;
  return ud_align_up((size_t)loss_blocks(BN, fH, fW) * 2 * sizeof(float));
}

extern "C" int ud_depth_loss_fwd(const float* logits, int64_t sn, int64_t sc, int64_t sh, int64_t sw, const int32_t* label,
                                 int BN, int D, int fH, int fW, float* result, void* workspace, size_t workspace_bytes,
                                 ud_stream_t stream_) {
  if (!logits || !label || !result || !loss_ok(BN, D, fH, fW)) return UD_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < ud_depth_loss_workspace_bytes(BN, fH, fW)) return UD_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int blocks = loss_blocks(BN, fH, fW);
  float* partial = (float*)workspace;
  {
    UdProfScope prof("depth_sup.k_depth_loss_fwd", stream);
    k_depth_loss_fwd<<<blocks, 256, 0, stream>>>(logits, sn, sc, sh, sw, label, (long long)BN * fH * fW, D, fH, fW, partial);
    UD_LAUNCH_CHECK();
  }
  return ud_mean_final(partial, blocks, result, stream);
}

extern "C" int ud_depth_loss_bwd(const float* logits, int64_t sn, int64_t sc, int64_t sh, int64_t sw, const int32_t* label,
                                 const float* result, const float* grad_out, float* dx, int64_t dn, int64_t dc, int64_t dh,
                                 int64_t dw, int BN, int D, int fH, int fW, ud_stream_t stream_) {
  if (!logits || !label || !result || !grad_out || !dx || !loss_ok(BN, D, fH, fW)) return UD_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("depth_sup.k_depth_loss_bwd", stream);
  k_depth_loss_bwd<<<loss_blocks(BN, fH, fW), 256, 0, stream>>>(logits, sn, sc, sh, sw, label, result, grad_out, dx, dn, dc,
                                                                dh, dw, (long long)BN * fH * fW, D, fH, fW);
  UD_LAUNCH_CHECK();
  return UD_OK;
}
