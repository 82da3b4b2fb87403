// Camera augmentation: ImageAffineTransformation.forward (data/multisensorfusion/transforms3d.py:298-347)
// -> functional.img_transform (functional.py:560-592), i.e. PIL resize (BICUBIC, a = -0.5) -> crop (zero fill) ->
// optional FLIP_LEFT_RIGHT -> rotate (NEAREST, centre, black fill) of every camera frame, bit-exact to Pillow's C code.
//
// The host (ops/input_prep.py) derives what Pillow derives in double: per axis the 22-bit fixed-point bicubic tables
// (precompute_coeffs + normalize_coeffs_8bpc), and the 16.16 constants of the nearest-neighbour affine loop.  The
// kernels only do integer arithmetic on them:
//   k_ia_hpass: Pillow's horizontal pass (rounded and clamped to uint8), but only over the source rows the crop's
//               vertical windows touch and the resized columns inside the crop, into a uint8 workspace;
//   k_ia_vpass: per output pixel: rotate -> flip -> crop offset -> vertical taps over the workspace -> clip8
//               -> uint8, or the ImageNormalize arithmetic (image_norm.h) -> float32 NCHW / channels-last.
// NEAREST rotation maps output pixels to resized pixels almost one to one, so evaluating the vertical pass on demand
// costs about one vertical sum per output pixel.  One launch of each handles every frame of a batch (blockIdx.y).
#include "ud_common.h"
#include "ud_prof.h"
#include "image_norm.h"

namespace {

constexpr int kPrec = 22;                    // Pillow's PRECISION_BITS for 8 bpc resampling
constexpr int kHeader = 2;                   // table row: lo, count, ksize weights
constexpr int kPx = 4;                       // pixels per thread (12 bytes: three dword stores)

__device__ __forceinline__ unsigned ud_clip8(int v) {
  v >>= kPrec;
  return v < 0 ? 0u : (v > 255 ? 255u : (unsigned)v);
}

__host__ __device__ __forceinline__ long long ia_ws_row(long long ncols) { return (ncols + kPx - 1) / kPx * kPx * 3; }

// Store 4 RGB uint8 pixels (12 bytes) at p; vec: p is 4-byte aligned and all 4 pixels are in range.
__device__ __forceinline__ void ia_store_u8(unsigned char* p, const unsigned* v, int n, bool vec) {
  if (vec) {
    unsigned* q = (unsigned*)p;
    q[0] = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
    q[1] = v[4] | v[5] << 8 | v[6] << 16 | v[7] << 24;
    q[2] = v[8] | v[9] << 8 | v[10] << 16 | v[11] << 24;
  } else {
    for (int i = 0; i < 3 * n; ++i) p[i] = (unsigned char)v[i];
  }
}

// Horizontal pass.  Thread = 4 adjacent resized columns of one band row of one frame (blockIdx.y).
__global__ __launch_bounds__(256) void k_ia_hpass(const unsigned char* __restrict__ img, long long row_stride,
                                                  const UdImageAffineFrame* __restrict__ frames,
                                                  unsigned char* __restrict__ ws) {
  const UdImageAffineFrame& f = frames[blockIdx.y];
  const long long ncols = f.ncols, groups = (ncols + kPx - 1) / kPx;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= groups * f.band_rows) return;
  const long long r = t / groups, g = t - r * groups;
  const long long srow = f.band0 + r - f.src_row0;                    // row inside the stored source rows
  if (srow < 0 || srow >= f.src_rows) return;                         // launcher guarantees the band is stored
  const unsigned char* src = img + f.src_off + srow * row_stride;
  const int* tab = (const int*)f.htab;
  const int stride = kHeader + (int)f.hk;
  unsigned v[3 * kPx];
  const int n = (int)(ncols - g * kPx < kPx ? ncols - g * kPx : kPx);
#pragma unroll
  for (int j = 0; j < kPx; ++j) {
    if (j >= n) break;
    const int* e = tab + (long long)(f.col0 + g * kPx + j) * stride;
    const int lo = e[0], cnt = e[1];
    int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
    const unsigned char* p = src + (long long)lo * 3;
    for (int k = 0; k < cnt; ++k) {
      const int w = e[kHeader + k];
      s0 += (int)p[3 * k] * w;
      s1 += (int)p[3 * k + 1] * w;
      s2 += (int)p[3 * k + 2] * w;
    }
    v[3 * j] = ud_clip8(s0), v[3 * j + 1] = ud_clip8(s1), v[3 * j + 2] = ud_clip8(s2);
  }
  ia_store_u8(ws + f.ws_off + r * ia_ws_row(ncols) + g * kPx * 3, v, n, n == kPx);
}

// Vertical pass + rotate / flip / crop + output.  Thread = 4 adjacent output pixels of one row of one frame.
// out_mode 0: u8 [N][fH][fW][3]; 1: f32 [N][3][fH][fW]; 2: f32 [N][fH][fW][3].
__global__ __launch_bounds__(256) void k_ia_vpass(const UdImageAffineFrame* __restrict__ frames,
                                                  const unsigned char* __restrict__ ws, void* __restrict__ out,
                                                  int fH, int fW, int out_mode, int vec, UdNorm nm) {
  const UdImageAffineFrame& f = frames[blockIdx.y];
  const int groups = (fW + kPx - 1) / kPx;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= groups * fH) return;
  const int y = t / groups, x0 = (t - y * groups) * kPx;
  const int n = fW - x0 < kPx ? fW - x0 : kPx;
  const int* vt = (const int*)f.vtab;
  const int vstride = kHeader + (int)f.vk;
  const long long wrow = ia_ws_row(f.ncols);
  const unsigned char* wsf = ws + f.ws_off;
  const int rot = (int)f.rotate, flip = (int)f.flip;
  const int a0 = (int)f.a0, a1 = (int)f.a1, a2 = (int)f.a2, a3 = (int)f.a3, a4 = (int)f.a4, a5 = (int)f.a5;
  unsigned v[3 * kPx];
#pragma unroll
  for (int j = 0; j < kPx; ++j) {
    v[3 * j] = v[3 * j + 1] = v[3 * j + 2] = 0;                       // fill of rotate / crop
    if (j >= n) continue;
    int xs = x0 + j, ys = y;
    if (rot) {                                                        // Pillow's NN_AFFINE, 16.16 fixed point
      xs = (a2 + a1 * y + a0 * (x0 + j)) >> 16;
      ys = (a5 + a4 * y + a3 * (x0 + j)) >> 16;
      if (xs < 0 || xs >= fW || ys < 0 || ys >= fH) continue;
    }
    if (flip) xs = fW - 1 - xs;
    const long long xr = f.cx + xs, yr = f.cy + ys;                   // resized-image coordinates
    if (xr < f.col0 || xr >= f.col0 + f.ncols || yr < 0 || yr >= f.rh) continue;
    const int* e = vt + yr * vstride;
    const long long r0 = e[0] - f.band0;
    const int cnt = e[1];
    if (r0 < 0 || r0 + cnt > f.band_rows) continue;                   // launcher guarantees the band covers the taps
    const unsigned char* p = wsf + r0 * wrow + (xr - f.col0) * 3;
    int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
    for (int k = 0; k < cnt; ++k, p += wrow) {
      const int w = e[kHeader + k];
      s0 += (int)p[0] * w;
      s1 += (int)p[1] * w;
      s2 += (int)p[2] * w;
    }
    v[3 * j] = ud_clip8(s0), v[3 * j + 1] = ud_clip8(s1), v[3 * j + 2] = ud_clip8(s2);
  }
  const long long npix = (long long)fH * fW, pix = (long long)blockIdx.y * npix + (long long)y * fW + x0;
  const bool full = vec && n == kPx;
  if (out_mode == 0) {
    ia_store_u8((unsigned char*)out + pix * 3, v, n, full);
    return;
  }
  float o[3 * kPx];
#pragma unroll
  for (int j = 0; j < kPx; ++j) ud_norm_apply(nm, v[3 * j], v[3 * j + 1], v[3 * j + 2], o[3 * j], o[3 * j + 1], o[3 * j + 2]);
  if (out_mode == 2) {
    float* q = (float*)out + pix * 3;
    if (full) {
      float4* q4 = (float4*)q;
      q4[0] = make_float4(o[0], o[1], o[2], o[3]);
      q4[1] = make_float4(o[4], o[5], o[6], o[7]);
      q4[2] = make_float4(o[8], o[9], o[10], o[11]);
    } else {
      for (int i = 0; i < 3 * n; ++i) q[i] = o[i];
    }
  } else {
    float* q = (float*)out + (long long)blockIdx.y * 3 * npix + (long long)y * fW + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* qc = q + c * npix;
      if (full) {
        *(float4*)qc = make_float4(o[c], o[3 + c], o[6 + c], o[9 + c]);
      } else {
        for (int j = 0; j < n; ++j) qc[j] = o[3 * j + c];
      }
    }
  }
}

size_t ia_frame_ws_bytes(const UdImageAffineFrame& f) {
  return ud_align_up((size_t)(f.band_rows * ia_ws_row(f.ncols)), 16);
}

}  // namespace

extern "C" size_t ud_image_affine_workspace_bytes(const UdImageAffineFrame* frames, int N) {
  if (!frames || N <= 0) return 0;
  size_t n = 0;
  for (int i = 0; i < N; ++i) n += ia_frame_ws_bytes(frames[i]);
  return n;
}

// Every read the kernels make is bounded by these checks: the band lies in the stored source rows and those in the
// input, the workspace regions lie in the workspace, the crop columns lie in the resized image, the fixed-point
// products fit in int32.  Pure host function of the records (the launcher runs it before anything is launched).
extern "C" int ud_image_affine_check(const UdImageAffineFrame* frames_host, int N, int64_t img_bytes, int H, int W,
                                     int64_t row_stride, int fH, int fW, size_t workspace_bytes) {
  if (N == 0) return UD_OK;
  if (!frames_host || N < 0 || N > 65535 || H <= 0 || W <= 0 || row_stride < 3LL * W || fH <= 0 || fW <= 0 ||
      fH > 8192 || fW > 8192)
    return UD_ERR_INVALID_ARG;
  for (int i = 0; i < N; ++i) {
    const UdImageAffineFrame& f = frames_host[i];
    if (f.rw <= 0 || f.rh <= 0 || f.hk < 1 || f.vk < 1 || f.hk > 4096 || f.vk > 4096 || f.flip < 0 || f.flip > 1 ||
        f.rotate < 0 || f.rotate > 1 || f.ncols < 0 || f.band_rows < 0 || f.src_rows < 0 || f.src_off < 0 ||
        f.ws_off < 0 || f.ws_off % 16 || f.src_row0 < 0 || f.src_row0 + f.src_rows > H ||
        (f.src_rows > 0 && f.src_off + (f.src_rows - 1) * row_stride + 3LL * W > img_bytes))
      return UD_ERR_INVALID_ARG;
    if (f.ncols > 0) {
      if (!f.htab || !f.vtab || f.col0 < 0 || f.col0 + f.ncols > f.rw || f.band0 < 0 || f.band0 + f.band_rows > H ||
          f.band0 < f.src_row0 || f.band0 + f.band_rows > f.src_row0 + f.src_rows)
        return UD_ERR_INVALID_ARG;
      if ((size_t)f.ws_off + ia_frame_ws_bytes(f) > workspace_bytes) return UD_ERR_WORKSPACE;
    }
  }
  return UD_OK;
}

extern "C" int ud_image_affine(const unsigned char* img, int64_t img_bytes, int H, int W, int64_t row_stride,
                               const UdImageAffineFrame* frames_host, const UdImageAffineFrame* frames_dev, int N,
                               int fH, int fW, int out_mode, void* out, const float* mean, const float* std,
                               int to_rgb, void* workspace, size_t workspace_bytes, ud_stream_t stream_) {
  if (N == 0) return UD_OK;
  if (!img || !frames_host || !frames_dev || !out || out_mode < 0 || out_mode > 2 || (uintptr_t)workspace % 16)
    return UD_ERR_INVALID_ARG;
  const int rc = ud_image_affine_check(frames_host, N, img_bytes, H, W, row_stride, fH, fW, workspace_bytes);
  if (rc != UD_OK) return rc;
  UdNorm nm = {};
  if (out_mode != 0) {
    if (!mean || !std) return UD_ERR_INVALID_ARG;
    for (int c = 0; c < 3; ++c)
      if (!(std[c] != 0.0f)) return UD_ERR_INVALID_ARG;
    nm = ud_norm_make(mean, std, to_rgb);
  }
  long long max_h = 0;
  for (int i = 0; i < N; ++i) {
    const UdImageAffineFrame& f = frames_host[i];
    const long long h = f.ncols > 0 ? f.band_rows * ((f.ncols + kPx - 1) / kPx) : 0;
    max_h = h > max_h ? h : max_h;
  }
  if (max_h > 0 && !workspace) return UD_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  unsigned char* ws = (unsigned char*)workspace;
  const int vec = fW % kPx == 0 && (uintptr_t)out % 16 == 0;
  UdProfScope prof("input.k_image_affine", stream);
  if (max_h > 0) {
    k_ia_hpass<<<dim3((unsigned)ud_div_up(max_h, 256), N), 256, 0, stream>>>(img, row_stride, frames_dev, ws);
    UD_LAUNCH_CHECK();
  }
  const long long vthreads = (long long)fH * ((fW + kPx - 1) / kPx);
  k_ia_vpass<<<dim3((unsigned)ud_div_up(vthreads, 256), N), 256, 0, stream>>>(frames_dev, ws, out, fH, fW, out_mode,
                                                                                vec, nm);
  UD_LAUNCH_CHECK();
  return UD_OK;
}
