// Depth metric of the camera student's LSS lift for MI355X / gfx950: the monocular-depth figures (abs-rel, RMSE,
// delta < 1.25^k, ...) of the depth net's distribution against the LiDAR minimum depth, accumulated on the device.
//   ud_depth_metric_accumulate   state f64[groups, ranges, 12] += the twelve sums of this batch's labelled pixels
//
// Per labelled pixel (dmin finite and floor((dmin - d_lo) / d_step) in [0, D): k_depth_convert's expression in depth_sup.hip),
// in fp32 as the loss kernel does: p = softmax over the D logits with the maximum subtracted, the arg-max bin (lowest index on
// a tie), and the EXPECTED DEPTH OVER THE BIN CENTRES
//   dhat = sum_j p_j * (d_lo + (j + 0.5) * d_step)
// -- centres, because label bin j covers [d_lo + j * d_step, d_lo + (j + 1) * d_step): with the frustum's left edges a perfect
// one-hot prediction would sit half a bin short of every depth it was trained on.  exp, p_j and dhat are fp32 values; the two
// sums over D (the softmax's denominator and dhat) are carried in fp64 and rounded to fp32 once, so that they do not depend on
// the order the two kernels below add in.  The error terms are then formed in fp64 from that fp32 dhat.  The softmax is never
// stored.
//
// Reduction: every 64 consecutive pixels of one image are a slice.  A workgroup lays the twelve terms of its slice's pixels
// out in LDS and adds them per (range, term) column in ascending pixel order into one fp64 row of the workspace; the rows of
// the images of a group are added by ud_reduce.h's fixed-order column sum and accumulated into the state.  The slices are a
// function of (BN, fH, fW) alone and both kernels below cut them alike, so the result depends neither on the grid nor on the
// device; no floating-point atomics.  Two launches.
#include <math.h>
#include "ud_common.h"
#include "ud_prof.h"
#include "ud_reduce.h"

namespace {

constexpr int DM_TERMS = 12;
constexpr int DM_SLICE = 64;               // pixels per slice: one per lane (NCHW), 16 per wave of four (channels-last)
constexpr int DM_MAX_RANGES = 8;

struct DmRanges {                          // by value in the launch: no device read, no copy
  double edge[DM_MAX_RANGES + 1];
  int n;
};

// k_depth_convert's rule (depth_sup.hip): the bin of a finite dmin, -1 where the pixel has no label
__device__ __forceinline__ int dm_bin(float dmin, double d_lo, double d_step, int D) {
  if (!isfinite(dmin)) return -1;
  const double k = floor(((double)dmin - d_lo) / d_step);
  return (k >= 0.0 && k < (double)D) ? (int)k : -1;
}

__device__ __forceinline__ int dm_range(double d, const DmRanges& rg) {
  for (int r = 0; r < rg.n; ++r)
    if (d >= rg.edge[r] && d < rg.edge[r + 1]) return r;
  return -1;
}

__device__ __forceinline__ float dm_centre(int j, double d_lo, double d_step) { return (float)(d_lo + ((double)j + 0.5) * d_step); }

// the twelve terms of one labelled pixel, fp64 from the fp32 dhat and p_b
__device__ __forceinline__ void dm_terms(float dhat, int ahat, float pb, double d, int b, double* __restrict__ t) {
  const double dh = (double)dhat, e = dh - d, ae = fabs(e), lg = log(dh) - log(d), ratio = fmax(dh / d, d / dh);
  const int da = ahat > b ? ahat - b : b - ahat;
  t[0] = 1.0;
  t[1] = ae;
  t[2] = ae / d;
  t[3] = (e * e) / d;
  t[4] = e * e;
  t[5] = lg * lg;
  t[6] = ratio < 1.25 ? 1.0 : 0.0;
  t[7] = ratio < 1.5625 ? 1.0 : 0.0;          // 1.25^2
  t[8] = ratio < 1.953125 ? 1.0 : 0.0;        // 1.25^3
  t[9] = da == 0 ? 1.0 : 0.0;
  t[10] = da <= 1 ? 1.0 : 0.0;
  t[11] = -log(fmax((double)pb, 1e-44));
}

// terms[pixel of the slice][12] and range_of[pixel] (-1: not counted) in LDS -> one row of the workspace: column (r, t) is the
// sum, in ascending pixel order, over the slice's pixels of range r.  Every column is written, so the workspace needs no clearing.
__device__ __forceinline__ void dm_slice_row(const double* __restrict__ terms, const int* __restrict__ range_of, int n_ranges,
                                             double* __restrict__ row) {
  for (int c = threadIdx.x; c < n_ranges * DM_TERMS; c += blockDim.x) {
    const int r = c / DM_TERMS, t = c - r * DM_TERMS;
    double a = 0.0;
    for (int l = 0; l < DM_SLICE; ++l)
      if (range_of[l] == r) a += terms[l * DM_TERMS + t];
    row[c] = a;
  }
}

// row of the workspace that image n's slice blk goes to: [group][image of the group][slice][ranges * 12]
__device__ __forceinline__ size_t dm_row_index(int n, int blk, int nblk, int BN, int groups) {
  const int g = n % groups, i = n / groups;
  return ((size_t)g * (BN / groups) + i) * nblk + blk;
}

// NCHW (any strides with sc != 1): one lane per pixel walks D, the 64 lanes of a row read 64 consecutive floats.
// Three passes over the pixel's logits (maximum and arg-max; sum of exp; p_j and the expectation): the second and third hit the cache.
__global__ __launch_bounds__(DM_SLICE) void k_depth_metric_nchw(const float* __restrict__ x, long long sn, long long sc,
                                                                long long sh, long long sw, const float* __restrict__ dmin,
                                                                int BN, int D, int fW, int HW, int nblk, int groups,
                                                                double d_lo, double d_step, DmRanges rg,
                                                                double* __restrict__ partial) {
  __shared__ double terms[DM_SLICE * DM_TERMS];
  __shared__ int range_of[DM_SLICE];
  const int lane = threadIdx.x, n = blockIdx.x / nblk, blk = blockIdx.x - n * nblk;
  const int hw = blk * DM_SLICE + lane;
  int r = -1;
  if (hw < HW) {
    const float dm = dmin[(size_t)n * HW + hw];
    const int b = dm_bin(dm, d_lo, d_step, D);
    if (b >= 0) r = dm_range((double)dm, rg);
    if (r >= 0) {
      const int h = hw / fW, w = hw - h * fW;
      const float* px = x + n * sn + h * sh + w * sw;
      float mx = -INFINITY;
      int ahat = 0;
      for (int j = 0; j < D; ++j) {
        const float v = px[j * sc];
        if (v > mx) { mx = v; ahat = j; }          // strict: the lowest index wins a tie
      }
      double sum64 = 0.0, dhat64 = 0.0;
      for (int j = 0; j < D; ++j) sum64 += (double)expf(px[j * sc] - mx);
      const float sum = (float)sum64;
      float pb = 0.f;
      for (int j = 0; j < D; ++j) {
        const float p = __fdiv_rn(expf(px[j * sc] - mx), sum);
        dhat64 += (double)p * (double)dm_centre(j, d_lo, d_step);
        if (j == b) pb = p;
      }
      dm_terms((float)dhat64, ahat, pb, (double)dm, b, terms + lane * DM_TERMS);
    }
  }
  range_of[lane] = r;
  __syncthreads();
  dm_slice_row(terms, range_of, rg.n, partial + dm_row_index(n, blk, nblk, BN, groups) * (rg.n * DM_TERMS));
}

__device__ __forceinline__ float dm_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ double dm_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Channels-last (sc == 1): a wave per pixel reads its D logits as one contiguous row, lane l holding bins l, l + 64, ...;
// the four waves of a workgroup take 16 pixels each of the slice.
__global__ __launch_bounds__(256) void k_depth_metric_cl(const float* __restrict__ x, long long sn, long long sh, long long sw,
                                                         const float* __restrict__ dmin, int BN, int D, int fW, int HW,
                                                         int nblk, int groups, double d_lo, double d_step, DmRanges rg,
                                                         double* __restrict__ partial) {
  __shared__ double terms[DM_SLICE * DM_TERMS];
  __shared__ int range_of[DM_SLICE];
  const int lane = ud_lane(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = blockIdx.x / nblk, blk = blockIdx.x - n * nblk;
  for (int k = 0; k < DM_SLICE / 4; ++k) {
    const int slot = wave * (DM_SLICE / 4) + k, hw = blk * DM_SLICE + slot;       // wave-uniform
    int r = -1;
    if (hw < HW) {
      const float dm = dmin[(size_t)n * HW + hw];
      const int b = dm_bin(dm, d_lo, d_step, D);
      if (b >= 0) r = dm_range((double)dm, rg);
      if (r >= 0) {
        const int h = hw / fW, w = hw - h * fW;
        const float* px = x + n * sn + h * sh + w * sw;
        float v[4], mx = -INFINITY;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int j = lane + 64 * s;
          v[s] = j < D ? px[j] : -INFINITY;
          mx = fmaxf(mx, v[s]);
        }
        mx = dm_wave_max(mx);
        int ahat = D;
        float e[4];
        double sum64 = 0.0, dhat64 = 0.0;
#pragma unroll
        for (int s = 3; s >= 0; --s) {
          const int j = lane + 64 * s;
          if (j < D && v[s] == mx) ahat = j;         // descending s: the lane's lowest bin at the maximum
          e[s] = j < D ? expf(v[s] - mx) : 0.f;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) sum64 += (double)e[s];
        ahat = ud_wave_min(ahat);
        if (ahat >= D) ahat = 0;                     // no bin compares equal (NaN logits): what the lane-per-pixel walk gives
        const float sum = (float)dm_wave_sum_d(sum64);
        float pbl = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int j = lane + 64 * s;
          const float p = __fdiv_rn(e[s], sum);
          if (j < D) dhat64 += (double)p * (double)dm_centre(j, d_lo, d_step);
          if (j == b) pbl = p;
        }
        const float dhat = (float)dm_wave_sum_d(dhat64), pb = ud_wave_sum(pbl);   // pbl: one lane's value, an exact broadcast
        if (lane == 0) dm_terms(dhat, ahat, pb, (double)dm, b, terms + slot * DM_TERMS);
      }
    }
    if (lane == 0) range_of[slot] = r;
  }
  __syncthreads();
  dm_slice_row(terms, range_of, rg.n, partial + dm_row_index(n, blk, nblk, BN, groups) * (rg.n * DM_TERMS));
}

int dm_slices_per_image(int fH, int fW) { return ud_div_up((long long)fH * fW, DM_SLICE); }

}  // namespace

extern "C" size_t ud_depth_metric_workspace_bytes(int BN, int fH, int fW) {
  if (BN <= 0 || fH <= 0 || fW <= 0) return 0;
  return ud_align_up((size_t)BN * dm_slices_per_image(fH, fW) * DM_MAX_RANGES * DM_TERMS * sizeof(double));
}

extern "C" int ud_depth_metric_accumulate(const float* logits, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                                          const float* dmin, int BN, int D, int fH, int fW, int ncam_groups, double d_lo,
                                          double d_step, const double* range_edges, int n_ranges, double* state,
                                          void* workspace, size_t workspace_bytes, ud_stream_t stream_) {
  if (BN < 0 || fH < 0 || fW < 0 || D < 1 || D > 256 || n_ranges < 1 || n_ranges > DM_MAX_RANGES || ncam_groups < 1 ||
      BN % ncam_groups != 0 || !range_edges || !state || !(d_step > 0.0) || !__builtin_isfinite(d_lo) || !__builtin_isfinite(d_step))
    return UD_ERR_INVALID_ARG;
  DmRanges rg;
  rg.n = n_ranges;
  for (int r = 0; r <= n_ranges; ++r) {
    rg.edge[r] = range_edges[r];
    if (rg.edge[r] != rg.edge[r] || (r > 0 && !(rg.edge[r] > rg.edge[r - 1]))) return UD_ERR_INVALID_ARG;   // NaN / not ascending
  }
  for (int r = n_ranges + 1; r <= DM_MAX_RANGES; ++r) rg.edge[r] = rg.edge[n_ranges];
  if (BN == 0 || fH == 0 || fW == 0) return UD_OK;
  if (!logits || !dmin || (long long)BN * fH * fW >= (1ll << 31)) return UD_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < ud_depth_metric_workspace_bytes(BN, fH, fW)) return UD_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int HW = fH * fW, nblk = dm_slices_per_image(fH, fW);
  const long long blocks = (long long)BN * nblk;
  double* partial = (double*)workspace;
  {
    UdProfScope prof("depth_metric.k_depth_metric", stream);
    if (sc == 1)
      k_depth_metric_cl<<<(unsigned)blocks, 256, 0, stream>>>(logits, sn, sh, sw, dmin, BN, D, fW, HW, nblk, ncam_groups, d_lo,
                                                              d_step, rg, partial);
    else
      k_depth_metric_nchw<<<(unsigned)blocks, DM_SLICE, 0, stream>>>(logits, sn, sc, sh, sw, dmin, BN, D, fW, HW, nblk,
                                                                     ncam_groups, d_lo, d_step, rg, partial);
    UD_LAUNCH_CHECK();
  }
  return ud_colsum_accum_f64(partial, ncam_groups, (BN / ncam_groups) * nblk, n_ranges * DM_TERMS, state, stream);
}
