// GT-sampling collision selection on the device: which database candidates may be pasted into a scene.
// The rule is OpenPCDet's DataBaseSampler (sample_with_fixed_number + the valid mask of its __call__), not a greedy
// NMS: the groups (one per sampler_groups entry; a group is a run of equal ids in cand_group) are processed in order,
// and a candidate of group g is accepted iff its rotated-BEV IoU (iou_bev of csrc/bev_iou.h, the NMS arithmetic) is
// exactly 0 with every scene box, with every accepted candidate of an earlier group, and with every other candidate
// of its own group -- two colliding candidates of one group are both dropped.  A candidate with a non-finite entry
// is rejected and blocks nobody; a scene box with a non-finite entry collides with nobody.
//
// One workgroup per sample, 256 threads = 64 candidates x 4 stripes: every thread tests its candidate against a
// quarter of the scene boxes and a quarter of the other candidates and keeps its own partial (a flag and a 64-bit
// row of the collision matrix) in LDS; the stripes are OR-ed, then one thread walks the groups.  No atomics, every
// output byte is written once by one thread, and OR does not depend on the order: the result is independent of the
// launch geometry.  The pair (i, j) is always evaluated as iou_bev(lower index, higher index), so the matrix is
// symmetric whatever the clipping order does in the last bit.
#include "ud_common.h"
#include "ud_prof.h"
#include "bev_iou.h"

namespace {

constexpr int kThreads = 256;
constexpr int kCand = 64;                 // candidate slots (UD_GT_PASTE_MAX_CAND = 63 are used)
constexpr int kStripes = kThreads / kCand;

__device__ __forceinline__ bool box_finite(const float* b) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 7; ++k) ok = ok && isfinite(b[k]);
  return ok;
}

__global__ __launch_bounds__(kThreads) void k_gt_paste_select(const float* __restrict__ gt,
                                                              const int64_t* __restrict__ gt_off,
                                                              const float* __restrict__ cand,
                                                              const int32_t* __restrict__ cand_group,
                                                              const int64_t* __restrict__ cand_off,
                                                              uint8_t* __restrict__ accept, int64_t accept_stride) {
  __shared__ float s_box[kCand][7];
  __shared__ int s_group[kCand];
  __shared__ int s_ok[kCand];                                   // finite
  __shared__ int s_hit[kStripes][kCand];                        // collides with a scene box
  __shared__ unsigned long long s_row[kStripes][kCand];         // collides with candidate j: bit j
  const int b = blockIdx.x;
  const int64_t c0 = cand_off[b];
  int64_t n64 = cand_off[b + 1] - c0;
  const int n = n64 < 0 ? 0 : (n64 > UD_GT_PASTE_MAX_CAND ? UD_GT_PASTE_MAX_CAND : (int)n64);   // host-checked
  const int64_t g0 = gt_off[b];
  const int64_t m = gt_off[b + 1] - g0;
  uint8_t* out = accept + (int64_t)b * accept_stride;
  if (n == 0) {                                                 // block-uniform
    for (int64_t i = threadIdx.x; i < accept_stride; i += kThreads) out[i] = 0;
    return;
  }
  const int c = threadIdx.x & (kCand - 1), stripe = threadIdx.x / kCand;
  if (stripe == 0) {
    bool ok = false;
    if (c < n) {
      const float* src = cand + (c0 + c) * 7;
#pragma unroll
      for (int k = 0; k < 7; ++k) s_box[c][k] = src[k];
      ok = box_finite(src);
      s_group[c] = cand_group[c0 + c];
    }
    s_ok[c] = ok ? 1 : 0;
  }
  __syncthreads();
  int hit = 0;
  unsigned long long row = 0;
  if (c < n && s_ok[c]) {
    float mine[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) mine[k] = s_box[c][k];
    for (int64_t j = stripe; j < m; j += kStripes) {
      float other[7];
      const float* src = gt + (g0 + j) * 7;
#pragma unroll
      for (int k = 0; k < 7; ++k) other[k] = src[k];
      if (box_finite(other) && ud_iou::iou_bev(mine, other) > 0.f) hit = 1;
    }
    for (int j = stripe; j < n; j += kStripes) {
      if (j == c || !s_ok[j]) continue;
      float other[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) other[k] = s_box[j][k];
      const float iou = c < j ? ud_iou::iou_bev(mine, other) : ud_iou::iou_bev(other, mine);
      if (iou > 0.f) row |= 1ull << j;
    }
  }
  s_hit[stripe][c] = hit;
  s_row[stripe][c] = row;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long accepted = 0;
    int i = 0;
    while (i < n) {
      int e = i + 1;
      while (e < n && s_group[e] == s_group[i]) ++e;
      const unsigned long long group = (e - i == 64 ? ~0ull : ((1ull << (e - i)) - 1)) << i;
      unsigned long long now = 0;
      for (int k = i; k < e; ++k) {
        int h = 0;
        unsigned long long r = 0;
#pragma unroll
        for (int s = 0; s < kStripes; ++s) {
          h |= s_hit[s][k];
          r |= s_row[s][k];
        }
        if (s_ok[k] && !h && !(r & (accepted | group))) now |= 1ull << k;   // bit k of r is never set
      }
      accepted |= now;
      i = e;
    }
    s_row[0][0] = accepted;
  }
  __syncthreads();
  const unsigned long long accepted = s_row[0][0];
  for (int64_t i = threadIdx.x; i < accept_stride; i += kThreads)
    out[i] = (i < n && ((accepted >> i) & 1ull)) ? 1 : 0;
}

}  // namespace

extern "C" int ud_gt_paste_select(const float* gt, const int64_t* gt_off_host, const int64_t* gt_off_dev,
                                  const float* cand, const int32_t* cand_group, const int64_t* cand_off_host,
                                  const int64_t* cand_off_dev, int B, uint8_t* accept, int64_t accept_stride,
                                  ud_stream_t stream_) {
  if (B < 0 || B > 65535 || accept_stride < 0) return UD_ERR_INVALID_ARG;
  if (B == 0) return UD_OK;
  if (!gt_off_host || !gt_off_dev || !cand_off_host || !cand_off_dev) return UD_ERR_INVALID_ARG;
  if (gt_off_host[0] < 0 || cand_off_host[0] < 0) return UD_ERR_INVALID_ARG;
  for (int b = 0; b < B; ++b) {
    const int64_t n = cand_off_host[b + 1] - cand_off_host[b];
    if (n < 0 || n > UD_GT_PASTE_MAX_CAND || n > accept_stride) return UD_ERR_INVALID_ARG;
    if (gt_off_host[b + 1] < gt_off_host[b]) return UD_ERR_INVALID_ARG;
  }
  if (gt_off_host[B] > gt_off_host[0] && !gt) return UD_ERR_INVALID_ARG;
  if (cand_off_host[B] > cand_off_host[0] && (!cand || !cand_group)) return UD_ERR_INVALID_ARG;
  if (accept_stride == 0) return UD_OK;
  if (!accept) return UD_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("input.k_gt_paste_select", stream);
  k_gt_paste_select<<<B, kThreads, 0, stream>>>(gt, gt_off_dev, cand, cand_group, cand_off_dev, accept, accept_stride);
  UD_LAUNCH_CHECK();
  return UD_OK;
}
