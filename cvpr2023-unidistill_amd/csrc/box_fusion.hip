// Box-level fusion (weighted box fusion) of the decoded boxes of S sources -- TTA views or models -- per sample
// (ops/box_fusion.py).  Three launches, no host synchronisation, no allocation, no floating-point atomics,
// bitwise reproducible.
//
// Inputs: the proposal layer's padded outputs, read in place: rois f32[S*B, R, box_dim], scores f32[S*B, R], labels
// i64[S*B, R], num i32[S*B]; source s of sample b is row s * B + b (view-major, as ops.tta.flip_views stacks them);
// box = (x, y, z, dx, dy, dz, yaw[, vx, vy]).  Per source a view (rot_deg, scale, flip_dx, flip_dy) and a weight w_s > 0.
//
// Un-view: every box goes back into the original frame under the inverse of A_v = F S R, in double from the fp32 inputs,
//   (x, y) = R^T F (x', y') / s, z = z' / s, dims = dims' / s, (vx, vy) = R^T F (vx', vy') / s, with the caller's sin / cos
//   (ops.tta._sincos: exact at multiples of 90 degrees); yaw takes no trigonometry: yaw' - rot (no flip), -yaw' - rot
//   (flip_dy), pi - yaw' - rot (flip_dx), pi + yaw' - rot (both), rot = rot_deg / 180 * pi.
// Validity: every entry and the score finite, score > score_threshold, label in [0, 65535]; other rows count nowhere.
// Order: per sample by (label ascending, score descending, source ascending, row ascending): a total order.
// Clusters: greedy NMS within one label on the un-viewed boxes rounded to fp32, iou_bev's fp32 arithmetic (earlier box
//   first), strict IoU > iou_threshold.  A box that no earlier kept box suppresses is an anchor; a suppressed box joins the
//   first anchor in order that suppresses it; suppressed boxes suppress nobody.  (Not the paper's running cluster matched
//   against the moving fused box: membership depends on the pairwise IoUs of the inputs alone.)
// Fusion: per cluster in double over the un-viewed (double) values, members in order, anchor first, c_i = w_s(i) * score_i:
//   centre, dims, velocity = sum c_i v_i / sum c_i; yaw = yaw_a + sum c_i d_i / sum c_i wrapped into [-pi, pi), d_i =
//   yaw_i - yaw_a wrapped to (-pi, pi], then folded by -+pi into [-pi/2, pi/2]; score = sum c_i / max(sum_i w_s(i),
//   sum_s w_s); rounded to fp32 once.
// Output: per sample the clusters by fused (fp32) score descending, ties by anchor order, at most max_out; zero padded.
//
//   k_bf_gather : one workgroup per sample: validity, ordered compaction, (label, score, position) keys, bitonic sort in
//                 LDS (lds_sort.h), then the un-viewed boxes written in sorted order.
//   k_bf_mask   : one thread per (box i, word of 64 later boxes): suppression bits of the same-label pairs only (nms_scan.h:
//                 ud_nms_mask_word with the labels) -- the order is label-major, so the mask is block-diagonal and words past
//                 the label's run cost one compare.
//   k_bf_fuse   : one workgroup per sample: wave 0 runs the one-wave NMS scan (nms_scan.h: ud_nms_scan, the scan of nms.hip)
//                 and records each box's anchor from the freshly removed bits; then one thread per anchor walks its mask row
//                 and accumulates its members; then the clusters are sorted by fused score in LDS and the first max_out are
//                 written.
#include "ud_common.h"
#include "ud_prof.h"
#include "lds_sort.h"
#include "nms_scan.h"
#include <cmath>

namespace {

constexpr int kMaxSources = 16;
constexpr int kMaxBoxes = ud_nms_scan_capacity(kNmsWordsPerLane);      // 16384 valid boxes per sample: the NMS scan's limit
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr double kPi = 3.14159265358979323846;
constexpr unsigned long long kPadKey = ~0ull;

struct Source {
  double sn, cs, scale, rot, w;
  int fx, fy;
};
struct Sources {
  Source s[kMaxSources];
};

__device__ __forceinline__ void unview(const Source& v, const float* in, int box_dim, double* u) {
  const double fx = v.fx ? -1.0 : 1.0, fy = v.fy ? -1.0 : 1.0;
  const double x = fx * (double)in[0], y = fy * (double)in[1];
  u[0] = (v.cs * x + v.sn * y) / v.scale;
  u[1] = (v.cs * y - v.sn * x) / v.scale;
  u[2] = (double)in[2] / v.scale;
  u[3] = (double)in[3] / v.scale;
  u[4] = (double)in[4] / v.scale;
  u[5] = (double)in[5] / v.scale;
  const double yaw = (double)in[6];
  u[6] = v.fx ? (v.fy ? kPi + yaw - v.rot : kPi - yaw - v.rot) : (v.fy ? -yaw - v.rot : yaw - v.rot);
  u[7] = u[8] = 0.0;
  if (box_dim == 9) {
    const double vx = fx * (double)in[7], vy = fy * (double)in[8];
    u[7] = (v.cs * vx + v.sn * vy) / v.scale;
    u[8] = (v.cs * vy - v.sn * vx) / v.scale;
  }
}

// slot[b][cap], order arrays [b][cap]: sorted position i of sample b is entry b * cap + i
__global__ __launch_bounds__(kThreads) void k_bf_gather(
    const float* __restrict__ rois, const float* __restrict__ scores, const long long* __restrict__ labels,
    const int* __restrict__ num, Sources src, int B, int S, int R, int box_dim, float score_thr, int cap, int npow2,
    int* __restrict__ slot, double* __restrict__ sboxd, float* __restrict__ sboxf, double* __restrict__ sconf,
    double* __restrict__ sweight, int* __restrict__ slabel, int* __restrict__ ssrc, int* __restrict__ nvalid) {
  extern __shared__ unsigned long long s_key[];
  __shared__ int s_wsum[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int total = S * R;
  int base = 0;
  for (int t0 = 0; t0 < total; t0 += kThreads) {
    const int t = t0 + tid;
    bool ok = false;
    float score = 0.f;
    long long label = 0;
    if (t < total) {
      const int s = t / R, r = t - s * R;
      const size_t row = (size_t)s * B + b;
      const int n = min(max(num[row], 0), R);
      if (r < n) {
        const float* p = rois + (row * R + r) * box_dim;
        score = scores[row * R + r];
        label = labels[row * R + r];
        ok = isfinite(score) && score > score_thr && label >= 0 && label <= 65535;
        for (int k = 0; k < box_dim; ++k) ok = ok && isfinite(p[k]);
      }
    }
    const UdBlockRank cr = ud_block_rank<kWaves>(ok, s_wsum);
    const int pos = base + cr.rank();
    if (ok && pos < cap) {
      s_key[pos] = ((unsigned long long)label << 48) | ((unsigned long long)ud_desc_bits(score + 0.0f) << 16) |
                   (unsigned long long)pos;
      slot[(size_t)b * cap + pos] = t;
    }
    base += cr.total;
    __syncthreads();                                   // s_wsum is read: the next trip may write it
  }
  // more valid boxes than the scan can hold (possible only when S * R > 16384): the sample is reported, not fused
  const bool overflow = base > kMaxBoxes;
  const int n = overflow ? 0 : base;
  if (tid == 0) nvalid[b] = overflow ? -1 : n;
  for (int i = tid; i < npow2; i += kThreads)
    if (i >= n) s_key[i] = kPadKey;
  __syncthreads();
  ud_bitonic_sort<kThreads>(s_key, npow2);
  for (int i = tid; i < n; i += kThreads) {
    const unsigned long long key = s_key[i];
    const size_t o = (size_t)b * cap + i;
    const int t = slot[(size_t)b * cap + (int)(key & 0xFFFFull)];
    const int s = t / R, r = t - s * R;
    const size_t row = (size_t)s * B + b;
    float in[9];
    for (int k = 0; k < box_dim; ++k) in[k] = rois[(row * R + r) * box_dim + k];
    double u[9];
    unview(src.s[s], in, box_dim, u);
#pragma unroll
    for (int k = 0; k < 9; ++k) sboxd[o * 9 + k] = u[k];
#pragma unroll
    for (int k = 0; k < 7; ++k) sboxf[o * 7 + k] = (float)u[k];
    sconf[o] = src.s[s].w * (double)scores[row * R + r];
    sweight[o] = src.s[s].w;
    slabel[o] = (int)(key >> 48);
    ssrc[o] = t;
  }
}

__global__ __launch_bounds__(256) void k_bf_mask(const float* __restrict__ sboxf, const int* __restrict__ slabel,
                                                 const int* __restrict__ nvalid, int cap, int words, float thresh,
                                                 unsigned long long* __restrict__ mask) {
  const int b = blockIdx.y;
  const int n = max(nvalid[b], 0), nwords = (n + 63) >> 6;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(t / words), wj = (int)(t - (long long)i * words);
  if (i >= n || wj >= nwords) return;
  // labels ascend: past the label's run nothing is suppressed
  mask[((size_t)b * cap + i) * words + wj] =
      ud_nms_mask_word<true>(sboxf + (size_t)b * cap * 7, 7, i, wj, n, thresh, slabel + (size_t)b * cap);
}

__global__ __launch_bounds__(kThreads) void k_bf_fuse(
    const unsigned long long* __restrict__ mask, const double* __restrict__ sboxd, const double* __restrict__ sconf,
    const double* __restrict__ sweight, const int* __restrict__ slabel, const int* __restrict__ ssrc,
    const int* __restrict__ nvalid, int cap, int words, int npow2, int box_dim, double wsum_all, int max_out,
    int* __restrict__ anchor, float* __restrict__ fbox, float* __restrict__ fscore, int* __restrict__ fcount,
    float* __restrict__ out_rois, float* __restrict__ out_scores, long long* __restrict__ out_labels,
    int* __restrict__ out_num, int* __restrict__ status, int* __restrict__ out_anchor, int* __restrict__ out_members) {
  extern __shared__ unsigned long long s_key[];
  __shared__ int s_count;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nv = nvalid[b], n = max(nv, 0), nwords = (n + 63) >> 6;
  const size_t o0 = (size_t)b * cap;
  mask += o0 * words;
  anchor += o0;
  if (tid < 64)                     // the NMS scan, recording for every box the anchor that took it (itself for a kept box)
    ud_nms_scan<kNmsWordsPerLane>(
        mask, n, nwords, words, n, [&](int i, int) { if (tid == 0) anchor[i] = i; },
        [&](int i, int wj, unsigned long long fresh) {
          while (fresh) {
            anchor[wj * 64 + __ffsll((long long)fresh) - 1] = i;
            fresh &= fresh - 1ull;
          }
        });
  if (tid == 0) s_count = 0;
  __syncthreads();
  for (int i = tid; i < npow2; i += kThreads) {
    unsigned long long key = kPadKey;
    if (i < n && anchor[i] == i) {
      const double* a = sboxd + (o0 + i) * 9;
      const double yaw_a = a[6];
      double csum = sconf[o0 + i], wsum = sweight[o0 + i], acc[9], dsum = 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[k] = csum * a[k];
      int members = 1;
      for (int wj = i >> 6; wj < nwords; ++wj) {
        unsigned long long bits = mask[(size_t)i * words + wj];
        while (bits) {
          const int j = wj * 64 + __ffsll((long long)bits) - 1;
          bits &= bits - 1ull;
          if (anchor[j] != i) continue;
          const double* m = sboxd + (o0 + j) * 9;
          const double c = sconf[o0 + j];
          csum += c;
          wsum += sweight[o0 + j];
#pragma unroll
          for (int k = 0; k < 9; ++k) acc[k] += c * m[k];
          double d = m[6] - yaw_a;
          d -= 2.0 * kPi * ceil((d - kPi) / (2.0 * kPi));         // (-pi, pi]
          if (d > 0.5 * kPi) d -= kPi;                            // a box and its half-turn: the same footprint
          else if (d < -0.5 * kPi) d += kPi;
          dsum += c * d;
          ++members;
        }
      }
      float* f = fbox + (o0 + i) * 9;
#pragma unroll
      for (int k = 0; k < 9; ++k) f[k] = (float)(acc[k] / csum);
      double yaw = yaw_a + dsum / csum;
      yaw -= 2.0 * kPi * floor((yaw + kPi) / (2.0 * kPi));        // [-pi, pi)
      f[6] = (float)yaw;
      const float sc = (float)(csum / fmax(wsum, wsum_all));
      fscore[o0 + i] = sc;
      fcount[o0 + i] = members;
      key = ((unsigned long long)ud_desc_bits(sc + 0.0f) << 32) | (unsigned long long)i;
    }
    s_key[i] = key;
  }
  __syncthreads();
  ud_bitonic_sort<kThreads>(s_key, npow2);
  for (int i = tid; i < npow2; i += kThreads)                     // clusters sort before the padding: their count
    if (s_key[i] != kPadKey && (i + 1 == npow2 || s_key[i + 1] == kPadKey)) s_count = i + 1;
  __syncthreads();
  const int count = min(s_count, max_out);
  for (int o = tid; o < max_out; o += kThreads) {
    const size_t q = (size_t)b * max_out + o;
    if (o < count) {
      const int i = (int)(s_key[o] & 0xFFFFFFFFull);
      for (int k = 0; k < box_dim; ++k) out_rois[q * box_dim + k] = fbox[(o0 + i) * 9 + k];
      out_scores[q] = fscore[o0 + i];
      out_labels[q] = slabel[o0 + i];
      if (out_anchor) out_anchor[q] = ssrc[o0 + i];
      if (out_members) out_members[q] = fcount[o0 + i];
    } else {
      for (int k = 0; k < box_dim; ++k) out_rois[q * box_dim + k] = 0.f;
      out_scores[q] = 0.f;
      out_labels[q] = 0;
      if (out_anchor) out_anchor[q] = -1;
      if (out_members) out_members[q] = 0;
    }
  }
  if (tid == 0) {
    out_num[b] = count;
    status[b] = nv < 0 ? 1 : 0;
  }
}

struct Plan {
  int cap, words, npow2;
  size_t lds;
};

bool make_plan(int B, int S, int R, Plan* p) {
  if (B < 1 || B > 65535 || S < 1 || S > kMaxSources || R < 1 || (long long)S * R > (1ll << 24)) return false;
  p->cap = std::min(S * R, kMaxBoxes);
  p->words = (p->cap + 63) / 64;
  p->npow2 = 2;
  while (p->npow2 < p->cap) p->npow2 <<= 1;
  p->lds = (size_t)p->npow2 * sizeof(unsigned long long);
  return true;
}

struct Buffers {
  int *slot, *slabel, *ssrc, *nvalid, *anchor, *fcount;
  double *sboxd, *sconf, *sweight;
  float *sboxf, *fbox, *fscore;
  unsigned long long* mask;
};

size_t carve(UdArena& a, int B, const Plan& p, Buffers* w) {
  const size_t n = (size_t)B * p.cap;
  w->mask = a.take<unsigned long long>(n * p.words);
  w->sboxd = a.take<double>(n * 9);
  w->sconf = a.take<double>(n);
  w->sweight = a.take<double>(n);
  w->sboxf = a.take<float>(n * 7);
  w->fbox = a.take<float>(n * 9);
  w->fscore = a.take<float>(n);
  w->slot = a.take<int>(n);
  w->slabel = a.take<int>(n);
  w->ssrc = a.take<int>(n);
  w->anchor = a.take<int>(n);
  w->fcount = a.take<int>(n);
  w->nvalid = a.take<int>(B);
  return a.used;
}

}  // namespace

extern "C" {

size_t ud_box_fusion_workspace_bytes(int B, int S, int R) {
  Plan p;
  if (!make_plan(B, S, R, &p)) return 0;
  UdArena a(nullptr, 0);
  Buffers w;
  return carve(a, B, p, &w);
}

int ud_box_fusion(const float* rois, const float* scores, const long long* labels, const int* num, int B, int S, int R,
                  int box_dim, const double* views, const double* weights, float iou_threshold, float score_threshold,
                  int max_out, float* out_rois, float* out_scores, long long* out_labels, int* out_num, int* status,
                  int* out_anchor, int* out_members, void* workspace, size_t workspace_bytes, ud_stream_t stream_) {
  Plan p;
  if (!make_plan(B, S, R, &p)) return UD_ERR_INVALID_ARG;
  if (box_dim != 7 && box_dim != 9) return UD_ERR_INVALID_ARG;
  if (max_out < 1 || (long long)B * max_out * box_dim > 0x7FFFFFFFll) return UD_ERR_INVALID_ARG;
  if (!std::isfinite(iou_threshold) || std::isnan(score_threshold)) return UD_ERR_INVALID_ARG;
  if (!rois || !scores || !labels || !num || !views || !weights) return UD_ERR_INVALID_ARG;
  if (!out_rois || !out_scores || !out_labels || !out_num || !status) return UD_ERR_INVALID_ARG;
  Sources src;
  double wsum_all = 0.0;
  for (int s = 0; s < S; ++s) {
    const double* v = views + s * 6;                    // rot_deg, scale, flip_dx, flip_dy, sin, cos
    for (int i = 0; i < 6; ++i)
      if (!std::isfinite(v[i])) return UD_ERR_INVALID_ARG;
    if (!(v[1] > 0.0) || std::fabs(v[4] * v[4] + v[5] * v[5] - 1.0) > 1e-12) return UD_ERR_INVALID_ARG;
    if (!std::isfinite(weights[s]) || !(weights[s] > 0.0)) return UD_ERR_INVALID_ARG;
    Source& o = src.s[s];
    o.rot = v[0] / 180 * kPi;
    o.scale = v[1];
    o.fx = v[2] != 0.0;
    o.fy = v[3] != 0.0;
    o.sn = v[4];
    o.cs = v[5];
    o.w = weights[s];
    wsum_all += weights[s];
  }
  for (int s = S; s < kMaxSources; ++s) src.s[s] = src.s[0];
  UdArena arena(workspace, workspace_bytes);
  Buffers w;
  carve(arena, B, p, &w);
  if (!arena.ok()) return UD_ERR_WORKSPACE;
  static UdDeviceOnce once;
  if (const int e = ud_allow_dyn_lds(once, kMaxBoxes * (int)sizeof(unsigned long long), k_bf_gather, k_bf_fuse)) return e;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("box_fusion", stream);
  k_bf_gather<<<B, kThreads, p.lds, stream>>>(rois, scores, labels, num, src, B, S, R, box_dim, score_threshold, p.cap,
                                              p.npow2, w.slot, w.sboxd, w.sboxf, w.sconf, w.sweight, w.slabel, w.ssrc,
                                              w.nvalid);
  UD_LAUNCH_CHECK();
  k_bf_mask<<<dim3(ud_div_up((long long)p.cap * p.words, 256), B), 256, 0, stream>>>(w.sboxf, w.slabel, w.nvalid, p.cap,
                                                                                     p.words, iou_threshold, w.mask);
  UD_LAUNCH_CHECK();
  k_bf_fuse<<<B, kThreads, p.lds, stream>>>(w.mask, w.sboxd, w.sconf, w.sweight, w.slabel, w.ssrc, w.nvalid, p.cap, p.words,
                                            p.npow2, box_dim, wsum_all, max_out, w.anchor, w.fbox, w.fscore, w.fcount,
                                            out_rois, out_scores, out_labels, out_num, status, out_anchor, out_members);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

}  // extern "C"
