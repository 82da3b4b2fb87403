// Greedy rotated-BEV NMS over boxes already in suppression order, stated once for nms.hip, proposals.hip and box_fusion.hip:
// the suppression bits of one (box, word of 64 later boxes), and the one-wave scan of the finished mask.  The kernels keep
// their own grids, bounds and stores.  __forceinline__ with compile-time callbacks: every includer gets its own copy
// (anonymous namespace) and pays for nothing it does not use.
#pragma once
#include "ud_common.h"
#include "bev_iou.h"

namespace {

// Boxes one scan can walk: lane w of the wave owns words w, w + 64, ... of the running "removed" bitmap.
constexpr int ud_nms_scan_capacity(int words_per_lane) { return 64 * UD_WAVE * words_per_lane; }
constexpr int kNmsWordsPerLane = 4;          // nms.hip and box_fusion.hip: 16384 boxes

// Word wj of box i's mask row: bit (j - 64 * wj) is set for every j in [max(i + 1, 64 * wj), min(n, 64 * wj + 64)) with
// iou_bev(box i, box j) > thresh, box i first.  A box is the first 7 floats of a row of `stride` floats.  With
// kLabelRuns, lab[] holds the boxes' labels, ascending in box order: the loop ends at the first j of another label than
// box i's, and a word that begins past i's label run costs one compare.  (A template argument, not a null test: the
// kernel's pointer is a run-time value.)
template <bool kLabelRuns = false>
__device__ __forceinline__ unsigned long long ud_nms_mask_word(const float* __restrict__ boxes, int stride, int i, int wj,
                                                               int n, float thresh, const int* __restrict__ lab = nullptr) {
  const int j0 = wj * 64, jbeg = max(j0, i + 1), jend = min(j0 + 64, n);
  if (jbeg >= jend) return 0ull;
  const int li = kLabelRuns ? lab[i] : 0;
  if (kLabelRuns && lab[jbeg] != li) return 0ull;
  float bi[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) bi[k] = boxes[(size_t)i * stride + k];
  unsigned long long bits = 0ull;
  for (int j = jbeg; j < jend; ++j) {
    if (kLabelRuns && lab[j] != li) break;
    float bj[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) bj[k] = boxes[(size_t)j * stride + k];
    if (ud_iou::iou_bev(bi, bj) > thresh) bits |= 1ull << (j - j0);
  }
  return bits;
}

// ONE wave walks boxes 0 .. n - 1 in order (the inherently sequential part): box i is kept unless an earlier kept box
// has its bit set; a kept box ORs words [0, words) of its mask row (rows `row_words` apart) into `removed`.  The walk ends
// after `limit` kept boxes; the count of kept boxes is returned to every lane.  words <= 64 * kWordsPerLane.
//   on_keep(i, count)      : every lane, per kept box, count = kept boxes before it
//   on_fresh(i, wj, fresh) : the lane that owns word wj, per kept box: the bits of that word that box i removes first
template <int kWordsPerLane, class OnKeep, class OnFresh>
__device__ __forceinline__ int ud_nms_scan(const unsigned long long* __restrict__ mask, int n, int words, int row_words,
                                           int limit, OnKeep on_keep, OnFresh on_fresh) {
  const int lane = ud_lane();
  unsigned long long removed[kWordsPerLane] = {};
  int count = 0;
  for (int i = 0; i < n && count < limit; ++i) {
    const int w = i >> 6, owner = w & 63, slot = w >> 6;
    unsigned long long word = removed[0];
#pragma unroll
    for (int s = 1; s < kWordsPerLane; ++s)
      if (s == slot) word = removed[s];
    const unsigned lo = __shfl((unsigned)(word & 0xFFFFFFFFull), owner);
    const unsigned hi = __shfl((unsigned)(word >> 32), owner);
    const unsigned long long cur = ((unsigned long long)hi << 32) | lo;
    if (!((cur >> (i & 63)) & 1ull)) {              // wave-uniform
      on_keep(i, count);
      ++count;
#pragma unroll
      for (int s = 0; s < kWordsPerLane; ++s) {
        const int wj = lane + 64 * s;
        if (wj < words) {
          const unsigned long long row = mask[(size_t)i * row_words + wj];
          on_fresh(i, wj, row & ~removed[s]);
          removed[s] |= row;
        }
      }
    }
  }
  return count;
}

}  // namespace
