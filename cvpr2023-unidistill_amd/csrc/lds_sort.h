// Ordering inside one workgroup, stated once for the post-processing stages (proposals.hip, box_fusion.hip, track.hip,
// track_interp.hip, track_metric.hip, nus_eval.hip): order keys, the whole-workgroup bitonic sort in LDS, and the ordered
// compaction.  Every includer gets its own copy (anonymous namespace); the workgroup's width is a template argument.
#pragma once
#include "ud_common.h"

namespace {

// Bits that ascend (unsigned) as the value descends.  -0 sorts after +0: a caller that wants them equal adds 0 first.
__device__ __forceinline__ unsigned ud_desc_bits(float v) {
  const unsigned u = __float_as_uint(v);
  return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}
__device__ __forceinline__ unsigned long long ud_desc_bits(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return ~((u >> 63) ? ~u : (u | 0x8000000000000000ull));
}

// The bitonic network over n (a power of two) LDS elements, run by all kThreads threads of the workgroup: one barrier per
// stage.  swap_if(i, p, up) orders elements i < p: the smaller first if up, the larger first otherwise (equal elements may
// change places: they are indistinguishable).
template <int kThreads, bool kDescending, class SwapIf>
__device__ __forceinline__ void ud_bitonic_network(int n, SwapIf swap_if) {
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += kThreads) {
        const int p = i ^ j;
        if (p > i) swap_if(i, p, ((i & k) == 0) != kDescending);
      }
      __syncthreads();
    }
}

// Sort of n (a power of two) 64-bit keys in LDS.  The caller's barrier stands between its writes of key[] and the call; the
// last stage's barrier stands behind the result.
template <int kThreads, bool kDescending = false>
__device__ __forceinline__ void ud_bitonic_sort(unsigned long long* key, int n) {
  ud_bitonic_network<kThreads, kDescending>(n, [&](int i, int p, bool up) {
    const unsigned long long a = key[i], c = key[p];
    if ((a > c) == up) { key[i] = c; key[p] = a; }
  });
}

// The same for (key, value) pairs, ordered by key, then by value.
template <int kThreads, bool kDescending = false>
__device__ __forceinline__ void ud_bitonic_sort(unsigned long long* key, int* val, int n) {
  ud_bitonic_network<kThreads, kDescending>(n, [&](int i, int p, bool up) {
    const unsigned long long a = key[i], c = key[p];
    const int va = val[i], vc = val[p];
    const bool gt = a > c || (a == c && va > vc);
    if (gt == up) { key[i] = c; key[p] = a; val[i] = vc; val[p] = va; }
  });
}

// Ordered compaction across a workgroup of kWaves waves: rank() is the number of set flags in the threads before this
// one (formed where it is asked for: a thread whose flag is clear need not), total the number in the whole workgroup.
// ONE barrier, between the writes and the reads of s_wsum[kWaves]; the caller puts a barrier before the scratch array's
// next use.
struct UdBlockRank {
  unsigned long long ballot;     // this wave's flags
  int before, total;             // set flags in the waves before this one, and in all waves
  __device__ __forceinline__ int rank() const { return before + __popcll(ballot & ((1ull << ud_lane()) - 1ull)); }
};
template <int kWaves>
__device__ __forceinline__ UdBlockRank ud_block_rank(bool flag, int* s_wsum) {
  const int wave = threadIdx.x / UD_WAVE;
  UdBlockRank r = {__ballot(flag), 0, 0};
  if (ud_lane() == 0) s_wsum[wave] = __popcll(r.ballot);
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int c = s_wsum[w];
    r.before += w < wave ? c : 0;
    r.total += c;
  }
  return r;
}

}  // namespace
