// Stable LSD radix sort of (key, index) pairs on the device, integer counting only (no library primitive).
// Used by spconv_order.hip (rulebook row order) and nus_eval.hip (global score order per class).
#pragma once
#include "ud_common.h"
#include <algorithm>

namespace {

// ---- stable LSD radix sort of (key, row) pairs: digits of at most 9 bits, chunks of 2 048 keys ------------------------------
// Key type K: unsigned (spconv row masks) or unsigned long long (wider keys, nus_eval.hip); digits are taken from K, counted in 32 bits.
constexpr int kRsChunk = 2048, kRsBinsMax = 512, kRsWave = kRsChunk / 4;      // a wave owns 512 consecutive keys of its chunk

// hist[digit * nblk + chunk] = number of keys of the chunk with that digit
template <typename K>
__global__ __launch_bounds__(256) void k_rs_hist(const K* __restrict__ keys, int M, int shift, int bins, int nblk,
                                                 unsigned* __restrict__ hist) {
  __shared__ unsigned s_h[kRsBinsMax];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < bins; i += 256) s_h[i] = 0u;
  __syncthreads();
  const unsigned dm = (unsigned)bins - 1u;
#pragma unroll
  for (int r = 0; r < kRsChunk / 256; ++r) {
    const int i = b * kRsChunk + r * 256 + tid;
    if (i < M) atomicAdd(&s_h[(unsigned)(keys[i] >> shift) & dm], 1u);
  }
  __syncthreads();
  for (int i = tid; i < bins; i += 256) hist[(size_t)i * nblk + b] = s_h[i];
}

// hist[digit][0 .. nblk) -> its exclusive scan in place + dtot[digit] = the row's total: ONE WAVE per digit row, 64 chunks per trip.
// (First version: one workgroup scanning all bins * nblk counters, 97 uncoalesced counters per thread: 108 us per pass at 394 k
// rows -- 2.4 ms per encoder pass, more than the library sort it replaced.)
__global__ __launch_bounds__(256) void k_rs_rowscan(unsigned* __restrict__ hist, int bins, int nblk, unsigned* __restrict__ dtot) {
  const int lane = threadIdx.x & 63, d = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= bins) return;
  unsigned* row = hist + (size_t)d * nblk;
  unsigned carry = 0u;
  for (int b0 = 0; b0 < nblk; b0 += 64) {
    const int b = b0 + lane;
    const unsigned v = b < nblk ? row[b] : 0u;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned a = __shfl_up(inc, o);
      if (lane >= o) inc += a;
    }
    if (b < nblk) row[b] = carry + inc - v;
    carry += __shfl(inc, 63);
  }
  if (lane == 0) dtot[d] = carry;
}

// keys_out / vals_out[destination] = the pair, destinations in (digit, chunk, position inside the chunk) order: stable.
// vals_in == nullptr: the value of key i is i (first pass); keys_out == nullptr: only the values are needed (last pass).
template <typename K>
__global__ __launch_bounds__(256) void k_rs_scatter(const K* __restrict__ keys_in, const int32_t* __restrict__ vals_in, int M,
                                                    int shift, int bins, int nblk, const unsigned* __restrict__ hist,
                                                    const unsigned* __restrict__ dtot, K* __restrict__ keys_out,
                                                    int32_t* __restrict__ vals_out) {
  __shared__ unsigned s_run[4][kRsBinsMax];          // per wave: its keys per digit, then the running destination per digit
  __shared__ unsigned s_dpre[kRsBinsMax];            // where digit d's group starts = exclusive scan of the digit totals
  __shared__ unsigned s_wsum[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned dm = (unsigned)bins - 1u;
  for (int i = tid; i < 4 * bins; i += 256) s_run[i / bins][i % bins] = 0u;
  {   // exclusive scan of the <= 512 digit totals: two consecutive digits per thread
    const int d0 = 2 * tid;
    const unsigned t0 = d0 < bins ? dtot[d0] : 0u, t1 = d0 + 1 < bins ? dtot[d0 + 1] : 0u;
    unsigned inc = t0 + t1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned a = __shfl_up(inc, o);
      if (lane >= o) inc += a;
    }
    if (lane == 63) s_wsum[wv] = inc;
    __syncthreads();
    unsigned off = inc - (t0 + t1);
    for (int w = 0; w < wv; ++w) off += s_wsum[w];
    if (d0 < bins) s_dpre[d0] = off;
    if (d0 + 1 < bins) s_dpre[d0 + 1] = off + t0;
  }
  __syncthreads();
  const int w0 = b * kRsChunk + wv * kRsWave;
  K key[kRsWave / 64];
#pragma unroll
  for (int r = 0; r < kRsWave / 64; ++r) {
    const int i = w0 + r * 64 + lane;
    key[r] = i < M ? keys_in[i] : K(0);
    if (i < M) atomicAdd(&s_run[wv][(unsigned)(key[r] >> shift) & dm], 1u);
  }
  __syncthreads();
  for (int d = tid; d < bins; d += 256) {            // wave bases of digit d: the chunk's group start + the earlier waves' keys
    unsigned base = s_dpre[d] + hist[(size_t)d * nblk + b];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const unsigned c = s_run[w][d];
      s_run[w][d] = base;
      base += c;
    }
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < kRsWave / 64; ++r) {
    const int i = w0 + r * 64 + lane;
    const bool ok = i < M;
    const unsigned d = (unsigned)(key[r] >> shift) & dm;
    unsigned long long peers = __ballot(ok);          // lanes of this round with my digit
    for (int bit = 0; (1 << bit) < bins; ++bit) {
      const unsigned long long bal = __ballot((d >> bit) & 1u);
      peers &= ((d >> bit) & 1u) ? bal : ~bal;
    }
    unsigned pos = 0u;
    if (ok) pos = s_run[wv][d] + (unsigned)__popcll(peers & below);
    __builtin_amdgcn_wave_barrier();                  // every lane has read the counter before the group's first lane moves it
    if (ok && (peers & below) == 0ull) s_run[wv][d] += (unsigned)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);               // lgkmcnt(0): the update has landed before the next round reads it
    if (ok) {
      if (keys_out) keys_out[pos] = key[r];
      vals_out[pos] = vals_in ? vals_in[i] : i;
    }
  }
}

// order[] = 0 .. M-1 sorted (stably) by the low `bits` bits of keys[]: ceil(bits / 9) passes of hist -> rowscan -> scatter.
// Scratch: ktmp[2] / vtmp[2] of M entries, hist of kRsBinsMax * nblk counters (nblk = ceil(M / kRsChunk)), dtot of kRsBinsMax.
template <typename K>
int rs_sort_pairs(const K* keys, int M, int bits, int32_t* order, K* const ktmp[2], int32_t* const vtmp[2], unsigned* hist,
                  unsigned* dtot, hipStream_t stream) {
  const int nblk = ud_div_up(M, kRsChunk);
  const int passes = std::max(1, ud_div_up(bits, 9)), db = ud_div_up(std::max(bits, 1), passes);
  const K* kin = keys;
  const int32_t* vin = nullptr;
  for (int p = 0; p < passes; ++p) {
    const int shift = p * db, bins = 1 << std::min(db, bits - shift > 0 ? bits - shift : 1);
    const bool last = p + 1 == passes;
    K* kout = last ? nullptr : ktmp[p & 1];
    int32_t* vout = last ? order : vtmp[p & 1];
    k_rs_hist<K><<<nblk, 256, 0, stream>>>(kin, M, shift, bins, nblk, hist);
    UD_LAUNCH_CHECK();
    k_rs_rowscan<<<ud_div_up(bins, 4), 256, 0, stream>>>(hist, bins, nblk, dtot);
    UD_LAUNCH_CHECK();
    k_rs_scatter<K><<<nblk, 256, 0, stream>>>(kin, vin, M, shift, bins, nblk, hist, dtot, kout, vout);
    UD_LAUNCH_CHECK();
    kin = kout, vin = vout;
  }
  return UD_OK;
}

}  // namespace
