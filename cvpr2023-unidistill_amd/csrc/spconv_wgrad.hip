// Sparse 3-D convolution weight gradients for MI355X / gfx950 (see spconv_conv.hip for the forward / dgrad kernels and the
// rulebook layout): fp32 (exact-f32 MFMA) and bf16-operand kernels over (kernel offset, row chunk) workgroups, reduced over
// the chunks in a fixed order -- no fp atomics, the result is deterministic.
#include "ud_common.h"
#include "ud_prof.h"
#include "spconv_tile.h"

namespace {

// ---- weight gradient ------------------------------------------------------------------------
// partial[g][k][n][c] = sum over the rows o of chunk g of gout[o][n] * in[nbr[o][k]][c]
template <int CIN_P, int COUT_P>
__global__ __launch_bounds__(256) void k_wgrad_mfma(const float* __restrict__ in, int cin,
                                                    const int32_t* __restrict__ nbr, int K,
                                                    const float* __restrict__ gout, int cout,
                                                    float* __restrict__ partial, int Mout,
                                                    int rows_per_chunk) {
  constexpr int LDO = kTM + 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Gs = reinterpret_cast<float*>(smem);  // [COUT_P][LDO]   gout tile, transposed
  float* Is = Gs + COUT_P * LDO;                // [CIN_P][LDO]    gathered input tile, transposed
  int* s_nbr = reinterpret_cast<int*>(Is + CIN_P * LDO);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int k = blockIdx.x;
  const int chunk = blockIdx.y;
  constexpr int NTILES = (COUT_P / 16) * (CIN_P / 16);
  constexpr int TPW = (NTILES + 3) / 4;  // tiles per wave
  f32x4 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int r_begin = chunk * rows_per_chunk;
  const int r_end = min(r_begin + rows_per_chunk, Mout);
  for (int row0 = r_begin; row0 < r_end; row0 += kTM) {
    int r = -1;
    if (tid < kTM && row0 + tid < r_end) r = nbr[(size_t)(row0 + tid) * K + k];
    if (tid < kTM) s_nbr[tid] = r;
    if (!__syncthreads_or(r >= 0)) continue;
    // gout tile transposed: Gs[n][o]; rows whose neighbour is missing contribute zero anyway
    // because the matching Is column is zero.
    for (int idx = tid; idx < kTM * COUT_P; idx += 256) {
      const int o = idx / COUT_P, n = idx - o * COUT_P;
      const int row = row0 + o;
      Gs[n * LDO + o] = (row < r_end && n < cout) ? gout[(size_t)row * cout + n] : 0.f;
    }
    for (int idx = tid; idx < kTM * CIN_P; idx += 256) {
      const int o = idx / CIN_P, c = idx - o * CIN_P;
      const int rr = s_nbr[o];
      Is[c * LDO + o] = (rr >= 0 && c < cin) ? in[(size_t)rr * cin + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int tile = wave + 4 * t;
      if (tile < NTILES) {
        const int nt = tile / (CIN_P / 16), ct = tile - nt * (CIN_P / 16);
        const float* ga = Gs + (nt * 16 + li) * LDO + 4 * g;
        const float* ib = Is + (ct * 16 + li) * LDO + 4 * g;
#pragma unroll
        for (int ob = 0; ob < kTM / 16; ++ob) {
          const float4 a = *reinterpret_cast<const float4*>(ga + ob * 16);
          const float4 b = *reinterpret_cast<const float4*>(ib + ob * 16);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  float* p = partial + ((size_t)chunk * K + k) * COUT_P * CIN_P;
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tile = wave + 4 * t;
    if (tile < NTILES) {
      const int nt = tile / (CIN_P / 16), ct = tile - nt * (CIN_P / 16);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        p[(size_t)(nt * 16 + 4 * g + r) * CIN_P + ct * 16 + li] = acc[t][r];
    }
  }
}

// ---- weight gradient, fp32, row-major staging ------------------------------------------------------------------------
// k_wgrad_mfma above transposes both tiles into LDS element by element (one div / mod, one scalar load and one 8-way
// bank-conflicted ds_write_b32 per element, 64 per thread and tile) and gives every wave single 16 x 16 tiles with no
// fragment reuse: 4.2 ms per 128-channel layer of the LiDAR detector's fp32 step (198 k rows: 42 TFLOP/s; this kernel:
// 2.03 ms = 86 TFLOP/s = 55 % of the fp32 matrix peak).  Here the 64 gout rows and
// the 64 gathered input rows are copied as they lie in memory (16-byte loads and ds_write_b128, rows padded to a stride of
// 16 mod 32 banks) and the fp32 MFMA's operands are read straight out of the row-major tiles: lane (g, li) of
// v_mfma_f32_16x16x4_f32 wants A[i = li][k = g] = gout[row 4s + g][n0 + li] -- 16 consecutive floats of each of two rows per
// half wave, conflict-free at that stride.  Waves form a WN x WC grid over the Cout x Cin tile and reuse their fragments
// ((TN + TC) reads per TN x TC MFMAs).  Same decomposition (offset k, row chunk) and fixed-order chunk reduction as above.
template <int P>
struct WgLd { static constexpr int v = (P % 32 == 0) ? P + 16 : P + 32; };

template <int CIN_P, int COUT_P>
__global__ __launch_bounds__(256) void k_wgrad_rows(const float* __restrict__ in, int cin,
                                                    const int32_t* __restrict__ nbr, int K,
                                                    const float* __restrict__ gout, int cout,
                                                    float* __restrict__ partial, int Mout,
                                                    int rows_per_chunk) {
  constexpr int LDG = WgLd<COUT_P>::v, LDI = WgLd<CIN_P>::v;
  constexpr int NT = COUT_P / 16, CT = CIN_P / 16;
  constexpr int WN = NT >= 2 ? 2 : 1, WC = (4 / WN) < CT ? (4 / WN) : CT;   // wave grid (idle waves on the tiny layers)
  constexpr int TN = NT / WN, TC = CT / WC;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Gs = reinterpret_cast<float*>(smem);  // [kTM][LDG]  gout rows
  float* Is = Gs + kTM * LDG;                   // [kTM][LDI]  gathered input rows (zero where the neighbour is missing)
  int* s_nbr = reinterpret_cast<int*>(Is + kTM * LDI);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int k = blockIdx.x, chunk = blockIdx.y;
  const bool active_wave = wave < WN * WC;
  const int wn = wave / WC, wc = wave % WC;
  f32x4 acc[TN][TC];
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int b = 0; b < TC; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int r_begin = chunk * rows_per_chunk;
  const int r_end = min(r_begin + rows_per_chunk, Mout);
  for (int row0 = r_begin; row0 < r_end; row0 += kTM) {
    int r = -1;
    if (tid < kTM && row0 + tid < r_end) r = nbr[(size_t)(row0 + tid) * K + k];
    if (tid < kTM) s_nbr[tid] = r;
    if (!__syncthreads_or(r >= 0)) continue;
    for (int u = tid; u < kTM * (COUT_P / 4); u += 256) {
      const int o = u / (COUT_P / 4), n4 = (u - o * (COUT_P / 4)) * 4;
      const int row = row0 + o;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < r_end && n4 < cout) v = *reinterpret_cast<const float4*>(gout + (size_t)row * cout + n4);
      *reinterpret_cast<float4*>(Gs + o * LDG + n4) = v;
    }
    for (int u = tid; u < kTM * (CIN_P / 4); u += 256) {
      const int o = u / (CIN_P / 4), c4 = (u - o * (CIN_P / 4)) * 4;
      const int rr = s_nbr[o];
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rr >= 0 && c4 < cin) v = *reinterpret_cast<const float4*>(in + (size_t)rr * cin + c4);
      *reinterpret_cast<float4*>(Is + o * LDI + c4) = v;
    }
    __syncthreads();
    if (active_wave) {
      const float* ga = Gs + g * LDG + wn * TN * 16 + li;
      const float* ib = Is + g * LDI + wc * TC * 16 + li;
#pragma unroll 4
      for (int s4 = 0; s4 < kTM / 4; ++s4) {      // four rows per MFMA
        float a[TN], b[TC];
#pragma unroll
        for (int t = 0; t < TN; ++t) a[t] = ga[s4 * 4 * LDG + t * 16];
#pragma unroll
        for (int t = 0; t < TC; ++t) b[t] = ib[s4 * 4 * LDI + t * 16];
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
          for (int tc = 0; tc < TC; ++tc)
            acc[tn][tc] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tn], b[tc], acc[tn][tc], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (!active_wave) return;
  float* p = partial + ((size_t)chunk * K + k) * COUT_P * CIN_P;
#pragma unroll
  for (int tn = 0; tn < TN; ++tn)
#pragma unroll
    for (int tc = 0; tc < TC; ++tc)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        p[(size_t)((wn * TN + tn) * 16 + 4 * g + r) * CIN_P + (wc * TC + tc) * 16 + li] = acc[tn][tc][r];
}

// ---- weight gradient, bf16 operands (mixed-precision training) --------------------------------------
// Same decomposition (one workgroup per (offset k, row chunk g), ordered reduction of the chunks), but
// the products run on v_mfma_f32_16x16x32_bf16 -- 16x the rate of the fp32 matrix instruction the exact
// path uses.  The reduction index of this GEMM is the sparse ROW, i.e. both operands (gout[row][n] and
// the gathered in[nbr[row][k]][c]) are K-strided in memory: tiles of 64 rows are staged row-major as
// bf16 and the fragments are read with ds_read_b64_tr_b16 (see csrc/conv2d.hip: inside a 16-lane group
// lane j points at [row k0 + (j>>2)][channel 4*(j&3)..+3] and lane i receives [k0..k0+3][channel i]).
// Row tiles follow the mask-sorted row order of the forward kernel; a per-tile 27-bit activity mask
// (k_tile_masks) lets a workgroup skip the tiles that have no pair for its offset.
typedef short v4s_t __attribute__((ext_vector_type(4)));
constexpr int kWR = 64;                              // rows per step

__global__ __launch_bounds__(256) void k_tile_masks(const int32_t* __restrict__ nbr, int K,
                                                    const int32_t* __restrict__ order, int Mout,
                                                    unsigned* __restrict__ masks, int ntiles) {
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (tile >= ntiles) return;
  const int p = tile * kWR + lane;
  unsigned m = 0u;
  if (p < Mout) {
    const int row = order ? order[p] : p;
    for (int k = 0; k < K; ++k)
      if (nbr[(size_t)row * K + k] >= 0) m |= 1u << k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m |= __shfl_xor((int)m, o);
  if (lane == 0) masks[tile] = m;
}

__device__ __forceinline__ v4s_t tr_issue(unsigned lds_byte_addr) {
  v4s_t r;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(lds_byte_addr));
  return r;
}
__device__ __forceinline__ bf16x8 cat8(v4s_t lo, v4s_t hi) {
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
__device__ __forceinline__ bf16x8 tr_frag8(const unsigned short* lo_p, const unsigned short* hi_p) {
  const v4s_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)lo_p);
  const v4s_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)hi_p);
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// Compact the ids of this workgroup's tiles that have a pair for offset k into LDS (one wave, ordered).
// Scanning the tile masks in global memory one dependent load at a time cost more than the MFMAs.
constexpr int kMaxTilesPerChunk = 2048;
__device__ __forceinline__ int build_active_list(const unsigned* __restrict__ masks, int k, int t_begin,
                                                 int t_end, short* list) {
  __shared__ int s_count;
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    int count = 0;
    for (int base = t_begin; base < t_end; base += 64) {
      const int t = base + lane;
      const bool on = t < t_end && ((masks[t] >> k) & 1u);
      const unsigned long long b = __ballot(on);
      if (on) list[count + __popcll(b & ((1ull << lane) - 1ull))] = (short)(t - t_begin);
      count += __popcll(b);
    }
    if (lane == 0) s_count = count;
  }
  __syncthreads();
  return s_count;
}

template <int CIN_P, int COUT_P, bool BF_IO>   // BF_IO: `in` and `gout` already hold bf16 (cin, cout % 8 == 0)
__global__ __launch_bounds__(256) void k_wgrad_bf16(const float* __restrict__ in, int cin,
                                                    const int32_t* __restrict__ nbr, int K,
                                                    const float* __restrict__ gout, int cout,
                                                    float* __restrict__ partial, int Mout,
                                                    const int32_t* __restrict__ order,
                                                    const unsigned* __restrict__ masks, int ntiles,
                                                    int tiles_per_chunk) {
  constexpr int LDN = COUT_P + 16, LDC = CIN_P + 16;          // bf16 elements per LDS row
  constexpr int NT = COUT_P / 16, CTT = CIN_P / 16;
  constexpr int WM = NT >= 2 ? 2 : 1, WN = 4 / WM;
  constexpr int TI = NT / WM, TJ = (CTT / WN) > 0 ? (CTT / WN) : 1;
  constexpr int NU = (kWR * (COUT_P / 4) + 255) / 256;        // float4 units per thread
  constexpr int CU = (kWR * (CIN_P / 4) + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned short* Ns = reinterpret_cast<unsigned short*>(smem);      // [2][kWR][LDN]
  unsigned short* Cs = Ns + 2 * kWR * LDN;                             // [2][kWR][LDC]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int wm = wave / WN, wn = wave % WN;
  const bool wave_on = wn * TJ < CTT;
  const int k = blockIdx.x, chunk = blockIdx.y;
  const int t_begin = chunk * tiles_per_chunk, t_end = min(ntiles, (chunk + 1) * tiles_per_chunk);
  __shared__ short s_list[kMaxTilesPerChunk];
  const int n_active = build_active_list(masks, k, t_begin, t_end, s_list);
  f32x4 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  constexpr int NU8 = (kWR * (COUT_P / 8) + 255) / 256, CU8 = (kWR * (CIN_P / 8) + 255) / 256;
  float4 rn[BF_IO ? 1 : NU], rc[BF_IO ? 1 : CU];
  uint4 hn[BF_IO ? NU8 : 1], hc[BF_IO ? CU8 : 1];
  const unsigned short* in_h = reinterpret_cast<const unsigned short*>(in);
  const unsigned short* gout_h = reinterpret_cast<const unsigned short*>(gout);
  const bool vec_n = (cout & 3) == 0, vec_c = (cin & 3) == 0;
  auto fetch = [&](int t) {
    if constexpr (BF_IO) {
#pragma unroll
      for (int j = 0; j < NU8; ++j) {
        const int u = tid + 256 * j, r = u / (COUT_P / 8), n8 = (u - r * (COUT_P / 8)) * 8;
        const int p = t * kWR + r;
        hn[j] = make_uint4(0u, 0u, 0u, 0u);
        if (r < kWR && p < Mout && n8 < cout)
          hn[j] = *reinterpret_cast<const uint4*>(gout_h + (size_t)(order ? order[p] : p) * cout + n8);
      }
#pragma unroll
      for (int j = 0; j < CU8; ++j) {
        const int u = tid + 256 * j, r = u / (CIN_P / 8), c8 = (u - r * (CIN_P / 8)) * 8;
        const int p = t * kWR + r;
        hc[j] = make_uint4(0u, 0u, 0u, 0u);
        if (r < kWR && p < Mout && c8 < cin) {
          const int rr = nbr[(size_t)(order ? order[p] : p) * K + k];
          if (rr >= 0) hc[j] = *reinterpret_cast<const uint4*>(in_h + (size_t)rr * cin + c8);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < NU; ++j) {
        const int u = tid + 256 * j, r = u / (COUT_P / 4), n4 = (u - r * (COUT_P / 4)) * 4;
        const int p = t * kWR + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < kWR && p < Mout) {
          const float* src = gout + (size_t)(order ? order[p] : p) * cout + n4;
          if (vec_n) {
            if (n4 < cout) v = *reinterpret_cast<const float4*>(src);
          } else {
            if (n4 + 0 < cout) v.x = src[0];
            if (n4 + 1 < cout) v.y = src[1];
            if (n4 + 2 < cout) v.z = src[2];
            if (n4 + 3 < cout) v.w = src[3];
          }
        }
        rn[j] = v;
      }
#pragma unroll
      for (int j = 0; j < CU; ++j) {
        const int u = tid + 256 * j, r = u / (CIN_P / 4), c4 = (u - r * (CIN_P / 4)) * 4;
        const int p = t * kWR + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < kWR && p < Mout) {
          const int rr = nbr[(size_t)(order ? order[p] : p) * K + k];
          if (rr >= 0) {
            const float* src = in + (size_t)rr * cin + c4;
            if (vec_c) {
              if (c4 < cin) v = *reinterpret_cast<const float4*>(src);
            } else {
              if (c4 + 0 < cin) v.x = src[0];
              if (c4 + 1 < cin) v.y = src[1];
              if (c4 + 2 < cin) v.z = src[2];
              if (c4 + 3 < cin) v.w = src[3];
            }
          }
        }
        rc[j] = v;
      }
    }
  };
  auto commit = [&](int buf) {
    if constexpr (BF_IO) {
#pragma unroll
      for (int j = 0; j < NU8; ++j) {
        const int u = tid + 256 * j, r = u / (COUT_P / 8), n8 = (u - r * (COUT_P / 8)) * 8;
        if (r < kWR) *reinterpret_cast<uint4*>(Ns + (buf * kWR + r) * LDN + n8) = hn[j];
      }
#pragma unroll
      for (int j = 0; j < CU8; ++j) {
        const int u = tid + 256 * j, r = u / (CIN_P / 8), c8 = (u - r * (CIN_P / 8)) * 8;
        if (r < kWR) *reinterpret_cast<uint4*>(Cs + (buf * kWR + r) * LDC + c8) = hc[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < NU; ++j) {
        const int u = tid + 256 * j, r = u / (COUT_P / 4), n4 = (u - r * (COUT_P / 4)) * 4;
        if (r < kWR)
          *reinterpret_cast<uint2*>(Ns + (buf * kWR + r) * LDN + n4) =
              make_uint2(ud_pack_bf16x2(rn[j].x, rn[j].y), ud_pack_bf16x2(rn[j].z, rn[j].w));
      }
#pragma unroll
      for (int j = 0; j < CU; ++j) {
        const int u = tid + 256 * j, r = u / (CIN_P / 4), c4 = (u - r * (CIN_P / 4)) * 4;
        if (r < kWR)
          *reinterpret_cast<uint2*>(Cs + (buf * kWR + r) * LDC + c4) =
              make_uint2(ud_pack_bf16x2(rc[j].x, rc[j].y), ud_pack_bf16x2(rc[j].z, rc[j].w));
      }
    }
  };
  if (n_active > 0) {
    fetch(t_begin + s_list[0]);
    commit(0);
  }
  __syncthreads();
  int buf = 0;
  for (int ai = 0; ai < n_active; ++ai) {
    const bool more = ai + 1 < n_active;
    if (more) fetch(t_begin + s_list[ai + 1]);
    if (wave_on) {
      const unsigned short* nb = Ns + (buf * kWR + 8 * g + (li >> 2)) * LDN + 16 * TI * wm + 4 * (li & 3);
      const unsigned short* cb = Cs + (buf * kWR + 8 * g + (li >> 2)) * LDC + 16 * TJ * wn + 4 * (li & 3);
#pragma unroll
      for (int ks = 0; ks < kWR / 32; ++ks) {
        bf16x8 a[TI];
#pragma unroll
        for (int ti = 0; ti < TI; ++ti)
          a[ti] = tr_frag8(nb + 32 * ks * LDN + 16 * ti, nb + (32 * ks + 4) * LDN + 16 * ti);
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj) {
          const bf16x8 bb = tr_frag8(cb + 32 * ks * LDC + 16 * tj, cb + (32 * ks + 4) * LDC + 16 * tj);
#pragma unroll
          for (int ti = 0; ti < TI; ++ti)
            acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ti], bb, acc[ti][tj], 0, 0, 0);
        }
      }
    }
    if (more) commit(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  // partial[chunk][k][n][c] (padded sizes); D layout: column c = li, rows n = 4g + r
  if (wave_on) {
    float* pbase = partial + ((size_t)chunk * K + k) * COUT_P * CIN_P;
#pragma unroll
    for (int ti = 0; ti < TI; ++ti)
#pragma unroll
      for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          pbase[(size_t)(16 * (TI * wm + ti) + 4 * g + r) * CIN_P + 16 * (TJ * wn + tj) + li] = acc[ti][tj][r];
  }
}

// bf16-IO weight gradient with LDS-DMA staging (cin == CIN_P, cout == COUT_P in {64, 128}): the 64-row
// gout / gathered-input tiles go L2 -> LDS by global_load_lds_dwordx4 into unpadded rows whose 32-byte
// pieces are XOR-swizzled on the source address so that the transposing fragment reads
// (ds_read_b64_tr_b16: 8 rows x 32 B per 32 lanes) hit 8 different pieces; double-buffered, one barrier
// per tile.  Removes the ds_write pass that made the register-staged kernel LDS-bound.
template <int CIN_P, int COUT_P, bool GATHER_G>   // GATHER_G: gout rows are fetched through gorder
__global__ __launch_bounds__(256) void k_wgrad_bf16_dma(const unsigned short* __restrict__ in,
                                                        const int32_t* __restrict__ nbr, int K,
                                                        const unsigned short* __restrict__ gout,
                                                        float* __restrict__ partial, int Mout,
                                                        const int32_t* __restrict__ gorder,
                                                        const unsigned* __restrict__ masks, int ntiles,
                                                        int tiles_per_chunk) {
  constexpr int SN = COUT_P / 8, SC = CIN_P / 8;             // 16-byte slots per row
  constexpr int RN = 64 / SN, RC = 64 / SC;                   // rows per 1-KiB piece
  constexpr int PN = kWR / RN, PC = kWR / RC;                 // pieces per tile
  constexpr int NT = COUT_P / 16, CTT = CIN_P / 16;
  constexpr int TI = NT / 2, TJ = CTT / 2;                    // 2 x 2 waves
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned short* Ns = reinterpret_cast<unsigned short*>(smem);       // [2][kWR][COUT_P]
  unsigned short* Cs = Ns + 2 * kWR * COUT_P;                           // [2][kWR][CIN_P]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int wm = wave >> 1, wn = wave & 1;
  const int k = blockIdx.x, chunk = blockIdx.y;
  const int t_begin = chunk * tiles_per_chunk, t_end = min(ntiles, (chunk + 1) * tiles_per_chunk);
  __shared__ short s_list[kMaxTilesPerChunk];
  const int n_active = build_active_list(masks, k, t_begin, t_end, s_list);
  const unsigned short* zero = reinterpret_cast<const unsigned short*>(g_sp_zero16);
  // swizzle of the 32-byte piece index by the row (see the header comment); in 16-byte slot units << 1
  auto fsw = [](int r, int slots) -> int {
    // 256-, 128- and 64-byte rows: the 8 rows x 32 B of a half-wave fragment read land on distinct banks
    return slots == 16 ? (((r & 3) | ((r >> 1) & 4)) << 1)
                       : (slots == 8 ? ((((r >> 1) & 1) | (((r >> 3) & 1) << 1)) << 1) : (((r >> 3) & 1) << 1));
  };
  // The rows a tile gathers are known only through an index load (nbr; the host passes rulebook and gout rows
  // already in tile order).  Issued inside the staging it would put a memory latency in front of every
  // tile's DMA; it is issued one tile AHEAD instead, before this iteration's DMAs (so that nothing waits on
  // them), and lands while the tile is multiplied.
  struct TileIdx {
    int t;              // tile
    int rr[PC / 4];     // gathered input rows of this lane's pieces as loaded (validity is re-derived from t:
                        // nothing may consume the loaded values before the next iteration)
    int og[GATHER_G ? PN / 4 : 1];   // gout rows (GATHER_G)
  };
  auto load_idx = [&](int t, TileIdx& ix) {
    ix.t = t;
    if (GATHER_G) {
#pragma unroll
      for (int j = 0; j < PN / 4; ++j)
        ix.og[j] = gorder[min(t * kWR + (wave + 4 * j) * RN + lane / SN, Mout - 1)];
    }
#pragma unroll
    for (int j = 0; j < PC / 4; ++j) {
      const int p = t * kWR + (wave + 4 * j) * RC + lane / SC;
      ix.rr[j] = nbr[(size_t)min(p, Mout - 1) * K + k];         // branch-free: all loads issue back to back
    }
  };
  auto stage = [&](const TileIdx& ix, int buf) {
#pragma unroll
    for (int j = 0; j < PN / 4; ++j) {
      const int piece = wave + 4 * j, r = piece * RN + lane / SN, slot = lane % SN;
      const int p = ix.t * kWR + r;
      const unsigned short* src = zero;
      if (p < Mout) src = gout + (size_t)(GATHER_G ? ix.og[j] : p) * COUT_P + ((slot ^ fsw(r, SN)) << 3);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(Ns + (buf * kWR + piece * RN) * COUT_P),
                                       16, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < PC / 4; ++j) {
      const int piece = wave + 4 * j, r = piece * RC + lane / SC, slot = lane % SC;
      const int p = ix.t * kWR + r;
      const unsigned short* src = zero;
      if (p < Mout && ix.rr[j] >= 0) src = in + (size_t)ix.rr[j] * CIN_P + ((slot ^ fsw(r, SC)) << 3);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(Cs + (buf * kWR + piece * RC) * CIN_P),
                                       16, 0, 0);
    }
  };
  f32x4 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  TileIdx ix, nxt;
  if (n_active > 0) {
    load_idx(t_begin + s_list[0], ix);
    stage(ix, 0);
  }
  if (n_active > 1) load_idx(t_begin + s_list[1], ix);
  __syncthreads();
  int buf = 0;
  const int sub = (li & 3) >> 1, half = (li & 1) << 2;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  for (int ai = 0; ai < n_active; ++ai) {
    if (ai + 2 < n_active) load_idx(t_begin + s_list[ai + 2], nxt);  // lands while this tile is multiplied
    if (ai + 1 < n_active) stage(ix, buf ^ 1);
    {
      // transposing fragment read: lane li of a 16-lane group points at [row k0 + (li>>2)][channels c0 + 4*(li&3) ..+3].
      // Issued as inline asm + an explicit lgkmcnt wait tied to the fragment registers: the compiler makes
      // the ds_read_tr builtin wait for ALL outstanding LDS-DMA (vmcnt(0)), which would serialise the next
      // tile's DMAs behind this tile's MFMAs.
      const unsigned nbuf = lds0 + buf * (kWR * COUT_P * 2);
      const unsigned cbuf = lds0 + (2 * kWR * COUT_P + buf * kWR * CIN_P) * 2;
#pragma unroll
      for (int ks = 0; ks < kWR / 32; ++ks) {
        const int r0 = 32 * ks + 8 * g + (li >> 2), r1 = r0 + 4;
        v4s_t al[TI], ah[TI], bl[TJ], bh[TJ];
#pragma unroll
        for (int ti = 0; ti < TI; ++ti) {
          const int slot = 2 * (TI * wm + ti) + sub;
          al[ti] = tr_issue(nbuf + 2 * (r0 * COUT_P + ((slot ^ fsw(r0, SN)) << 3) + half));
          ah[ti] = tr_issue(nbuf + 2 * (r1 * COUT_P + ((slot ^ fsw(r1, SN)) << 3) + half));
        }
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj) {
          const int slot = 2 * (TJ * wn + tj) + sub;
          bl[tj] = tr_issue(cbuf + 2 * (r0 * CIN_P + ((slot ^ fsw(r0, SC)) << 3) + half));
          bh[tj] = tr_issue(cbuf + 2 * (r1 * CIN_P + ((slot ^ fsw(r1, SC)) << 3) + half));
        }
        asm volatile("s_waitcnt lgkmcnt(0)");
#pragma unroll
        for (int ti = 0; ti < TI; ++ti) asm volatile("" : "+v"(al[ti]), "+v"(ah[ti]));
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj) asm volatile("" : "+v"(bl[tj]), "+v"(bh[tj]));
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj) {
          const bf16x8 bb = cat8(bl[tj], bh[tj]);
#pragma unroll
          for (int ti = 0; ti < TI; ++ti)
            acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cat8(al[ti], ah[ti]), bb, acc[ti][tj], 0, 0, 0);
        }
      }
    }
    __syncthreads();
    buf ^= 1;
    ix = nxt;
  }
  float* pbase = partial + ((size_t)chunk * K + k) * COUT_P * CIN_P;
#pragma unroll
  for (int ti = 0; ti < TI; ++ti)
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        pbase[(size_t)(16 * (TI * wm + ti) + 4 * g + r) * CIN_P + 16 * (TJ * wn + tj) + li] = acc[ti][tj][r];
}

// gW[n][k][c] (KRSC, dense) = sum over chunks in order of partial[g][k][n][c]
__global__ __launch_bounds__(256) void k_wgrad_reduce(const float* __restrict__ partial, int G,
                                                      int K, int cinp, int coutp, int cin, int cout,
                                                      float* __restrict__ gW) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)cout * K * cin) return;
  const int c = (int)(t % cin);
  const int k = (int)((t / cin) % K);
  const int n = (int)(t / ((long long)cin * K));
  float acc = 0.f;
  for (int gi = 0; gi < G; ++gi)
    acc += partial[(((size_t)gi * K + k) * coutp + n) * cinp + c];
  gW[t] = acc;
}

__global__ __launch_bounds__(256) void k_wgrad_generic(const float* __restrict__ in, int cin,
                                                       const int32_t* __restrict__ nbr, int K,
                                                       const float* __restrict__ gout, int cout,
                                                       float* __restrict__ gW, int Mout) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)cout * K * cin) return;
  const int c = (int)(t % cin);
  const int k = (int)((t / cin) % K);
  const int n = (int)(t / ((long long)cin * K));
  float acc = 0.f;
  for (int o = 0; o < Mout; ++o) {
    const int r = nbr[(size_t)o * K + k];
    if (r >= 0) acc = fmaf(gout[(size_t)o * cout + n], in[(size_t)r * cin + c], acc);
  }
  gW[t] = acc;
}

template <int CIN_P, int COUT_P>
int launch_wgrad(const float* in, int cin, const int32_t* nbr, int K, const float* gout, int cout,
                 float* gW, int Mout, float* partial, int G, int rows_per_chunk,
                 hipStream_t stream) {
  dim3 grid(K, G);
  if (cin % 4 == 0 && cout % 4 == 0) {        // 16-byte row copies (every layer but the 5-channel input conv)
    const size_t lds = (size_t)kTM * (WgLd<CIN_P>::v + WgLd<COUT_P>::v) * sizeof(float) + kTM * sizeof(int);
    static UdDeviceOnce attr_set;
    if (const int e = ud_allow_dyn_lds(attr_set, (int)lds, k_wgrad_rows<CIN_P, COUT_P>)) return e;
    k_wgrad_rows<CIN_P, COUT_P><<<grid, 256, lds, stream>>>(in, cin, nbr, K, gout, cout, partial, Mout, rows_per_chunk);
  } else {
    const size_t lds = (size_t)(CIN_P + COUT_P) * (kTM + 4) * sizeof(float) + kTM * sizeof(int);
    static UdDeviceOnce attr_set;
    if (const int e = ud_allow_dyn_lds(attr_set, (int)lds, k_wgrad_mfma<CIN_P, COUT_P>)) return e;
    k_wgrad_mfma<CIN_P, COUT_P><<<grid, 256, lds, stream>>>(in, cin, nbr, K, gout, cout, partial,
                                                            Mout, rows_per_chunk);
  }
  UD_LAUNCH_CHECK();
  k_wgrad_reduce<<<ud_div_up((long long)cout * K * cin, 256), 256, 0, stream>>>(
      partial, G, K, CIN_P, COUT_P, cin, cout, gW);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

int wgrad_chunks(int Mout, int* rows_per_chunk) {
  // K x G workgroups: with K = 27 offsets, ~40 row chunks give ~1 000 workgroups (two rounds of two per CU); at least
  // 512 rows (8 tiles) per chunk.  (The first version used >= 4 096 rows per chunk: 216 workgroups for a 30 k-row layer.)
  int G = (Mout + 511) / 512;
  if (G > 40) G = 40;
  if (G < 1) G = 1;
  int rpc = (Mout + G - 1) / G;
  rpc = (rpc + kTM - 1) / kTM * kTM;
  *rows_per_chunk = rpc;
  return (Mout + rpc - 1) / rpc > 0 ? (Mout + rpc - 1) / rpc : 1;
}

}  // namespace

extern "C" size_t ud_spconv_wgrad_workspace_bytes(int Mout, int K, int Cin, int Cout) {
  if (Mout < 0 || K <= 0 || Cin <= 0 || Cout <= 0) return 0;
  int rpc;
  const int G = wgrad_chunks(Mout > 0 ? Mout : 1, &rpc);
  return ud_align_up((size_t)G * K * pad16(Cin) * pad16(Cout) * sizeof(float));
}

namespace {
// Row chunks per offset: many small (offset, chunk) units balance the very different number of active
// tiles per offset (the centre offset touches every tile, corner offsets a third of them); bounded by
// the size of the ordered partial-sum buffer (<= 128 MiB).
int wgrad_bf16_max_chunks(int K, int cin_p, int cout_p) {
  const long long per = (long long)K * cin_p * cout_p * (long long)sizeof(float);
  long long g = (128ll << 20) / (per > 0 ? per : 1);
  if (g > 64) g = 64;
  if (g < 8) g = 8;
  return (int)g;
}
int wgrad_bf16_chunks(int ntiles, int K, int cin_p, int cout_p, int* tiles_per_chunk) {
  int G = wgrad_bf16_max_chunks(K, cin_p, cout_p);
  if (G > ntiles) G = ntiles;
  if (G < 1) G = 1;
  *tiles_per_chunk = (ntiles + G - 1) / G;
  if (*tiles_per_chunk > kMaxTilesPerChunk) return -1;      // caller falls back (never at real sizes)
  return (ntiles + *tiles_per_chunk - 1) / *tiles_per_chunk;
}

template <int CIN_P, int COUT_P>
int launch_wgrad_bf16(const float* in, int cin, const int32_t* nbr, int K, const float* gout, int cout,
                      float* gW, int Mout, const int32_t* order, float* partial, unsigned* masks,
                      const unsigned* given_masks, int io_bf16, hipStream_t stream) {
  const int ntiles = ud_div_up(Mout, kWR);
  int tpc;
  const int G = wgrad_bf16_chunks(ntiles, K, CIN_P, COUT_P, &tpc);
  if (G < 0) return UD_ERR_UNSUPPORTED;
  if (given_masks) {
    masks = const_cast<unsigned*>(given_masks);
  } else {
    k_tile_masks<<<ud_div_up(ntiles, 4), 256, 0, stream>>>(nbr, K, order, Mout, masks, ntiles);
    UD_LAUNCH_CHECK();
  }
  const dim3 grid(K, G);
  // the DMA kernel walks nbr in tile order: either nothing is permuted (order NULL) or the caller passes a
  // rulebook already in row_order (io bit 1) and row_order only locates the gout rows
  const bool presorted = (io_bf16 & 2) != 0;
  constexpr bool dma_pair = (CIN_P == 32 || CIN_P == 64 || CIN_P == 128) && (COUT_P == 32 || COUT_P == 64 || COUT_P == 128);
  if (dma_pair && (io_bf16 & 1) && cin == CIN_P && cout == COUT_P && (order == nullptr || presorted)) {
    if constexpr (dma_pair) {
      const size_t lds_d = (size_t)2 * kWR * (CIN_P + COUT_P) * sizeof(unsigned short);
      static UdDeviceOnce dma_set;
      if (const int e = ud_allow_dyn_lds(dma_set, (int)lds_d, k_wgrad_bf16_dma<CIN_P, COUT_P, false>,
                                         k_wgrad_bf16_dma<CIN_P, COUT_P, true>))
        return e;
      const unsigned short* in16 = reinterpret_cast<const unsigned short*>(in);
      const unsigned short* g16 = reinterpret_cast<const unsigned short*>(gout);
      if (order)
        k_wgrad_bf16_dma<CIN_P, COUT_P, true><<<grid, 256, lds_d, stream>>>(in16, nbr, K, g16, partial, Mout, order, masks,
                                                                            ntiles, tpc);
      else
        k_wgrad_bf16_dma<CIN_P, COUT_P, false><<<grid, 256, lds_d, stream>>>(in16, nbr, K, g16, partial, Mout, nullptr,
                                                                             masks, ntiles, tpc);
    }
  } else {
    if (presorted) return UD_ERR_UNSUPPORTED;     // the pre-sorted-rulebook mode exists for the DMA kernel only
    const size_t lds = (size_t)2 * kWR * (CIN_P + COUT_P + 32) * sizeof(unsigned short);
    static UdDeviceOnce attr_set;
    if (const int e = ud_allow_dyn_lds(attr_set, (int)lds, k_wgrad_bf16<CIN_P, COUT_P, false>,
                                       k_wgrad_bf16<CIN_P, COUT_P, true>))
      return e;
    if (io_bf16 & 1)
      k_wgrad_bf16<CIN_P, COUT_P, true><<<grid, 256, lds, stream>>>(in, cin, nbr, K, gout, cout, partial, Mout, order,
                                                                    masks, ntiles, tpc);
    else
      k_wgrad_bf16<CIN_P, COUT_P, false><<<grid, 256, lds, stream>>>(in, cin, nbr, K, gout, cout, partial, Mout, order,
                                                                     masks, ntiles, tpc);
  }
  UD_LAUNCH_CHECK();
  k_wgrad_reduce<<<ud_div_up((long long)cout * K * cin, 256), 256, 0, stream>>>(
      partial, G, K, CIN_P, COUT_P, cin, cout, gW);
  UD_LAUNCH_CHECK();
  return UD_OK;
}
}  // namespace

extern "C" size_t ud_spconv_wgrad_bf16_workspace_bytes(int Mout, int K, int Cin, int Cout) {
  if (Mout < 0 || K <= 0 || Cin <= 0 || Cout <= 0) return 0;
  const int ntiles = ud_div_up(Mout > 0 ? Mout : 1, kWR);
  const size_t G = (size_t)wgrad_bf16_max_chunks(K, pad16(Cin), pad16(Cout));
  return ud_align_up(G * K * pad16(Cin) * pad16(Cout) * sizeof(float)) +
         ud_align_up((size_t)ntiles * sizeof(unsigned));
}

// Per-64-row-tile activity masks (bit k: some row of the tile has a pair at offset k) of a rulebook in
// the given row order; depends on the rulebook only, so callers may compute it once and reuse it.
extern "C" int ud_spconv_tile_masks(const int32_t* nbr, int Mout, int K, const int32_t* row_order,
                                    unsigned* masks, ud_stream_t stream_) {
  if (Mout < 0 || K <= 0 || K > 32) return UD_ERR_INVALID_ARG;
  if (Mout == 0) return UD_OK;
  if (!nbr || !masks) return UD_ERR_INVALID_ARG;
  const int ntiles = ud_div_up(Mout, kWR);
  k_tile_masks<<<ud_div_up(ntiles, 4), 256, 0, (hipStream_t)stream_>>>(nbr, K, row_order, Mout, masks, ntiles);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

// Mixed-precision weight gradient: bf16 operands (rounded when the row tiles are staged), fp32
// accumulation, ordered reduction.  row_order (optional) = the forward's mask-sorted row permutation.
extern "C" int ud_spconv_wgrad_bf16(const void* in_, const int32_t* nbr, const void* gout_, float* gW,
                                    int Mout, int K, int Cin, int Cout, int io_bf16,
                                    const int32_t* row_order, const unsigned* tile_masks,
                                    void* workspace, size_t workspace_bytes, ud_stream_t stream_) {
  const float* in = reinterpret_cast<const float*>(in_);
  const float* gout = reinterpret_cast<const float*>(gout_);
  if (Mout < 0 || K <= 0 || K > 32 || Cin <= 0 || Cout <= 0 || !gW) return UD_ERR_INVALID_ARG;
  if ((io_bf16 & 1) && ((Cin & 7) || (Cout & 7))) return UD_ERR_UNSUPPORTED;
  if ((io_bf16 & 2) && (!(io_bf16 & 1) || !row_order || !tile_masks)) return UD_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  if (Mout == 0) {
    UD_HIP_TRY(hipMemsetAsync(gW, 0, (size_t)Cout * K * Cin * sizeof(float), stream));
    return UD_OK;
  }
  if (!in || !nbr || !gout) return UD_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < ud_spconv_wgrad_bf16_workspace_bytes(Mout, K, Cin, Cout))
    return UD_ERR_WORKSPACE;
  const int cp = pad16(Cin), np = pad16(Cout);
  float* partial = reinterpret_cast<float*>(workspace);
  unsigned* masks = reinterpret_cast<unsigned*>(
      reinterpret_cast<char*>(workspace) +
      ud_align_up((size_t)wgrad_bf16_max_chunks(K, cp, np) * K * cp * np * sizeof(float)));
  UdProfScope prof("spconv.k_wgrad", stream);
#define X(A, B) \
  if (cp == A && np == B) \
    return launch_wgrad_bf16<A, B>(in, Cin, nbr, K, gout, Cout, gW, Mout, row_order, partial, masks, tile_masks, io_bf16, stream);
  UD_CONV_CASES(X)
#undef X
  return UD_ERR_UNSUPPORTED;
}

// gW f32[Cout,K,Cin] (dense KRSC) = sum_o gout[o,:]^T (x) in[nbr[o][k], :]
extern "C" int ud_spconv_wgrad(const float* in, const int32_t* nbr, const float* gout, float* gW,
                               int Mout, int K, int Cin, int Cout, int algo, void* workspace,
                               size_t workspace_bytes, ud_stream_t stream_) {
  if (Mout < 0 || K <= 0 || Cin <= 0 || Cout <= 0 || !gW) return UD_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  if (Mout == 0) {
    UD_HIP_TRY(hipMemsetAsync(gW, 0, (size_t)Cout * K * Cin * sizeof(float), stream));
    return UD_OK;
  }
  if (!in || !nbr || !gout) return UD_ERR_INVALID_ARG;
  const int cp = pad16(Cin), np = pad16(Cout);
  UdProfScope prof("spconv.k_wgrad", stream);
  if (algo != 1) {   // weight gradients accumulate in fp32 MFMA for every MFMA algo (0, 2, 3)
    int rpc;
    const int G = wgrad_chunks(Mout, &rpc);
    if (!workspace || workspace_bytes < ud_spconv_wgrad_workspace_bytes(Mout, K, Cin, Cout))
      return UD_ERR_WORKSPACE;
#define X(A, B) \
  if (cp == A && np == B) \
    return launch_wgrad<A, B>(in, Cin, nbr, K, gout, Cout, gW, Mout, (float*)workspace, G, rpc, stream);
    UD_CONV_CASES(X)
#undef X
  }
  k_wgrad_generic<<<ud_div_up((long long)Cout * K * Cin, 256), 256, 0, stream>>>(
      in, Cin, nbr, K, gout, Cout, gW, Mout);
  UD_LAUNCH_CHECK();
  return UD_OK;
}
