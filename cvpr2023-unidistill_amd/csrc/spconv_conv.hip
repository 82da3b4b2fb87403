// Sparse 3-D convolution compute kernels for MI355X / gfx950 (fp32, exact-f32 MFMA).
//
// Replaces spconv's gather-GEMM-scatter (ConvAlgo.Native) behind SubMConv3d / SparseConv3d
// (unidistill/layers/blocks_3d/det3d/spconv_backbone.py:21-48,71-92,259-340).
//
// Output-stationary implicit GEMM over the dense rulebook nbr[site][K] of spconv_index.hip:
//   out[o, :] = bias + sum_k sum_c in[nbr[o][k], c] * W[:, k, c]
// A 256-thread workgroup owns 64 output rows; per kernel offset k (skipped when no row of the
// tile has that neighbour) the gathered input rows and W[:,k,:] are staged in LDS and multiplied
// with v_mfma_f32_16x16x4_f32 (exact fp32, f32 accumulate).  No scatter-add, no fp atomics: the
// result is deterministic.  dgrad is the same kernel on the transposed rulebook with W's n/c
// strides swapped; wgrad reduces over row chunks into ordered partials.
#include "ud_common.h"
#include "ud_prof.h"
#include "spconv_tile.h"
#include <cstdlib>

namespace {

template <int CIN_P, int COUT_P>
__global__ __launch_bounds__(256) void k_conv_mfma(const float* __restrict__ in, int cin,
                                                   const int32_t* __restrict__ nbr, int K,
                                                   int mirror, const float* __restrict__ W,
                                                   WStrides ws, const float* __restrict__ bias,
                                                   float* __restrict__ out, int cout, int Mout) {
  constexpr int LDA = CIN_P + 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* As = reinterpret_cast<float*>(smem);       // [kTM][LDA]
  float* Bs = As + kTM * LDA;                        // [COUT_P][LDA]
  int* s_nbr = reinterpret_cast<int*>(Bs + COUT_P * LDA);  // [kTM]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int row0 = blockIdx.x * kTM;
  constexpr int NT = COUT_P / 16;
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int k = 0; k < K; ++k) {
    const int kk = mirror ? (K - 1 - k) : k;  // rulebook column to read for weight offset k
    int r = -1;
    if (tid < kTM && row0 + tid < Mout) r = nbr[(size_t)(row0 + tid) * K + kk];
    if (tid < kTM) s_nbr[tid] = r;
    if (!__syncthreads_or(r >= 0)) continue;  // nobody in this tile has neighbour k
    // ---- stage gathered input rows (zeros where the neighbour is missing / padded channels)
    if ((cin & 3) == 0) {
      for (int idx = tid; idx < kTM * (CIN_P / 4); idx += 256) {
        const int row = idx / (CIN_P / 4), c4 = (idx - row * (CIN_P / 4)) * 4;
        const int rr = s_nbr[row];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rr >= 0 && c4 < cin) v = *reinterpret_cast<const float4*>(in + (size_t)rr * cin + c4);
        *reinterpret_cast<float4*>(As + row * LDA + c4) = v;
      }
    } else {
      for (int idx = tid; idx < kTM * CIN_P; idx += 256) {
        const int row = idx / CIN_P, c = idx - row * CIN_P;
        const int rr = s_nbr[row];
        As[row * LDA + c] = (rr >= 0 && c < cin) ? in[(size_t)rr * cin + c] : 0.f;
      }
    }
    // ---- stage W[:, k, :] as Bs[n][c]
    if (ws.sc == 1 && (cin & 3) == 0) {
      for (int idx = tid; idx < COUT_P * (CIN_P / 4); idx += 256) {
        const int n = idx / (CIN_P / 4), c4 = (idx - n * (CIN_P / 4)) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n < cout && c4 < cin)
          v = *reinterpret_cast<const float4*>(W + n * ws.sn + k * ws.sk + c4);
        *reinterpret_cast<float4*>(Bs + n * LDA + c4) = v;
      }
    } else {
      // strided weights (dgrad reads W with n/c swapped): make n the fast thread index when sn == 1
      for (int idx = tid; idx < COUT_P * CIN_P; idx += 256) {
        int n, c;
        if (ws.sn == 1) {
          c = idx / COUT_P;
          n = idx - c * COUT_P;
        } else {
          n = idx / CIN_P;
          c = idx - n * CIN_P;
        }
        Bs[n * LDA + c] = (n < cout && c < cin) ? W[n * ws.sn + k * ws.sk + c * ws.sc] : 0.f;
      }
    }
    __syncthreads();
    // ---- MFMA: wave owns rows [16*wave, 16*wave+16) x all COUT_P columns
    const float* arow = As + (wave * 16 + li) * LDA + 4 * g;
#pragma unroll 2
    for (int cb = 0; cb < CIN_P / 16; ++cb) {
      const float4 a = *reinterpret_cast<const float4*>(arow + cb * 16);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float4 b = *reinterpret_cast<const float4*>(Bs + (t * 16 + li) * LDA + cb * 16 + 4 * g);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[t], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // ---- epilogue: acc[t][r] = out[row0 + 16*wave + 4*g + r][16*t + li]
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = t * 16 + li;
    if (col >= cout) continue;
    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + wave * 16 + 4 * g + r;
      if (row < Mout) out[(size_t)row * cout + col] = acc[t][r] + bv;
    }
  }
}

// ---- v2: 128-row tiles, 8 waves, register-prefetched staging (wide channels) --------------------
// Used when both padded channel counts are >= 64.  Differences to k_conv_mfma:
//   * the tile's whole rulebook slice (K x 128 neighbour ids) is read once into LDS and turned
//     into a block-level and per-wave activity mask -> no global read / block reduction per offset;
//   * the gathered rows and W[:,k,:] of the NEXT active offset are fetched into registers before
//     the MFMA phase of the current one (global latency hidden under the matrix work) and written
//     to LDS after it; a wave skips the MFMAs of offsets none of its 16 rows uses;
//   * MFMAs are issued round-robin over the accumulators (no back-to-back dependent pairs).

template <int CIN_P, int COUT_P, bool VA, bool VB>   // VA: cin % 4 == 0 (16-byte row pieces); VB: VA and channel-contiguous weights
__global__ __launch_bounds__(512) void k_conv_mfma_v2(const float* __restrict__ in, int cin,
                                                      const int32_t* __restrict__ nbr, int K,
                                                      int mirror, const float* __restrict__ W,
                                                      WStrides ws, const float* __restrict__ bias,
                                                      float* __restrict__ out, int cout, int Mout,
                                                      const int32_t* __restrict__ order,
                                                      ConvEpilogue ep) {
  // +8 floats per row: row stride = 8 (mod 64) banks, so the 16 lanes a ds_read_b128 serves together -- rows {0-3, 12-15}
  // of one 16-byte column and rows {4-11} of the next -- land on 16 distinct 16-byte slots (with +4, rows 11 and 12 of
  // neighbouring columns shared a slot: SQ_LDS_BANK_CONFLICT was 40 % of the LDS cycles)
  constexpr int LDA = CIN_P + 8;
  constexpr int NT = COUT_P / 16;
  constexpr int A4 = kTM2 * (CIN_P / 4) / 512;                  // float4 per thread for the A tile
  constexpr int B4 = (COUT_P * (CIN_P / 4) + 511) / 512;        // float4 per thread for the B tile
  constexpr int BU = COUT_P * (CIN_P / 4);                      // float4 units in the B tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* As = reinterpret_cast<float*>(smem);          // [kTM2][LDA]
  float* Bs = As + kTM2 * LDA;                          // [COUT_P][LDA]
  int* s_nbr = reinterpret_cast<int*>(Bs + COUT_P * LDA);  // [K][kTM2]
  // all LDS lives in the dynamic region (a static __shared__ in front would shift its base off
  // the 16-byte alignment the b128 reads need)
  unsigned& s_active = *reinterpret_cast<unsigned*>(s_nbr + K * kTM2);
  int* s_row = s_nbr + K * kTM2 + 4;                    // [kTM2] output row of each tile row (-1: none)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const SpTile tile = sp_tile_setup<16>(s_nbr, s_active, s_row, nbr, K, mirror, order, Mout, tid, lane, wave);
  const unsigned active = tile.active, wmask = tile.wmask;
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float4 ra[A4], rb[VB ? B4 : 1];
  // thread <-> (row or weight row r0 + RPP j, 16-byte channel piece c4): the same piece for every j
  constexpr int PER = CIN_P / 4, RPP = 512 / PER;
  const int r0 = tid / PER, c4 = (tid % PER) * 4;
  const bool cok = c4 < cin;
  const float* in_c = in + (cok ? c4 : 0);
  const int wc4 = cok ? c4 : 0;

  // The gathered rows AND W[:,k,:] of the next active offset are fetched into registers during the MFMA phase of the
  // current one and written to LDS after it.  Every load is unconditional (rows without a neighbour read row 0, weight
  // rows past cout re-read the last one; the zeros go in at commit time), and the vector / scalar variants are template
  // parameters: chosen at run time (round 1) the 128 x 128 instance needed 256 VGPRs and spilled 95 SGPRs, and its
  // weights were loaded synchronously inside the commit.
  auto fetch_a = [&](int k, int j) {
    const int rr = s_nbr[k * kTM2 + r0 + RPP * j];
    if constexpr (VA) {
      ra[j] = *reinterpret_cast<const float4*>(in_c + (size_t)(rr < 0 ? 0 : rr) * cin);
    } else {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rr >= 0) {
        const float* src = in + (size_t)rr * cin + c4;
        if (c4 + 0 < cin) v.x = src[0];
        if (c4 + 1 < cin) v.y = src[1];
        if (c4 + 2 < cin) v.z = src[2];
        if (c4 + 3 < cin) v.w = src[3];
      }
      ra[j] = v;
    }
  };
  auto fetch_b = [&](int k, int j) {
    if constexpr (VB) {
      const int n = r0 + RPP * j;
      // 32-bit offset from the (uniform) weight pointer: eight 64-bit row pointers would be hoisted out of the offset loop
      // and spilled
      if (n < COUT_P)
        rb[j] = *reinterpret_cast<const float4*>(W + (unsigned)(k * (int)ws.sk + (n < cout ? n : cout - 1) * (int)ws.sn + wc4));
    }
  };
  auto fetch = [&](int k) {
#pragma unroll
    for (int j = 0; j < A4; ++j) fetch_a(k, j);
#pragma unroll
    for (int j = 0; j < B4; ++j) fetch_b(k, j);
  };
  auto commit = [&](int k) {
    // component-wise selects: `ok ? ra[j] : zero4` on the float4 structs becomes a select of two ADDRESSES, which sends the
    // register arrays to scratch memory
    auto keep = [](bool ok, const float4& v) { return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f); };
#pragma unroll
    for (int j = 0; j < A4; ++j) {
      const int row = r0 + RPP * j;
      const bool ok = !VA || (cok && s_nbr[k * kTM2 + row] >= 0);
      *reinterpret_cast<float4*>(As + row * LDA + c4) = keep(ok, ra[j]);
    }
    if constexpr (VB) {
#pragma unroll
      for (int j = 0; j < B4; ++j) {
        const int n = r0 + RPP * j;
        if (n < COUT_P) *reinterpret_cast<float4*>(Bs + n * LDA + c4) = keep(cok && n < cout, rb[j]);
      }
    } else {
      // strided weights (dgrad: n is the fast axis in memory): thread <-> (c, 4 consecutive n)
#pragma unroll
      for (int j = 0; j < B4; ++j) {
        const int u = tid + 512 * j;
        if (u >= BU) break;
        const int c = u / (COUT_P / 4), n4 = (u - c * (COUT_P / 4)) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < cin) {
          const float* src = W + k * ws.sk + c * ws.sc;
          if (n4 + 0 < cout) v.x = src[(n4 + 0) * ws.sn];
          if (n4 + 1 < cout) v.y = src[(n4 + 1) * ws.sn];
          if (n4 + 2 < cout) v.z = src[(n4 + 2) * ws.sn];
          if (n4 + 3 < cout) v.w = src[(n4 + 3) * ws.sn];
        }
        Bs[(n4 + 0) * LDA + c] = v.x;
        Bs[(n4 + 1) * LDA + c] = v.y;
        Bs[(n4 + 2) * LDA + c] = v.z;
        Bs[(n4 + 3) * LDA + c] = v.w;
      }
    }
  };

  unsigned todo = active;
  int k = sp_next_offset(todo);
  if (k >= 0) fetch(k);
  while (k >= 0) {
    todo &= todo - 1;
    __builtin_amdgcn_sched_barrier(0);     // the phases stay apart too (same reason as between the matrix steps below)
    commit(k);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    const int knext = sp_next_offset(todo);
    // The next offset's loads are issued BETWEEN the matrix steps, one row piece (and at most one weight piece) per
    // 16-channel step: issued in one burst after the barrier, the eight waves' 128 KB of requests took 4 600 cycles to
    // get into the memory pipeline with the MFMA pipes idle (in-kernel cycle stamps).
    constexpr int CB = CIN_P / 16;
    static_assert(A4 == CB, "one gathered-row piece per 16-channel step");
    if ((wmask >> k) & 1u) {
      const float* arow = As + (wave * 16 + li) * LDA + 4 * g;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        if (knext >= 0) {
          fetch_a(knext, cb);
#pragma unroll
          for (int j = 0; j < B4; ++j)
            if (j * CB / B4 == cb) fetch_b(knext, j);
        }
        const float4 a = *reinterpret_cast<const float4*>(arow + cb * 16);
        float4 b[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
          b[t] = *reinterpret_cast<const float4*>(Bs + (t * 16 + li) * LDA + cb * 16 + 4 * g);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[t].x, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[t].y, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[t].z, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[t].w, acc[t], 0, 0, 0);
        // keep the steps apart: with the loop unrolled the scheduler hoists the fragment reads of several steps to the top
        // (256 VGPRs, 24 of them spilled in the 128 x 128 instance)
        __builtin_amdgcn_sched_barrier(0);
      }
    } else if (knext >= 0) {
      fetch(knext);
    }
    __syncthreads();
    k = knext;
  }
  // epilogue: acc[t][r] = out[s_row[16*wave + 4*g + r]][16*t + li]
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = t * 16 + li;
    if (col >= cout) continue;
    sp_epilogue_tile<false>(acc[t], s_row, wave * 16 + 4 * g, col, cout, bias, ep, out, false);
  }
}

// ---- bf16-MFMA variant (algo 3, mixed-precision mode) -------------------------------------------
// Same tiling / masks / prefetch as k_conv_mfma_v2, but the gathered rows and the weights are
// rounded to bf16 when they are written to LDS and multiplied with v_mfma_f32_16x16x32_bf16
// (fp32 accumulate): 8x fewer matrix instructions at ~2x the issue rate, so the wide layers stop
// being bound by the fp32 matrix pipe (157 TF) and become staging bound.  Inputs/outputs in HBM
// stay fp32.  Used when the caller runs under bf16 autocast; NOT bit-compatible with the fp32 path.

__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) { return ud_pack_bf16x2(a, b); }

template <int CIN_P, int COUT_P>   // CIN_P multiple of 32
__global__ __launch_bounds__(512) void k_conv_mfma_bf16(const float* __restrict__ in, int cin,
                                                        const int32_t* __restrict__ nbr, int K,
                                                        int mirror, const float* __restrict__ W,
                                                        WStrides ws, const float* __restrict__ bias,
                                                        float* __restrict__ out, int cout, int Mout,
                                                        const int32_t* __restrict__ order,
                                                        ConvEpilogue ep, int io) {
  // io bit 0: `in` holds bf16 rows; bit 1: `out` and ep.residual hold bf16; bit 2: W holds bf16
  const bool in_bf = io & 1, out_bf = io & 2, w_bf = io & 4;
  const unsigned short* in_h = reinterpret_cast<const unsigned short*>(in);
  const unsigned short* W_h = reinterpret_cast<const unsigned short*>(W);
  constexpr int LDB = CIN_P + 8;                                 // bf16 elements per LDS row
  constexpr int NT = COUT_P / 16;
  constexpr int A4 = kTM2 * (CIN_P / 4) / 512;
  constexpr int B4 = (COUT_P * (CIN_P / 4) + 511) / 512;
  constexpr int BU = COUT_P * (CIN_P / 4);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned short* As = reinterpret_cast<unsigned short*>(smem);  // [kTM2][LDB]
  unsigned short* Bs = As + kTM2 * LDB;                           // [COUT_P][LDB]
  int* s_nbr = reinterpret_cast<int*>(Bs + COUT_P * LDB);         // [K][kTM2]
  unsigned& s_active = *reinterpret_cast<unsigned*>(s_nbr + K * kTM2);
  int* s_row = s_nbr + K * kTM2 + 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const SpTile tile = sp_tile_setup<16>(s_nbr, s_active, s_row, nbr, K, mirror, order, Mout, tid, lane, wave);
  const unsigned active = tile.active, wmask = tile.wmask;
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const bool vecA = (cin & 3) == 0;
  const bool vecB = (ws.sc == 1) && vecA;
  float4 ra[A4];
  auto fetch = [&](int k) {
#pragma unroll
    for (int j = 0; j < A4; ++j) {
      const int u = tid + 512 * j;
      const int row = u / (CIN_P / 4), c4 = (u - row * (CIN_P / 4)) * 4;
      const int rr = s_nbr[k * kTM2 + row];
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rr >= 0 && in_bf) {          // bf16 rows (cin % 4 == 0): 8 bytes carry the 4 channels
        if (c4 < cin) {
          const uint2 h = *reinterpret_cast<const uint2*>(in_h + (size_t)rr * cin + c4);
          v.x = __uint_as_float(h.x);
          v.y = __uint_as_float(h.y);
        }
      } else if (rr >= 0) {
        const float* src = in + (size_t)rr * cin + c4;
        if (vecA) {
          if (c4 < cin) v = *reinterpret_cast<const float4*>(src);
        } else {
          if (c4 + 0 < cin) v.x = src[0];
          if (c4 + 1 < cin) v.y = src[1];
          if (c4 + 2 < cin) v.z = src[2];
          if (c4 + 3 < cin) v.w = src[3];
        }
      }
      ra[j] = v;
    }
  };
  auto commit = [&](int k) {
#pragma unroll
    for (int j = 0; j < A4; ++j) {
      const int u = tid + 512 * j;
      const int row = u / (CIN_P / 4), c4 = (u - row * (CIN_P / 4)) * 4;
      *reinterpret_cast<uint2*>(As + row * LDB + c4) =
          in_bf ? make_uint2(__float_as_uint(ra[j].x), __float_as_uint(ra[j].y))
                : make_uint2(pack_bf16x2(ra[j].x, ra[j].y), pack_bf16x2(ra[j].z, ra[j].w));
    }
    if (vecB) {
#pragma unroll
      for (int j = 0; j < B4; ++j) {
        const int u = tid + 512 * j;
        if (u >= BU) break;
        const int n = u / (CIN_P / 4), c4 = (u - n * (CIN_P / 4)) * 4;
        uint2 o = make_uint2(0u, 0u);
        if (n < cout && c4 < cin) {
          if (w_bf) {
            o = *reinterpret_cast<const uint2*>(W_h + n * ws.sn + k * ws.sk + c4);
          } else {
            const float4 v = *reinterpret_cast<const float4*>(W + n * ws.sn + k * ws.sk + c4);
            o = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
          }
        }
        *reinterpret_cast<uint2*>(Bs + n * LDB + c4) = o;
      }
    } else {
#pragma unroll
      for (int j = 0; j < B4; ++j) {
        const int u = tid + 512 * j;
        if (u >= BU) break;
        const int c = u / (COUT_P / 4), n4 = (u - c * (COUT_P / 4)) * 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (c < cin) {
          const float* src = W + k * ws.sk + c * ws.sc;
          for (int q = 0; q < 4; ++q)
            if (n4 + q < cout) v[q] = src[(n4 + q) * ws.sn];
        }
        for (int q = 0; q < 4; ++q)
          Bs[(n4 + q) * LDB + c] = (unsigned short)(ud_pack_bf16x2(v[q], 0.f) & 0xFFFFu);
      }
    }
  };
  unsigned todo = active;
  int k = sp_next_offset(todo);
  if (k >= 0) fetch(k);
  while (k >= 0) {
    todo &= todo - 1;
    commit(k);
    __syncthreads();
    const int knext = sp_next_offset(todo);
    if (knext >= 0) fetch(knext);
    if ((wmask >> k) & 1u) {
      const unsigned short* arow = As + (wave * 16 + li) * LDB + 8 * g;
#pragma unroll
      for (int cb = 0; cb < CIN_P / 32; ++cb) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(arow + cb * 32);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(Bs + (t * 16 + li) * LDB + cb * 32 + 8 * g);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
    k = knext;
  }
  // epilogue: acc[t][r] = out[s_row[16*wave + 4*g + r]][16*t + li]
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = t * 16 + li;
    if (col >= cout) continue;
    sp_epilogue_tile<true>(acc[t], s_row, wave * 16 + 4 * g, col, cout, bias, ep, out, out_bf);
  }
}

// ---- all-bf16 inference kernel (bf16 rows, bf16 weights, bf16 output) ------------------------------
// Same tile / mask scheme as k_conv_mfma_bf16, with everything the mixed-precision teacher path
// allows: 16-byte gathers of bf16 rows, the next offset's A rows AND weight slice prefetched in
// registers while the current one is multiplied (the weight slice was a synchronous L2 round trip
// per offset before -- the dominant cost once the products run on the bf16 pipe), and the output tile
// staged through LDS as fp32 so residual rows are read and results written as 16-byte pieces.
// bytes of the region shared by the operand tiles (K loop) and the staged fp32 output tile (epilogue)
__host__ __device__ constexpr size_t fast_front_bytes(int cin_p, int cout_p) {
  const size_t a = (size_t)(kTM2 + cout_p) * (cin_p + 8) * 2, o = (size_t)kTM2 * (cout_p + 4) * 4;
  return ((a > o ? a : o) + 15) / 16 * 16;
}

template <int CIN_P, int COUT_P>   // CIN_P multiple of 32; cin, cout multiples of 8
__global__ __launch_bounds__(512) void k_conv_mfma_bf16_fast(
    const unsigned short* __restrict__ in, int cin, const int32_t* __restrict__ nbr, int K, int mirror,
    const unsigned short* __restrict__ W, WStrides ws, const float* __restrict__ bias,
    unsigned short* __restrict__ out, int cout, int Mout, const int32_t* __restrict__ order,
    ConvEpilogue ep) {
  constexpr int LDB = CIN_P + 8;
  constexpr int NT = COUT_P / 16;
  constexpr int AU = kTM2 * (CIN_P / 8);            // 16-byte units of the A tile
  constexpr int BU = COUT_P * (CIN_P / 8);
  constexpr int A8 = (AU + 511) / 512, B8 = (BU + 511) / 512;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned short* As = reinterpret_cast<unsigned short*>(smem);
  unsigned short* Bs = As + kTM2 * LDB;
  int* s_nbr = reinterpret_cast<int*>(smem + fast_front_bytes(CIN_P, COUT_P));
  unsigned& s_active = *reinterpret_cast<unsigned*>(s_nbr + K * kTM2);
  int* s_row = s_nbr + K * kTM2 + 4;
  float* Os = reinterpret_cast<float*>(smem);       // [kTM2][COUT_P + 4] fp32, aliases As/Bs after the K loop
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const SpTile tile = sp_tile_setup<16>(s_nbr, s_active, s_row, nbr, K, mirror, order, Mout, tid, lane, wave);
  const unsigned active = tile.active, wmask = tile.wmask;
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  uint4 ra[A8], rb[B8];
  auto fetch = [&](int k) {
#pragma unroll
    for (int j = 0; j < A8; ++j) {
      const int u = tid + 512 * j;
      ra[j] = make_uint4(0u, 0u, 0u, 0u);
      if (u < AU) {
        const int row = u / (CIN_P / 8), c8 = (u - row * (CIN_P / 8)) * 8;
        const int rr = s_nbr[k * kTM2 + row];
        if (rr >= 0 && c8 < cin) ra[j] = *reinterpret_cast<const uint4*>(in + (size_t)rr * cin + c8);
      }
    }
#pragma unroll
    for (int j = 0; j < B8; ++j) {
      const int u = tid + 512 * j;
      rb[j] = make_uint4(0u, 0u, 0u, 0u);
      if (u < BU) {
        const int n = u / (CIN_P / 8), c8 = (u - n * (CIN_P / 8)) * 8;
        if (n < cout && c8 < cin) rb[j] = *reinterpret_cast<const uint4*>(W + n * ws.sn + k * ws.sk + c8);
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int j = 0; j < A8; ++j) {
      const int u = tid + 512 * j;
      if (u < AU) {
        const int row = u / (CIN_P / 8), c8 = (u - row * (CIN_P / 8)) * 8;
        *reinterpret_cast<uint4*>(As + row * LDB + c8) = ra[j];
      }
    }
#pragma unroll
    for (int j = 0; j < B8; ++j) {
      const int u = tid + 512 * j;
      if (u < BU) {
        const int n = u / (CIN_P / 8), c8 = (u - n * (CIN_P / 8)) * 8;
        *reinterpret_cast<uint4*>(Bs + n * LDB + c8) = rb[j];
      }
    }
  };
  unsigned todo = active;
  int k = sp_next_offset(todo);
  if (k >= 0) fetch(k);
  while (k >= 0) {
    todo &= todo - 1;
    commit();
    __syncthreads();
    const int knext = sp_next_offset(todo);
    if (knext >= 0) fetch(knext);
    if ((wmask >> k) & 1u) {
      const unsigned short* arow = As + (wave * 16 + li) * LDB + 8 * g;
#pragma unroll
      for (int cb = 0; cb < CIN_P / 32; ++cb) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(arow + cb * 32);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(Bs + (t * 16 + li) * LDB + cb * 32 + 8 * g);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
    k = knext;
  }
  // epilogue through LDS: acc[t][r] = tile row 16*wave + 4*g + r, column 16*t + li
#pragma unroll
  for (int t = 0; t < NT; ++t) sp_stage_out_tile<COUT_P>(Os, acc[t], wave * 16 + 4 * g, t * 16 + li, cout, bias, ep);
  sp_store_staged_bf16<COUT_P>(Os, s_row, ep, out, cout, tid);
}

// bytes of the LDS region shared by the double-buffered operand tiles and the staged fp32 output tile
__host__ __device__ constexpr size_t dma_front_bytes(int cin_p, int cout_p) {
  const int rpp = 64 / (cin_p / 8);
  const size_t a = (size_t)2 * (kTM2 + (cout_p + rpp - 1) / rpp * rpp) * cin_p * 2;
  const size_t o = (size_t)kTM2 * (cout_p + 4) * 4;
  return ((a > o ? a : o) + 15) / 16 * 16;
}

// ---- all-bf16 kernel with LDS-DMA staging -----------------------------------------------------------
// k_conv_mfma_bf16_fast with the gathered rows and the weight slice moved L2 -> LDS by
// global_load_lds_dwordx4 (no VGPR round trip, no ds_write), double-buffered so the next offset's
// operands fly while the current offset is multiplied: one barrier per offset instead of two.
template <int CIN_P, int COUT_P>   // cin == CIN_P in {32, 64, 128}; cout multiple of 8
__global__ __launch_bounds__(512) void k_conv_mfma_bf16_dma(
    const unsigned short* __restrict__ in, int cin, const int32_t* __restrict__ nbr, int K, int mirror,
    const unsigned short* __restrict__ W, WStrides ws, const float* __restrict__ bias,
    unsigned short* __restrict__ out, int cout, int Mout, const int32_t* __restrict__ order,
    ConvEpilogue ep) {
  constexpr int NT = COUT_P / 16;
  constexpr int S = CIN_P / 8;                      // 16-byte slots per (unpadded) LDS row
  constexpr int RPP = 64 / S;                       // rows per 1-KiB DMA piece
  constexpr int APIECES = kTM2 / RPP, BPIECES = (COUT_P + RPP - 1) / RPP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned short* As = reinterpret_cast<unsigned short*>(smem);            // [2][kTM2][CIN_P]
  unsigned short* Bs = As + 2 * kTM2 * CIN_P;                                // [2][BPIECES*RPP][CIN_P]
  int* s_nbr = reinterpret_cast<int*>(smem + dma_front_bytes(CIN_P, COUT_P));
  unsigned& s_active = *reinterpret_cast<unsigned*>(s_nbr + K * kTM2);
  int* s_row = s_nbr + K * kTM2 + 4;
  float* Os = reinterpret_cast<float*>(smem);       // [kTM2][COUT_P + 4] fp32, aliases As/Bs after the K loop
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const SpTile tile = sp_tile_setup<16>(s_nbr, s_active, s_row, nbr, K, mirror, order, Mout, tid, lane, wave);
  const unsigned active = tile.active, wmask = tile.wmask;
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // Row r of a tile keeps its 16-byte slot t at position t ^ swz(r): the swizzle is applied to the SOURCE
  // address (the DMA's LDS pattern is fixed: lane l lands at piece base + 16 l) and makes every
  // ds_read_b128 fragment load below conflict-free on the unpadded rows.
  auto swz = [](int r) -> int {
    if (S == 16) return r & 15;
    if (S == 8) return (r >> 1) & 7;
    const int q = (r >> 2) & 3;                      // S == 4
    return q == 0 ? 0 : (q == 1 ? 2 : (q == 2 ? 3 : 1));
  };
  const unsigned short* zero = reinterpret_cast<const unsigned short*>(g_sp_zero16);
  const int prow = lane / S, pslot = lane % S;
  auto stage = [&](int k, int buf) {
#pragma unroll
    for (int j = 0; j < (APIECES + 7) / 8; ++j) {
      const int piece = wave + 8 * j;
      if (piece < APIECES) {
        const int r = piece * RPP + prow;
        const int rr = s_nbr[k * kTM2 + r];
        const unsigned short* src = rr >= 0 ? in + (size_t)rr * cin + ((pslot ^ swz(r)) << 3) : zero;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(As + (buf * kTM2 + piece * RPP) * CIN_P),
                                         16, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < (BPIECES + 7) / 8; ++j) {
      const int piece = wave + 8 * j;
      if (piece < BPIECES) {
        const int n = piece * RPP + prow;
        const unsigned short* src = n < cout ? W + n * ws.sn + k * ws.sk + ((pslot ^ swz(n)) << 3) : zero;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(Bs + (buf * BPIECES * RPP + piece * RPP) * CIN_P),
                                         16, 0, 0);
      }
    }
  };
  unsigned todo = active;
  int k = sp_next_offset(todo);
  int buf = 0;
  if (k >= 0) stage(k, 0);
  __syncthreads();                                   // drains the DMAs (vmcnt(0)) and publishes the tiles
  while (k >= 0) {
    todo &= todo - 1;
    const int knext = sp_next_offset(todo);
    if (knext >= 0) stage(knext, buf ^ 1);           // flies while this offset is multiplied
    if ((wmask >> k) & 1u) {
      const int ar = wave * 16 + li;
      const unsigned short* arow = As + (buf * kTM2 + ar) * CIN_P;
      const int asw = swz(ar);
#pragma unroll
      for (int cb = 0; cb < CIN_P / 32; ++cb) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(arow + (((4 * cb + g) ^ asw) << 3));
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int n = t * 16 + li;
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(Bs + (buf * BPIECES * RPP + n) * CIN_P +
                                                             (((4 * cb + g) ^ swz(n)) << 3));
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
    buf ^= 1;
    k = knext;
  }
  // epilogue through LDS: acc[t][r] = tile row 16*wave + 4*g + r, column 16*t + li
#pragma unroll
  for (int t = 0; t < NT; ++t) sp_stage_out_tile<COUT_P>(Os, acc[t], wave * 16 + 4 * g, t * 16 + li, cout, bias, ep);
  sp_store_staged_bf16<COUT_P>(Os, s_row, ep, out, cout, tid);
}

// Any-size fallback (and the cross-check in tests): one thread per (row, n), sequential k, c.
__global__ __launch_bounds__(256) void k_conv_generic(const float* __restrict__ in, int cin,
                                                      const int32_t* __restrict__ nbr, int K,
                                                      int mirror, const float* __restrict__ W,
                                                      WStrides ws, const float* __restrict__ bias,
                                                      float* __restrict__ out, int cout, int Mout) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)Mout * cout) return;
  const int row = (int)(t / cout), n = (int)(t - (long long)row * cout);
  float acc = 0.f;
  for (int k = 0; k < K; ++k) {
    const int r = nbr[(size_t)row * K + (mirror ? K - 1 - k : k)];
    if (r < 0) continue;
    const float* x = in + (size_t)r * cin;
    const float* w = W + n * ws.sn + k * ws.sk;
    for (int c = 0; c < cin; ++c) acc = fmaf(x[c], w[c * ws.sc], acc);
  }
  out[t] = acc + (bias ? bias[n] : 0.f);
}

// ---- v3 (fp32, 64 / 128 channels, channel-contiguous weights): LDS-DMA, double-buffered 64-channel stages ---------------------
// k_conv_mfma_v2 above commits the gathered rows and the offset's weights through registers into ONE 153 KB tile: its waves
// spend 41-45 % of their time in the commit -> barrier -> MFMA -> barrier hand-over (81 TFLOP/s on the 128-channel layers).
// Here a stage = (active offset, 64-channel half of Cin): 128 gathered row pieces (256 B each) + Cout weight row pieces,
// moved L2 -> LDS by global_load_lds (per-lane source addresses: the gather costs no VGPR round trip, no ds_write), into one of
// TWO stage buffers: stage s + 1 flies while stage s is multiplied, one barrier per stage.  Rows are unpadded 256 B = 16
// 16-byte slots, XOR-swizzled with (row & 15) on the SOURCE address, so the b128 fragment reads (16 lanes = 16 rows, same
// logical slot) touch 16 distinct slots.  Waves: 4 (32 rows) x 2 (Cout / 2 columns); per 16-channel group a wave reads 2 A + NT B
// fragments for 8 NT MFMAs (a lane's 16-byte piece feeds four MFMAs, see conv2d_f32.hip).
constexpr unsigned kDmaOob = 0xFFFF0000u;      // size of the buffer descriptors of k_conv_dma_f32 = the byte offset that reads zeros
// LDS-DMA of 16 bytes per lane through a raw buffer descriptor: LDS[lds_wave_base + lane * 16] = buffer[voff + soff]; an offset past
// the descriptor's size reads zeros.  (A __device__ function: the builtin does not exist in the host pass, and a lambda of a
// kernel is compiled for both sides -- called from the lambda directly it silently drops the kernel's host stub.)
__device__ __forceinline__ void sp_dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff, unsigned lds_wave_base) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(size_t)lds_wave_base, 16, voff, soff, 0, 0);
}

// (A three-buffer ring for the 64 -> 64 layers -- two stages in flight under a counted vmcnt -- was measured in round 4 and
// removed in round 5: 670 us against k_conv_mfma_v2's 620 us on the step's four layers.)
template <int CIN, int COUT, int NBUF>
__global__ __launch_bounds__(512) void k_conv_dma_f32(const float* __restrict__ in, const int32_t* __restrict__ nbr, int K,
                                                      int mirror, const float* __restrict__ W, WStrides ws,
                                                      const float* __restrict__ bias, float* __restrict__ out, int Mout,
                                                      const int32_t* __restrict__ order, ConvEpilogue ep) {
  constexpr int NT = COUT / 32;                      // 16-column tiles per wave (2 column halves)
  constexpr int kAB = kTM2 * 256, kWB = COUT * 256, kStage = kAB + kWB;
  constexpr int kHalves = CIN / 64;
  constexpr int kAPieces = kTM2 / 4, kWPieces = COUT / 4;      // 1-KiB DMA pieces: 4 rows x 256 B
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* s_nbr = reinterpret_cast<int*>(smem + NBUF * kStage);   // [K][kTM2]
  unsigned& s_active = *reinterpret_cast<unsigned*>(s_nbr + K * kTM2);
  int* s_row = s_nbr + K * kTM2 + 4;                            // [kTM2]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int wm = wave >> 1, wn = wave & 1;
  // (per-wave mask over the wave's 32 rows: skipping per 16-row tile instead measured no faster)
  const SpTile tile = sp_tile_setup<32>(s_nbr, s_active, s_row, nbr, K, mirror, order, Mout, tid, lane, wm);
  const unsigned active = tile.active, wmask = tile.wmask;
  f32x4 acc[2][NT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[i][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // DMA of one stage: pieces are dealt to the 8 waves round-robin; lane -> (row 4 p + g, LDS slot li <- source slot li ^ (row & 15)).
  // Sources go through raw buffer descriptors (round 6): a lane's byte offset is ONE shift-add of the gathered row id (rows are
  // CIN * 4 = 256 / 512 bytes) -- or an out-of-range offset, which reads zeros, for a missing neighbour -- and the (offset, half)
  // part of a weight address rides in the scalar offset; the per-lane weight offsets are fixed for the whole launch.  With
  // 64-bit pointer arithmetic a stage cost every wave ~90 vector + ~70 scalar instructions beside its 128 MFMAs, and on this
  // chip every issued instruction of an fp32-MFMA kernel is paid in MFMA issue time (SQ counters, profiles/r06_spconv_encoder.md).
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void*)in, 0, (int)kDmaOob, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)W, 0, (int)kDmaOob, 0x00020000);
  const unsigned swz = (unsigned)((li ^ ((4 * wave + g) & 15)) << 4);      // (4 (wave + 8 i) + g) & 15 does not depend on i
  unsigned wvo[kWPieces / 8];
#pragma unroll
  for (int i = 0; i < kWPieces / 8; ++i) wvo[i] = (unsigned)(4 * (wave + 8 * i) + g) * (unsigned)ws.sn * 4u + swz;
  auto stage = [&](int k, int half, int buf) {
    const unsigned sb = (unsigned)(size_t)smem + buf * kStage;
    int rr[kAPieces / 8];
    {
      const unsigned na = NBUF * kStage + (unsigned)(k * kTM2 + 4 * wave + g) * 4u;              // one LDS round trip, not four
#pragma unroll
      for (int i = 0; i < kAPieces / 8; ++i) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(rr[i]) : "v"(na), "n"(i * 128));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int i = 0; i < kAPieces / 8; ++i) asm volatile("" : "+v"(rr[i]));
    }
    const unsigned sa = (unsigned)half * 256u;
    const unsigned sw = __builtin_amdgcn_readfirstlane((unsigned)k * (unsigned)ws.sk * 4u + (unsigned)half * 256u);
#pragma unroll
    for (int i = 0; i < kAPieces / 8; ++i) {
      const int p = wave + 8 * i;
      const unsigned vo = rr[i] >= 0 ? (unsigned)rr[i] * (unsigned)(CIN * 4) + swz : kDmaOob;
      sp_dma16(rin, vo, sa, sb + p * 1024);
    }
#pragma unroll
    for (int i = 0; i < kWPieces / 8; ++i) {
      const int p = wave + 8 * i;
      sp_dma16(rw, wvo[i], sw, sb + kAB + p * 1024);
    }
  };
  // fragment byte offsets inside a stage buffer, per 16-channel group cb: slot (4 cb + g) ^ li of row (tile * 16 + li)
  int fo[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) fo[cb] = li * 256 + (((4 * cb + g) ^ li) << 4);

  // stage list: (active offset, half) in order; m walks the offsets (its lowest set bit = the stage's offset)
  auto succ = [&](int& k, int& half, unsigned& m) {
    if (++half == kHalves) {
      half = 0;
      m &= m - 1;
      k = sp_next_offset(m);
    }
  };
  unsigned m0 = active;
  int k = sp_next_offset(m0), half = 0, buf = 0;
  int k1 = k, h1 = half;
  unsigned m1 = m0;
  if (k >= 0) {
    stage(k, 0, 0);
    succ(k1, h1, m1);
  }
  while (k >= 0) {
    // the stage after the next one
    int k2 = k1, h2 = h1;
    unsigned m2 = m1;
    if (k1 >= 0) succ(k2, h2, m2);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // raw barrier: __syncthreads() is lowered to `s_waitcnt vmcnt(0) lgkmcnt(0)` + s_barrier, which would drain the stage in
    // flight.  The waves' own LDS reads (inline asm) were awaited with lgkmcnt(0) before their last MFMA group.
    __builtin_amdgcn_s_barrier();          // this stage has landed for everybody; everybody is done with the previous stage's buffer
    asm volatile("" ::: "memory");
    if (k1 >= 0) stage(k1, h1, buf ^ 1);
    if ((wmask >> k) & 1u) {
      // fragment reads by hand, one 16-channel group ahead of its MFMAs: hipcc puts `s_waitcnt vmcnt(0)` in front of a compiled LDS
      // read that follows an LDS-DMA issue -- i.e. it waited here for the NEXT stage's DMA issued four lines up, and the double
      // buffer bought nothing
      const unsigned ab = buf * kStage + (wm * 32) * 256, wb = buf * kStage + kAB + (wn * (COUT / 2)) * 256;
      f32x4 fa[2][2], fbv[2][NT];
#define UD_SD_LOADS(BUF, CB)                                                                                            \
  do {                                                                                                                  \
    const unsigned va_ = ab + fo[CB], vb_ = wb + fo[CB];                                                                \
    _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                                       \
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fa[BUF][i]) : "v"(va_), "n"(i * 4096));                       \
    _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                                      \
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fbv[BUF][t]) : "v"(vb_), "n"(t * 4096));                      \
  } while (0)
      UD_SD_LOADS(0, 0);
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const int cur = cb & 1;
        if (cb + 1 < 4) {
          if (cur == 0) UD_SD_LOADS(1, cb + 1); else UD_SD_LOADS(0, cb + 1);
          if (NT == 4) asm volatile("s_waitcnt lgkmcnt(6)" ::: "memory"); else asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
        } else {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) asm volatile("" : "+v"(fa[cur][i]));       // the values are valid from here on
#pragma unroll
        for (int t = 0; t < NT; ++t) asm volatile("" : "+v"(fbv[cur][t]));
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 2; ++i)
              acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[cur][i][e], fbv[cur][t][e], acc[i][t], 0, 0, 0);
      }
#undef UD_SD_LOADS
    }
    k = k1, half = h1, m0 = m1;
    k1 = k2, h1 = h2, m1 = m2;
    buf = buf + 1 == NBUF ? 0 : buf + 1;
  }
  // epilogue: acc[i][t][r] = out[row(wm * 32 + 16 i + 4 g + r)][wn * COUT / 2 + 16 t + li]
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = wn * (COUT / 2) + t * 16 + li;
    const float bv = bias ? bias[col] : 0.f;
    const float sc = ep.scale ? ep.scale[col] : 1.f;
    const float sh = ep.shift ? ep.shift[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = s_row[wm * 32 + 16 * i + 4 * g + r];
        if (row >= 0) {
          float v = acc[i][t][r] + bv;
          if (ep.scale) v = v * sc + sh;
          if (ep.residual) v += ep.residual[(size_t)row * COUT + col];
          if (ep.relu) v = fmaxf(v, 0.f);
          out[(size_t)row * COUT + col] = v;
        }
      }
  }
}

template <int CIN, int COUT>
int launch_conv_dma_f32(const float* in, const int32_t* nbr, int K, int mirror, const float* W, WStrides ws,
                        const float* bias, float* out, int Mout, const int32_t* order, ConvEpilogue ep,
                        hipStream_t stream) {
  constexpr int NBUF = 2;
  constexpr size_t front = NBUF * (size_t)(kTM2 * 256 + COUT * 256);
  const size_t lds = front + sp_tile_meta_bytes(K);
  if (lds > kSpLdsMax) return UD_ERR_UNSUPPORTED;
  static UdDeviceOnce attr_set;
  if (const int e = ud_allow_dyn_lds(attr_set, sp_lds_limit(front), k_conv_dma_f32<CIN, COUT, NBUF>)) return e;
  k_conv_dma_f32<CIN, COUT, NBUF><<<ud_div_up(Mout, kTM2), 512, lds, stream>>>(in, nbr, K, mirror, W, ws, bias, out, Mout, order, ep);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

template <int CIN_P, int COUT_P>
int launch_conv_v2(const float* in, int cin, const int32_t* nbr, int K, int mirror, const float* W,
                   WStrides ws, const float* bias, float* out, int cout, int Mout,
                   const int32_t* order, ConvEpilogue ep, hipStream_t stream) {
  constexpr size_t front = (size_t)(kTM2 + COUT_P) * (CIN_P + 8) * sizeof(float);
  const size_t lds = front + sp_tile_meta_bytes(K);
  static UdDeviceOnce attr_set;
  if (const int e = ud_allow_dyn_lds(attr_set, sp_lds_limit(front), k_conv_mfma_v2<CIN_P, COUT_P, true, true>,
                                     k_conv_mfma_v2<CIN_P, COUT_P, true, false>, k_conv_mfma_v2<CIN_P, COUT_P, false, false>))
    return e;
  const bool va = (cin & 3) == 0, vb = va && ws.sc == 1;
  const dim3 grid(ud_div_up(Mout, kTM2));
  if (vb)
    k_conv_mfma_v2<CIN_P, COUT_P, true, true><<<grid, 512, lds, stream>>>(in, cin, nbr, K, mirror, W, ws, bias, out, cout,
                                                                          Mout, order, ep);
  else if (va)
    k_conv_mfma_v2<CIN_P, COUT_P, true, false><<<grid, 512, lds, stream>>>(in, cin, nbr, K, mirror, W, ws, bias, out, cout,
                                                                           Mout, order, ep);
  else
    k_conv_mfma_v2<CIN_P, COUT_P, false, false><<<grid, 512, lds, stream>>>(in, cin, nbr, K, mirror, W, ws, bias, out,
                                                                            cout, Mout, order, ep);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

template <int CIN_P, int COUT_P>
int launch_conv_bf16(const float* in, int cin, const int32_t* nbr, int K, int mirror, const float* W,
                     WStrides ws, const float* bias, float* out, int cout, int Mout,
                     const int32_t* order, ConvEpilogue ep, int io, hipStream_t stream) {
  constexpr int CP = CIN_P < 32 ? 32 : CIN_P;
  if ((io & 1) && (cin & 3)) return UD_ERR_UNSUPPORTED;          // bf16 rows are read 4 channels at a time
  if ((io & 4) && !(ws.sc == 1 && (cin & 3) == 0)) return UD_ERR_UNSUPPORTED;
  if (io == 7 && cin == CP && (cout & 7) == 0 && (ws.sn & 7) == 0 && (ws.sk & 7) == 0) {
    const size_t lds_d = dma_front_bytes(CP, COUT_P) + sp_tile_meta_bytes(K);
    if (lds_d <= kSpLdsMax) {
      static UdDeviceOnce dma_attr_set;
      if (const int e = ud_allow_dyn_lds(dma_attr_set, sp_lds_limit(dma_front_bytes(CP, COUT_P)), k_conv_mfma_bf16_dma<CP, COUT_P>))
        return e;
      k_conv_mfma_bf16_dma<CP, COUT_P><<<ud_div_up(Mout, kTM2), 512, lds_d, stream>>>(
          reinterpret_cast<const unsigned short*>(in), cin, nbr, K, mirror,
          reinterpret_cast<const unsigned short*>(W), ws, bias, reinterpret_cast<unsigned short*>(out), cout,
          Mout, order, ep);
      UD_LAUNCH_CHECK();
      return UD_OK;
    }
  }
  if (io == 7 && (cin & 7) == 0 && (cout & 7) == 0 && (ws.sn & 7) == 0 && (ws.sk & 7) == 0) {
    const size_t lds_f = fast_front_bytes(CP, COUT_P) + sp_tile_meta_bytes(K);
    static UdDeviceOnce fast_attr_set;
    if (const int e = ud_allow_dyn_lds(fast_attr_set, sp_lds_limit(fast_front_bytes(CP, COUT_P)), k_conv_mfma_bf16_fast<CP, COUT_P>))
      return e;
    k_conv_mfma_bf16_fast<CP, COUT_P><<<ud_div_up(Mout, kTM2), 512, lds_f, stream>>>(
        reinterpret_cast<const unsigned short*>(in), cin, nbr, K, mirror,
        reinterpret_cast<const unsigned short*>(W), ws, bias, reinterpret_cast<unsigned short*>(out), cout,
        Mout, order, ep);
    UD_LAUNCH_CHECK();
    return UD_OK;
  }
  constexpr size_t front = (size_t)(kTM2 + COUT_P) * (CP + 8) * sizeof(unsigned short);
  const size_t lds = front + sp_tile_meta_bytes(K);
  static UdDeviceOnce attr_set;
  if (const int e = ud_allow_dyn_lds(attr_set, sp_lds_limit(front), k_conv_mfma_bf16<CP, COUT_P>)) return e;
  k_conv_mfma_bf16<CP, COUT_P><<<ud_div_up(Mout, kTM2), 512, lds, stream>>>(
      in, cin, nbr, K, mirror, W, ws, bias, out, cout, Mout, order, ep, io);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

template <int CIN_P, int COUT_P>
int launch_conv(const float* in, int cin, const int32_t* nbr, int K, int mirror, const float* W,
                WStrides ws, const float* bias, float* out, int cout, int Mout,
                const int32_t* order, ConvEpilogue ep, int algo, hipStream_t stream) {
  if (K <= 32 && algo == 3)
    return launch_conv_bf16<CIN_P, COUT_P>(in, cin, nbr, K, mirror, W, ws, bias, out, cout, Mout, order, ep, 0, stream);
  // fp32, 64 / 128 channels exactly, channel-contiguous 16-byte-aligned weights: the LDS-DMA kernel
  // 64 -> 64 stays on k_conv_mfma_v2: a stage there is 64 MFMAs per wave, shorter than the DMA round trip and than the skew of
  // an 8-wave barrier.  Measured on the step's four 64 -> 64 layers (394 k rows, 5.45 M pairs): v2 620 us, this kernel with two
  // stage buffers 700 us (round 3), with a three-stage ring 670 us (round 4; removed), with the round-6 descriptor addressing 660 us.
  if constexpr ((CIN_P == 64 || CIN_P == 128) && (COUT_P == 64 || COUT_P == 128) && !(CIN_P == 64 && COUT_P == 64)) {
    static const bool no_dma = getenv("UD_SPCONV_NO_DMA") != nullptr;       // A/B timing
    // (32-bit byte offsets into W through a buffer descriptor; the INPUT tensor must be smaller than 4 GiB - 64 KiB as well --
    // the entry point does not know its row count: include/unidistill_hip.h states the limit, ops/spconv.py enforces it)
    const long long w_span = ((long long)(cout - 1) * ws.sn + (long long)(K - 1) * ws.sk + cin) * 4;
    if (!no_dma && K <= 32 && algo == 0 && cin == CIN_P && cout == COUT_P && ws.sc == 1 && (ws.sn & 3) == 0 && (ws.sk & 3) == 0 &&
        ws.sn >= 0 && ws.sk >= 0 && w_span < (long long)kDmaOob && ((size_t)W & 15) == 0 && ((size_t)in & 15) == 0)
      return launch_conv_dma_f32<CIN_P, COUT_P>(in, nbr, K, mirror, W, ws, bias, out, Mout, order, ep, stream);
  }
  // activity masks are 32-bit; the LDS rulebook slice must fit next to the tiles
  if (K <= 32 && algo != 2)
    return launch_conv_v2<CIN_P, COUT_P>(in, cin, nbr, K, mirror, W, ws, bias, out, cout, Mout, order, ep, stream);
  if (ep.scale || ep.residual || ep.relu) return UD_ERR_UNSUPPORTED;
  const size_t lds = (size_t)(kTM + COUT_P) * (CIN_P + 4) * sizeof(float) + kTM * sizeof(int);
  static UdDeviceOnce attr_set;
  if (const int e = ud_allow_dyn_lds(attr_set, (int)lds, k_conv_mfma<CIN_P, COUT_P>)) return e;
  k_conv_mfma<CIN_P, COUT_P><<<ud_div_up(Mout, kTM), 256, lds, stream>>>(
      in, cin, nbr, K, mirror, W, ws, bias, out, cout, Mout);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

}  // namespace

// out f32[Mout,Cout] = bias + implicit-GEMM over nbr i32[Mout,K] of in f32[Min,Cin] with weights
// addressed as W[n*w_sn + k*w_sk + c*w_sc] (n < Cout, k < K, c < Cin).  mirror != 0 reads rulebook
// column K-1-k for weight offset k (submanifold dgrad).  algo, when the padded channel pair is instantiated
// (otherwise the generic kernel runs): 0 = fp32 MFMA (LDS-DMA kernel or k_conv_mfma_v2), 1 = force the generic
// VALU kernel, 2 = the first-generation fp32 MFMA kernel, 3 = bf16 MFMA (fp32 tensors, bf16 operands).
extern "C" int ud_spconv_conv(const float* in, const int32_t* nbr, const float* W, int64_t w_sn,
                              int64_t w_sk, int64_t w_sc, int mirror, const float* bias,
                              float* out, int Mout, int K, int Cin, int Cout, int algo,
                              const int32_t* row_order, const float* ep_scale,
                              const float* ep_shift, const float* ep_residual, int ep_relu,
                              ud_stream_t stream_) {
  if (Mout < 0 || K <= 0 || Cin <= 0 || Cout <= 0) return UD_ERR_INVALID_ARG;
  if (Mout == 0) return UD_OK;
  if (!in || !nbr || !W || !out) return UD_ERR_INVALID_ARG;
  if ((ep_scale == nullptr) != (ep_shift == nullptr)) return UD_ERR_INVALID_ARG;
  ConvEpilogue ep{ep_scale, ep_shift, ep_residual, ep_relu};
  hipStream_t stream = (hipStream_t)stream_;
  WStrides ws{w_sn, w_sk, w_sc};
  const int cp = pad16(Cin), np = pad16(Cout);
  UdProfScope prof("spconv.k_conv", stream);
  if (algo == 0 || algo == 2 || algo == 3) {   // 0: fp32 MFMA, 2: first-generation kernel, 3: bf16 MFMA
#define X(A, B) \
  if (cp == A && np == B) \
    return launch_conv<A, B>(in, Cin, nbr, K, mirror, W, ws, bias, out, Cout, Mout, row_order, ep, algo, stream);
    UD_CONV_CASES(X)
#undef X
  }
  if (ep.scale || ep.residual || ep.relu) return UD_ERR_UNSUPPORTED;
  k_conv_generic<<<ud_div_up((long long)Mout * Cout, 256), 256, 0, stream>>>(
      in, Cin, nbr, K, mirror, W, ws, bias, out, Cout, Mout);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

// Mixed-precision inference variant of ud_spconv_conv: the bf16 MFMA kernel with bf16 tensors in HBM.
// io_flags bit 0: in is bf16 [*, Cin]; bit 1: out and ep_residual are bf16 [Mout, Cout]; bit 2: W is bf16.
extern "C" int ud_spconv_conv_bf16io(const void* in, const int32_t* nbr, const void* W, int64_t w_sn,
                                     int64_t w_sk, int64_t w_sc, int mirror, const float* bias,
                                     void* out, int Mout, int K, int Cin, int Cout, int io_flags,
                                     const int32_t* row_order, const float* ep_scale,
                                     const float* ep_shift, const void* ep_residual, int ep_relu,
                                     ud_stream_t stream_) {
  if (Mout < 0 || K <= 0 || K > 32 || Cin <= 0 || Cout <= 0 || (io_flags & ~7)) return UD_ERR_INVALID_ARG;
  if (Mout == 0) return UD_OK;
  if (!in || !nbr || !W || !out) return UD_ERR_INVALID_ARG;
  if ((ep_scale == nullptr) != (ep_shift == nullptr)) return UD_ERR_INVALID_ARG;
  ConvEpilogue ep{ep_scale, ep_shift, reinterpret_cast<const float*>(ep_residual), ep_relu};
  hipStream_t stream = (hipStream_t)stream_;
  WStrides ws{w_sn, w_sk, w_sc};
  const int cp = pad16(Cin), np = pad16(Cout);
  UdProfScope prof("spconv.k_conv", stream);
#define X(A, B)             \
  if (cp == A && np == B)   \
    return launch_conv_bf16<A, B>(reinterpret_cast<const float*>(in), Cin, nbr, K, mirror,           \
                                  reinterpret_cast<const float*>(W), ws, bias,                        \
                                  reinterpret_cast<float*>(out), Cout, Mout, row_order, ep, io_flags, \
                                  stream);
  UD_CONV_CASES(X)
#undef X
  return UD_ERR_UNSUPPORTED;
}
