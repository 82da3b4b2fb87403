// Shared by the sparse-convolution translation units (spconv_conv.hip: forward / dgrad, spconv_wgrad.hip: weight
// gradient): the tile constants and argument structs, and the tile prologue / epilogue every 128-row forward kernel runs.
//
// The device helpers are __forceinline__ and take what the kernels already hold in registers BY VALUE (tid, lane, one
// accumulator tile at a time): the kernels sit at the register limit, and a register array whose address escapes goes
// to scratch memory.
#pragma once
#include "ud_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kTM = 64;    // output rows per workgroup (first-generation kernels, fp32 weight gradient)
constexpr int kTM2 = 128;  // output rows per workgroup (512-thread forward kernels)

// W element (n, k, c) lives at W[n*sn + k*sk + c*sc]
struct WStrides {
  long long sn, sk, sc;
};

// Optional fused epilogue: y = relu?((conv + bias) * scale + shift + residual)
struct ConvEpilogue {
  const float* scale;     // [Cout] or nullptr
  const float* shift;     // [Cout] or nullptr
  const float* residual;  // [Mout, Cout] or nullptr
  int relu;
};

inline int pad16(int c) { return (c + 15) / 16 * 16; }

#define UD_CONV_CASES(X) \
  X(16, 16) X(16, 32) X(32, 16) X(32, 32) X(32, 64) X(64, 32) X(64, 64) X(64, 128) X(128, 64) X(128, 128)

// LDS behind the operand tiles of a 128-row kernel: s_nbr[K][kTM2], s_active (16 bytes keep the alignment), s_row[kTM2]
constexpr size_t sp_tile_meta_bytes(int K) { return (size_t)K * kTM2 * sizeof(int) + 16 + kTM2 * sizeof(int); }
constexpr int kSpMaxK = 32;                 // activity masks are 32-bit: the entry points route K <= 32 to these kernels
constexpr size_t kSpLdsMax = 160 * 1024;    // LDS of a CU
// Dynamic-LDS limit to allow for a kernel whose operand tiles take `front` bytes: the request of a launch depends on
// the runtime K, and the limit is set once per device -- sized for this call's K, a K = 3 layer launched first would
// pin it below what a later K = 27 layer needs.
constexpr int sp_lds_limit(size_t front) {
  return (int)(front + sp_tile_meta_bytes(kSpMaxK) < kSpLdsMax ? front + sp_tile_meta_bytes(kSpMaxK) : kSpLdsMax);
}

#ifdef __HIPCC__
// Out-of-rulebook rows and output channels past cout are DMA'd from here (LDS-DMA cannot write a constant).
__device__ __attribute__((aligned(16))) unsigned int g_sp_zero16[4];

// Lowest set bit of an activity mask = the next active kernel offset; -1 when none is left.
__device__ __forceinline__ int sp_next_offset(unsigned todo) { return todo ? (__ffs((int)todo) - 1) : -1; }

struct SpTile {
  int row0;          // first position of this workgroup's tile in the row order
  unsigned active;   // bit k: some row of the tile has a neighbour at offset k
  unsigned wmask;    // the same for the calling wave's RPW rows
};

// Tile prologue of the 128-row kernels (512 threads).  Fills s_row[kTM2] (tile row -> output row, -1: none) and
// s_nbr[K][kTM2] (the tile's rulebook slice; column K-1-k of the rulebook serves weight offset k when mirror is set)
// and returns the activity masks.  The calling wave's RPW rows are tile rows [wgroup * RPW, wgroup * RPW + RPW).  Ends after a barrier: the
// LDS arrays are complete when it returns.
template <int RPW>
__device__ __forceinline__ SpTile sp_tile_setup(int* s_nbr, unsigned& s_active, int* s_row,
                                                const int32_t* nbr, int K, int mirror,
                                                const int32_t* order, int Mout, int tid, int lane,
                                                int wgroup) {
  SpTile t;
  t.row0 = (int)(gridDim.x - 1u - blockIdx.x) * kTM2;   // mask-sorted rows: the tiles with the most active offsets sit at the end -> dispatch them first (longest first)
  if (tid == 0) s_active = 0u;
  // tile row -> output row: identity, or the caller's mask-sorted order (rows with similar
  // neighbour masks share a tile, so far fewer offsets are active per tile)
  if (tid < kTM2) {
    const int p = t.row0 + tid;
    s_row[tid] = (p < Mout) ? (order ? order[p] : p) : -1;
  }
  __syncthreads();
  // rulebook slice -> LDS (column kk of the rulebook serves weight offset k)
  unsigned mine = 0u;
  for (int idx = tid; idx < kTM2 * K; idx += 512) {
    const int r = idx / K, k = idx - r * K;
    int v = -1;
    const int orow = s_row[r];
    if (orow >= 0) v = nbr[(size_t)orow * K + (mirror ? K - 1 - k : k)];
    s_nbr[k * kTM2 + r] = v;
    if (v >= 0) mine |= 1u << k;
  }
  // block-wide OR of the per-thread masks
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine |= __shfl_xor((int)mine, o);
  if (lane == 0 && mine) atomicOr(&s_active, mine);
  __syncthreads();
  t.active = s_active;
  // per-wave mask: which offsets do my RPW rows use
  t.wmask = 0u;
  for (int k = 0; k < K; ++k) {
    const int v = (lane < RPW) ? s_nbr[k * kTM2 + wgroup * RPW + lane] : -1;
    if (__any(v >= 0)) t.wmask |= 1u << k;
  }
  return t;
}

// Per-element epilogue of one 16 x 16 accumulator tile: a[r] belongs to output row rows4[r] (an LDS pointer into
// s_row; -1: no such row), column col.  Only a BF16_OUT kernel may be asked (out_bf) for a bf16 `out` and ep.residual.
template <bool BF16_OUT>
__device__ __forceinline__ void sp_epilogue_tile(f32x4 a, const int* s_row, int trow, int col, int cout,
                                                 const float* bias, const ConvEpilogue& ep,
                                                 float* out, bool out_bf) {
  const bool obf = BF16_OUT && out_bf;
  const float bv = bias ? bias[col] : 0.f;
  const float sc = ep.scale ? ep.scale[col] : 1.f;
  const float sh = ep.shift ? ep.shift[col] : 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = s_row[trow + r];
    if (row >= 0) {
      float v = a[r] + bv;
      if (ep.scale) v = v * sc + sh;                       // folded eval-mode BatchNorm
      if (ep.residual)
        v += obf ? __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(
                                       ep.residual)[(size_t)row * cout + col] << 16)
                 : ep.residual[(size_t)row * cout + col];
      if (ep.relu) v = fmaxf(v, 0.f);
      if (obf)
        reinterpret_cast<unsigned short*>(out)[(size_t)row * cout + col] =
            (unsigned short)(ud_pack_bf16x2(v, 0.f) & 0xFFFFu);
      else
        out[(size_t)row * cout + col] = v;
    }
  }
}

// LDS-staged epilogue of the all-bf16 kernels, phase 1 (per accumulator tile): bias + folded BatchNorm in registers,
// fp32 tile -> Os[kTM2][COUT_P + 4]; a[r] belongs to tile row trow + r.
template <int COUT_P>
__device__ __forceinline__ void sp_stage_out_tile(float* Os, f32x4 a, int trow, int col, int cout,
                                                  const float* bias, const ConvEpilogue& ep) {
  constexpr int LDO = COUT_P + 4;
  const bool cv = col < cout;
  const float bv = (cv && bias) ? bias[col] : 0.f;
  const float sc = (cv && ep.scale) ? ep.scale[col] : 1.f;
  const float sh = (cv && ep.shift) ? ep.shift[col] : 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) Os[(trow + r) * LDO + col] = (a[r] + bv) * sc + sh;
}

// ... and phase 2 (whole workgroup, after every tile is staged).
template <int COUT_P>
__device__ __forceinline__ void sp_store_staged_bf16(const float* Os, const int* s_row, const ConvEpilogue& ep,
                                                     unsigned short* out, int cout, int tid) {
  constexpr int LDO = COUT_P + 4;
  __syncthreads();
  // epilogue 2: + residual, ReLU, bf16, 16-byte rows
  const unsigned short* res = reinterpret_cast<const unsigned short*>(ep.residual);
  for (int u = tid; u < kTM2 * (COUT_P / 8); u += 512) {
    const int r = u / (COUT_P / 8), c8 = (u - r * (COUT_P / 8)) * 8;
    const int row = s_row[r];
    if (row < 0 || c8 >= cout) continue;
    const float4 v0 = *reinterpret_cast<const float4*>(Os + r * LDO + c8);
    const float4 v1 = *reinterpret_cast<const float4*>(Os + r * LDO + c8 + 4);
    float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    if (res) {
      const uint4 h = *reinterpret_cast<const uint4*>(res + (size_t)row * cout + c8);
      const unsigned hw[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[2 * q] += __uint_as_float(hw[q] << 16);
        v[2 * q + 1] += __uint_as_float(hw[q] & 0xFFFF0000u);
      }
    }
    if (ep.relu) {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = fmaxf(v[q], 0.f);
    }
    *reinterpret_cast<uint4*>(out + (size_t)row * cout + c8) =
        make_uint4(ud_pack_bf16x2(v[0], v[1]), ud_pack_bf16x2(v[2], v[3]), ud_pack_bf16x2(v[4], v[5]),
                   ud_pack_bf16x2(v[6], v[7]));
  }
}
#endif

}  // namespace
