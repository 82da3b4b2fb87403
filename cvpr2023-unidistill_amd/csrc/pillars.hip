// PointPillars LiDAR encoder: PillarVFE (feature augmentation + ONE PFNLayer: Linear, BatchNorm1d, ReLU, max over the rows)
// and PointPillarScatter in one pass over the voxelizer's [M, P, F] rows.
//
// Shape of every pass: a workgroup of C / 64 waves walks a contiguous chunk of pillars; wave s owns the channels
// 64 s .. 64 s + 63, one per lane, and keeps that channel's K weights (padded to a multiple of 4 with zeros) in registers.  A
// pillar's num x K row features are built once per wave (lane = row) in the wave's own LDS region and read back as broadcast
// float4s, so a wave never waits for another.  z = w . f is a sequential sum over k from 0.f (mul, add: -ffp-contract=off),
// the same in every pass: the backward recomputes the very bits the forward saw.  Padded rows (row >= num) have a zero
// feature row, so z = 0 there: they are not computed, their share of every sum is added in closed form.
// All sums over pillars are per-workgroup partial rows in ascending pillar order, then one of ud_reduce.h's finalize kernels.
#include "ud_common.h"
#include "ud_reduce.h"

namespace {

constexpr int kPMax = 64;        // rows per pillar: a lane per row while staging
constexpr int kStatGroups = 2048;  // partial rows of the channel sums
constexpr int kDwGroups = 512;     // partial rows of the weight gradient (C * K floats each)

struct PillarArgs {
  const float* voxels;
  const int32_t* coords;
  const int32_t* num;
  const float* weight;
  int M, P, F, C, K;
  int per;             // pillars per workgroup
  unsigned flags;
  float vx, vy, vz, ox, oy, oz;
};

// Row features of pillar m -> f[row][4 * KQ] for row < n (n = num[m] clamped to [0, P]); returns n in every lane.
template <int KQ>
__device__ __forceinline__ int stage_rows(const PillarArgs& a, int m, float (*f)[4 * KQ]) {
  const int lane = ud_lane();
  const int n = min(max(a.num[m], 0), a.P);
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = 0.f;
  if (lane < a.P) {
    const float* row = a.voxels + ((size_t)m * a.P + lane) * a.F;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < a.F) r[j] = row[j];
  }
  // the mean divides the sum over ALL P rows (padded rows are zero by the voxelizer's contract) by num, as the reference does
  const float nf = (float)a.num[m];
  const float mx = ud_wave_sum(r[0]) / nf, my = ud_wave_sum(r[1]) / nf, mz = ud_wave_sum(r[2]) / nf;
  const int4 c = *reinterpret_cast<const int4*>(a.coords + (size_t)m * 4);
  const float cx = (float)c.w * a.vx + a.ox, cy = (float)c.z * a.vy + a.oy, cz = (float)c.y * a.vz + a.oz;
  if (lane < n) {
    float* o = f[lane];
    int k = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < a.F && ((a.flags & UD_PILLAR_ABS_XYZ) || j >= 3)) o[k++] = r[j];
    o[k++] = r[0] - mx;
    o[k++] = r[1] - my;
    o[k++] = r[2] - mz;
    o[k++] = r[0] - cx;
    o[k++] = r[1] - cy;
    o[k++] = r[2] - cz;
    if (a.flags & UD_PILLAR_DISTANCE) o[k++] = sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (; k < 4 * KQ; ++k) o[k] = 0.f;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes have landed
  return n;
}

template <int KQ>
__device__ __forceinline__ void load_weights(const PillarArgs& a, int ch, float* w) {
#pragma unroll
  for (int k = 0; k < 4 * KQ; ++k) w[k] = (ch < a.C && k < a.K) ? a.weight[(size_t)ch * a.K + k] : 0.f;
}

// z of one staged row: sequential over k, from 0.f
template <int KQ>
__device__ __forceinline__ float row_dot(const float* w, const float* frow, float* fout = nullptr) {
  float z = 0.f;
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    const float4 v = *reinterpret_cast<const float4*>(frow + 4 * q);
    z += w[4 * q] * v.x;
    z += w[4 * q + 1] * v.y;
    z += w[4 * q + 2] * v.z;
    z += w[4 * q + 3] * v.w;
    if (fout) { fout[4 * q] = v.x; fout[4 * q + 1] = v.y; fout[4 * q + 2] = v.z; fout[4 * q + 3] = v.w; }
  }
  return z;
}

#define PILLAR_PROLOGUE()                                                              \
  __shared__ float s_f[4][kPMax][4 * KQ];                                              \
  const int wv = threadIdx.x >> 6, lane = ud_lane(), ch = wv * 64 + lane;              \
  float(*f)[4 * KQ] = s_f[wv];                                                         \
  float w[4 * KQ];                                                                     \
  load_weights<KQ>(a, ch, w);                                                          \
  const int m0 = blockIdx.x * a.per, m1 = min(a.M, m0 + a.per);                        \
  const bool live = ch < a.C

// partial[group][0 .. C) = sum z, partial[group][C .. 2C) = sum z * z over the group's real rows
template <int KQ>
__global__ __launch_bounds__(256) void k_pillar_stats(PillarArgs a, float* __restrict__ partial) {
  PILLAR_PROLOGUE();
  float s = 0.f, q = 0.f;
  for (int m = m0; m < m1; ++m) {
    const int n = stage_rows<KQ>(a, m, f);
    for (int p = 0; p < n; ++p) {
      const float z = row_dot<KQ>(w, f[p]);
      s += z;
      q += z * z;
    }
    __builtin_amdgcn_wave_barrier();   // the next pillar's rows overwrite these
  }
  if (live) {
    partial[(size_t)blockIdx.x * 2 * a.C + ch] = s;
    partial[(size_t)blockIdx.x * 2 * a.C + a.C + ch] = q;
  }
}

// sums f32[2C] -> stats[4][C] = mean, invstd, scale, shift; running statistics as torch's BatchNorm1d updates them
__global__ void k_pillar_bn_final(const float* __restrict__ sums, int C, long long n, const float* __restrict__ gamma,
                                  const float* __restrict__ beta, float eps, float momentum, float* __restrict__ running_mean,
                                  float* __restrict__ running_var, float* __restrict__ stats) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double mean = (double)sums[c] / (double)n;
  double var = (double)sums[C + c] / (double)n - mean * mean;
  var = var > 0.0 ? var : 0.0;
  const float meanf = (float)mean, invstd = (float)(1.0 / sqrt(var + (double)eps));
  const float scale = gamma[c] * invstd;
  stats[c] = meanf;
  stats[C + c] = invstd;
  stats[2 * C + c] = scale;
  stats[3 * C + c] = beta[c] - meanf * scale;
  if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * meanf;
  if (running_var) {
    const float unbiased = (float)(n > 1 ? var * ((double)n / (double)(n - 1)) : var);
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
  }
}

template <int KQ>
__global__ __launch_bounds__(256) void k_pillar_apply(PillarArgs a, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, int B, int ny, int nx,
                                                      float* __restrict__ bev, float* __restrict__ pillars,
                                                      uint8_t* __restrict__ argmax) {
  PILLAR_PROLOGUE();
  const float sc = live ? scale[ch] : 0.f, sh = live ? shift[ch] : 0.f;
  const float pad = fmaxf(sh, 0.f);          // a padded row: z = 0
  for (int m = m0; m < m1; ++m) {
    const int n = stage_rows<KQ>(a, m, f);
    float best = -1.f;
    int arg = 0;
    for (int p = 0; p < n; ++p) {
      const float y = fmaxf(row_dot<KQ>(w, f[p]) * sc + sh, 0.f);
      if (y > best) { best = y; arg = p; }
    }
    if (n < a.P && pad > best) { best = pad; arg = n; }
    __builtin_amdgcn_wave_barrier();
    if (!live) continue;
    const int4 c = *reinterpret_cast<const int4*>(a.coords + (size_t)m * 4);
    if ((unsigned)c.x < (unsigned)B && (unsigned)c.z < (unsigned)ny && (unsigned)c.w < (unsigned)nx)
      bev[(((size_t)c.x * ny + c.z) * nx + c.w) * a.C + ch] = best;
    if (pillars) pillars[(size_t)m * a.C + ch] = best;
    if (argmax) argmax[(size_t)m * a.C + ch] = (uint8_t)arg;
  }
}

// masked upstream gradient of (pillar m, this lane's channel) and z of its argmax row
template <int KQ>
__device__ __forceinline__ float masked_dy(const PillarArgs& a, int m, int n, int arg, const float* w, float (*f)[4 * KQ],
                                           float sc, float sh, const float* __restrict__ dbev,
                                           const float* __restrict__ dpil, int B, int ny, int nx, int ch, float& zsel,
                                           float* fsel) {
  zsel = 0.f;
#pragma unroll
  for (int k = 0; k < 4 * KQ; ++k) fsel[k] = 0.f;
  if (arg < n) zsel = row_dot<KQ>(w, f[arg], fsel);      // a lane-own row; padded rows: z = 0, zero features
  const int4 c = *reinterpret_cast<const int4*>(a.coords + (size_t)m * 4);
  float dy = 0.f;
  if ((unsigned)c.x < (unsigned)B && (unsigned)c.z < (unsigned)ny && (unsigned)c.w < (unsigned)nx)
    dy = dbev[(((size_t)c.x * ny + c.z) * nx + c.w) * a.C + ch];
  if (dpil) dy += dpil[(size_t)m * a.C + ch];          // a consumer of the [M, C] features themselves
  return zsel * sc + sh > 0.f ? dy : 0.f;               // the forward's own bits: the ReLU mask of the winning row
}

// partial[group][c] = (sum g, sum g * (z - mean)) over the argmax rows: every other row has a zero upstream gradient
template <int KQ>
__global__ __launch_bounds__(256) void k_pillar_bwd_reduce(PillarArgs a, const float* __restrict__ dbev,
                                                           const float* __restrict__ dpil, int B, int ny, int nx,
                                                           const uint8_t* __restrict__ argmax, const float* __restrict__ stats,
                                                           float* __restrict__ partial) {
  PILLAR_PROLOGUE();
  const float mean = live ? stats[ch] : 0.f, sc = live ? stats[2 * a.C + ch] : 0.f, sh = live ? stats[3 * a.C + ch] : 0.f;
  float s = 0.f, q = 0.f;
  float fsel[4 * KQ];
  for (int m = m0; m < m1; ++m) {
    const int n = stage_rows<KQ>(a, m, f);
    if (live) {
      float zsel;
      const float g = masked_dy<KQ>(a, m, n, argmax[(size_t)m * a.C + ch], w, f, sc, sh, dbev, dpil, B, ny, nx, ch, zsel, fsel);
      s += g;
      q += g * (zsel - mean);
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (live) *reinterpret_cast<float2*>(partial + ((size_t)blockIdx.x * a.C + ch) * 2) = make_float2(s, q);
}

// partial[group][c][k] = sum over the group's rows of dz * f[k];  dz = scale * g (argmax row) + k2 * z + k0 (every row; not FROZEN)
template <int KQ, bool FROZEN>
__global__ __launch_bounds__(256) void k_pillar_bwd_dw(PillarArgs a, const float* __restrict__ dbev,
                                                       const float* __restrict__ dpil, int B, int ny, int nx,
                                                       const uint8_t* __restrict__ argmax, const float* __restrict__ stats,
                                                       const float* __restrict__ k0v, const float* __restrict__ k2v,
                                                       float* __restrict__ partial) {
  PILLAR_PROLOGUE();
  const float sc = live ? stats[2 * a.C + ch] : 0.f, sh = live ? stats[3 * a.C + ch] : 0.f;
  const float k0 = (!FROZEN && live) ? k0v[ch] : 0.f, k2 = (!FROZEN && live) ? k2v[ch] : 0.f;
  float acc[4 * KQ], fsel[4 * KQ];
#pragma unroll
  for (int k = 0; k < 4 * KQ; ++k) acc[k] = 0.f;
  for (int m = m0; m < m1; ++m) {
    const int n = stage_rows<KQ>(a, m, f);
    if (live) {
      float zsel;
      const float g = masked_dy<KQ>(a, m, n, argmax[(size_t)m * a.C + ch], w, f, sc, sh, dbev, dpil, B, ny, nx, ch, zsel, fsel);
      const float dsel = sc * g;
#pragma unroll
      for (int k = 0; k < 4 * KQ; ++k) acc[k] += dsel * fsel[k];
    }
    if (!FROZEN) {
      for (int p = 0; p < n; ++p) {
        float fr[4 * KQ];
        const float z = row_dot<KQ>(w, f[p], fr);
        const float dz = k2 * z + k0;
#pragma unroll
        for (int k = 0; k < 4 * KQ; ++k) acc[k] += dz * fr[k];
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (live) {
    float* o = partial + ((size_t)blockIdx.x * a.C + ch) * a.K;
#pragma unroll
    for (int k = 0; k < 4 * KQ; ++k)
      if (k < a.K) o[k] = acc[k];
  }
}

int feature_count(int F, unsigned flags) {
  return ((flags & UD_PILLAR_ABS_XYZ) ? F : F - 3) + 6 + ((flags & UD_PILLAR_DISTANCE) ? 1 : 0);
}

bool sizes_ok(int M, int P, int F, int C, unsigned flags) {
  if (M <= 0 || P <= 0 || P > kPMax || F < 3 || F > 8 || C <= 0 || C > 256 || C % 32 != 0) return false;
  if (flags & ~(UD_PILLAR_ABS_XYZ | UD_PILLAR_DISTANCE)) return false;
  return (long long)M * P * F < (1ll << 31) && (long long)M * C < (1ll << 31);
}

int groups_of(int M, int cap) { return M < cap ? M : cap; }

struct PillarScratch {
  float *stat_partial, *sums, *red_partial, *k0, *k2, *dgamma, *dbeta, *dw_partial;
  size_t bytes;
};

PillarScratch carve(void* ws, int M, int C, int K) {
  UdArena ar(ws, (size_t)-1);
  PillarScratch s;
  const int gs = groups_of(M, kStatGroups), gd = groups_of(M, kDwGroups);
  s.stat_partial = ar.take<float>((size_t)gs * 2 * C);
  s.sums = ar.take<float>(2 * C);
  s.red_partial = ar.take<float>((size_t)gs * 2 * C);
  s.k0 = ar.take<float>(C);
  s.k2 = ar.take<float>(C);
  s.dgamma = ar.take<float>(C);
  s.dbeta = ar.take<float>(C);
  s.dw_partial = ar.take<float>((size_t)gd * C * K);
  s.bytes = ar.used;
  return s;
}

int make_args(PillarArgs& a, const float* voxels, const int32_t* coords, const int32_t* num, int M, int P, int F,
              const float* weight, int C, unsigned flags, const float* geom, int groups) {
  if (!sizes_ok(M, P, F, C, flags)) return UD_ERR_UNSUPPORTED;
  if (!voxels || !coords || !num || !weight || !geom) return UD_ERR_INVALID_ARG;
  a.voxels = voxels; a.coords = coords; a.num = num; a.weight = weight;
  a.M = M; a.P = P; a.F = F; a.C = C; a.K = feature_count(F, flags);
  a.flags = flags;
  a.per = ud_div_up(M, groups);
  a.vx = geom[0]; a.vy = geom[1]; a.vz = geom[2]; a.ox = geom[3]; a.oy = geom[4]; a.oz = geom[5];
  return UD_OK;
}

// KQ = float4s per feature row: K in 6 .. 15 -> 2, 3 or 4
#define PILLAR_DISPATCH(K, CALL)                       \
  do {                                                 \
    if ((K) <= 8) { constexpr int KQ = 2; CALL; }      \
    else if ((K) <= 12) { constexpr int KQ = 3; CALL; } \
    else { constexpr int KQ = 4; CALL; }               \
  } while (0)

}  // namespace

extern "C" size_t ud_pillar_workspace_bytes(int M, int P, int F, int C, unsigned flags) {
  if (!sizes_ok(M, P, F, C, flags)) return 0;
  return carve(nullptr, M, C, feature_count(F, flags)).bytes;
}

extern "C" int ud_pillar_stats(const float* voxels, const int32_t* coords, const int32_t* num, int M, int P, int F,
                               const float* weight, int C, unsigned flags, const float* geom, const float* gamma,
                               const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                               float* stats, void* workspace, size_t workspace_bytes, ud_stream_t stream_) {
  const int groups = groups_of(M, kStatGroups);
  PillarArgs a;
  if (const int e = make_args(a, voxels, coords, num, M, P, F, weight, C, flags, geom, groups)) return e;
  if (!gamma || !beta || !stats) return UD_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < ud_pillar_workspace_bytes(M, P, F, C, flags)) return UD_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const PillarScratch s = carve(workspace, M, C, a.K);
  const int blocks = ud_div_up(M, a.per), threads = 64 * ud_div_up(C, 64);
  PILLAR_DISPATCH(a.K, (k_pillar_stats<KQ><<<blocks, threads, 0, stream>>>(a, s.stat_partial)));
  UD_LAUNCH_CHECK();
  if (const int e = ud_colsum_final(s.stat_partial, blocks, 2 * C, s.sums, stream)) return e;
  k_pillar_bn_final<<<ud_div_up(C, 64), 64, 0, stream>>>(s.sums, C, (long long)M * P, gamma, beta, eps, momentum, running_mean,
                                                         running_var, stats);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

extern "C" int ud_pillar_apply(const float* voxels, const int32_t* coords, const int32_t* num, int M, int P, int F,
                               const float* weight, int C, unsigned flags, const float* geom, const float* scale,
                               const float* shift, int B, int ny, int nx, float* bev, float* pillars, uint8_t* argmax,
                               ud_stream_t stream_) {
  const int groups = groups_of(M, 8 * kStatGroups);
  PillarArgs a;
  if (const int e = make_args(a, voxels, coords, num, M, P, F, weight, C, flags, geom, groups)) return e;
  if (!scale || !shift || !bev || B <= 0 || ny <= 0 || nx <= 0) return UD_ERR_INVALID_ARG;
  if ((long long)B * ny * nx * C >= (1ll << 40)) return UD_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  ud_zero_f32_async(bev, (size_t)B * ny * nx * C, stream);
  UD_LAUNCH_CHECK();
  const int blocks = ud_div_up(M, a.per), threads = 64 * ud_div_up(C, 64);
  PILLAR_DISPATCH(a.K, (k_pillar_apply<KQ><<<blocks, threads, 0, stream>>>(a, scale, shift, B, ny, nx, bev, pillars, argmax)));
  UD_LAUNCH_CHECK();
  return UD_OK;
}

extern "C" int ud_pillar_bwd(const float* voxels, const int32_t* coords, const int32_t* num, int M, int P, int F,
                             const float* weight, int C, unsigned flags, const float* geom, const float* dbev,
                             const float* dpillars, int B, int ny, int nx, const uint8_t* argmax, const float* stats,
                             int frozen, float* dweight, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, ud_stream_t stream_) {
  const int gs = groups_of(M, kStatGroups), gd = groups_of(M, kDwGroups);
  PillarArgs a;
  if (const int e = make_args(a, voxels, coords, num, M, P, F, weight, C, flags, geom, gs)) return e;
  if (!dbev || !argmax || !stats || B <= 0 || ny <= 0 || nx <= 0) return UD_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < ud_pillar_workspace_bytes(M, P, F, C, flags)) return UD_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const PillarScratch s = carve(workspace, M, C, a.K);
  const int threads = 64 * ud_div_up(C, 64);
  const bool affine = dgamma || dbeta;
  if (!frozen || affine) {
    // sum g and sum g * (z - mean) over the argmax rows -> dgamma, dbeta, and the constants of dz = scale * g + k2 * z + k0
    const int blocks = ud_div_up(M, a.per);
    PILLAR_DISPATCH(a.K, (k_pillar_bwd_reduce<KQ><<<blocks, threads, 0, stream>>>(a, dbev, dpillars, B, ny, nx, argmax, stats,
                                                                                  s.red_partial)));
    UD_LAUNCH_CHECK();
    if (const int e = ud_bn_bwd_final(s.red_partial, blocks, C, (long long)M * P, stats + 2 * C, stats, stats + C,
                                      dgamma ? dgamma : s.dgamma, dbeta ? dbeta : s.dbeta, s.k0, s.k2, stream))
      return e;
  }
  if (dweight) {
    a.per = ud_div_up(M, gd);
    const int blocks = ud_div_up(M, a.per);
    if (frozen)
      PILLAR_DISPATCH(a.K, (k_pillar_bwd_dw<KQ, true><<<blocks, threads, 0, stream>>>(a, dbev, dpillars, B, ny, nx, argmax, stats, nullptr,
                                                                                      nullptr, s.dw_partial)));
    else
      PILLAR_DISPATCH(a.K, (k_pillar_bwd_dw<KQ, false><<<blocks, threads, 0, stream>>>(a, dbev, dpillars, B, ny, nx, argmax, stats, s.k0,
                                                                                       s.k2, s.dw_partial)));
    UD_LAUNCH_CHECK();
    if (const int e = ud_wgrad_sum(s.dw_partial, blocks, (size_t)C * a.K, dweight, stream)) return e;
  }
  return UD_OK;
}
