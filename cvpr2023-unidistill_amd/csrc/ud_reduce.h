// The second half of the library's deterministic split reductions: a pass writes per-slice partial sums, one of these kernels adds
// them in a fixed order (no atomics).  Each kernel once, its launcher beside it; every includer gets its own copy (anonymous namespace).
#ifndef UD_REDUCE_H_
#define UD_REDUCE_H_
#include "ud_common.h"

namespace {

// out[i] = sum over slices of partial[s][i], i in float4 units: a workgroup owns 64 float4 outputs, its four
// waves each add a quarter of the slices (ascending), the four sub-sums are combined in wave order.
// Order: four ascending quarter sums, then the quarters -- the weight gradients of conv2d.hip and conv2d_f32_wgrad.hip.
__global__ __launch_bounds__(256) void k_wgrad_sum(const float* __restrict__ partial, int slices, size_t n,
                                                   float* __restrict__ out) {
  __shared__ float4 part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t i4 = (size_t)blockIdx.x * 64 + lane, n4 = n / 4;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i4 < n4) {
    const int per = (slices + 3) / 4, s0 = wave * per, s1 = min(slices, s0 + per);
    auto ld = [&](int s) { return *reinterpret_cast<const float4*>(partial + (size_t)s * n + 4 * i4); };
    int s = s0;
    for (; s + 3 < s1; s += 4) {          // four loads in flight per trip; the additions keep the ascending order
      const float4 v0 = ld(s), v1 = ld(s + 1), v2 = ld(s + 2), v3 = ld(s + 3);
      a.x += v0.x; a.y += v0.y; a.z += v0.z; a.w += v0.w;
      a.x += v1.x; a.y += v1.y; a.z += v1.z; a.w += v1.w;
      a.x += v2.x; a.y += v2.y; a.z += v2.z; a.w += v2.w;
      a.x += v3.x; a.y += v3.y; a.z += v3.z; a.w += v3.w;
    }
    for (; s < s1; ++s) {
      const float4 v = ld(s);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
  }
  part[wave][lane] = a;
  __syncthreads();
  if (wave == 0 && i4 < n4) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float4 v = part[w][lane];
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    *reinterpret_cast<float4*>(out + 4 * i4) = a;
  }
}

// n % 4 == 0
inline int ud_wgrad_sum(const float* partial, int slices, size_t n, float* out, hipStream_t stream) {
  k_wgrad_sum<<<ud_div_up((long long)(n / 4), 64), 256, 0, stream>>>(partial, slices, n, out);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

// out[i] = sum over slices of partial[s][i], a thread per output.
// Order: one ascending sum from 0.f -- the tail weight gradients of head_tail.hip and head_tail_f32.hip (a few dozen slices).
__global__ void k_slice_sum(const float* __restrict__ partial, int slices, size_t n, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float a = 0.f;
  for (int s = 0; s < slices; ++s) a += partial[(size_t)s * n + i];
  out[i] = a;
}

inline int ud_slice_sum(const float* partial, int slices, size_t n, float* out, hipStream_t stream) {
  k_slice_sum<<<ud_div_up((long long)n, 256), 256, 0, stream>>>(partial, slices, n, out);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

// BatchNorm backward, second half: partial[slice][c] = (sum dr, sum dr * (x - mean)) -> dbeta, dgamma and the per-channel
// constants of dx = scale * dr + k2 * x + k0.
// One workgroup of T threads per channel; every thread adds rows t, t + T, ... with FOUR independent loads in flight, then a fixed
// tree.  (Rounds 2-5: one wave per channel walking up to 1 024 partial rows in 16 dependent trips -- 3 us on an idle chip, 26 us
// on average inside the step, where every trip waits behind the other streams' memory traffic: 71 of them sit on the main
// stream's backward chain between a layer's reduction pass and its dx pass.)
template <int T>
__global__ __launch_bounds__(T) void k_bn_bwd_final(const float* __restrict__ partial, int slices, int C, long long P,
                                                    const float* __restrict__ scale, const float* __restrict__ mean,
                                                    const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                    float* __restrict__ dbeta, float* __restrict__ k0, float* __restrict__ k2) {
  __shared__ float red[T / 64][2];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  auto ld = [&](int s) { return *reinterpret_cast<const float2*>(partial + ((size_t)s * C + c) * 2); };
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
  int s = tid;
  for (; s + 3 * T < slices; s += 4 * T) {
    const float2 v0 = ld(s), v1 = ld(s + T), v2 = ld(s + 2 * T), v3 = ld(s + 3 * T);
    a0 += v0.x; q0 += v0.y;
    a1 += v1.x; q1 += v1.y;
    a2 += v2.x; q2 += v2.y;
    a3 += v3.x; q3 += v3.y;
  }
  for (; s < slices; s += T) {
    const float2 v = ld(s);
    a0 += v.x; q0 += v.y;
  }
  float a = (a0 + a1) + (a2 + a3), q = (q0 + q1) + (q2 + q3);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o);
    q += __shfl_xor(q, o);
  }
  if (T > 64) {
    if (lane == 0) { red[wv][0] = a; red[wv][1] = q; }
    __syncthreads();
    if (tid == 0) {
      a = red[0][0], q = red[0][1];
#pragma unroll
      for (int w = 1; w < T / 64; ++w) { a += red[w][0]; q += red[w][1]; }
    }
  }
  if (tid != 0) return;
  const float is = invstd[c], dg = q * is, inv_p = 1.0f / (float)P;
  dbeta[c] = a;
  dgamma[c] = dg;
  const float kk2 = -scale[c] * (dg * inv_p) * is;
  k2[c] = kk2;
  k0[c] = -scale[c] * (a * inv_p) - kk2 * mean[c];
}

// four waves per channel above 128 slices, one below: the width is part of the summation order
inline int ud_bn_bwd_final(const float* partial, int slices, int C, long long P, const float* scale, const float* mean,
                           const float* invstd, float* dgamma, float* dbeta, float* k0, float* k2, hipStream_t stream) {
  if (slices > 128)
    k_bn_bwd_final<256><<<C, 256, 0, stream>>>(partial, slices, C, P, scale, mean, invstd, dgamma, dbeta, k0, k2);
  else
    k_bn_bwd_final<64><<<C, 64, 0, stream>>>(partial, slices, C, P, scale, mean, invstd, dgamma, dbeta, k0, k2);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

// Sum over the slices of partial[slice][c] by a workgroup of T threads, in V: thread t adds slices t, t + T, ... with four
// independent loads in flight, then a fixed tree.  The total is valid on thread 0; red holds T / 64 values.
template <int T, typename V>
__device__ __forceinline__ V ud_colsum_block(const V* __restrict__ partial, int slices, int C, int c, V* __restrict__ red) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;      // T threads per channel, fixed-order reduction
  V a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  int s = tid;
  for (; s + 3 * T < slices; s += 4 * T) {
    const V v0 = partial[(size_t)s * C + c], v1 = partial[(size_t)(s + T) * C + c], v2 = partial[(size_t)(s + 2 * T) * C + c],
            v3 = partial[(size_t)(s + 3 * T) * C + c];
    a0 += v0; a1 += v1; a2 += v2; a3 += v3;
  }
  for (; s < slices; s += T) a0 += partial[(size_t)s * C + c];
  V a = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
  if (T > 64) {
    if (lane == 0) red[wv] = a;
    __syncthreads();
    if (tid == 0) {
      a = red[0];
#pragma unroll
      for (int w = 1; w < T / 64; ++w) a += red[w];
    }
  }
  return a;
}

// out[c] = sum over the slices of partial[slice][c]
template <int T>
__global__ __launch_bounds__(T) void k_colsum_final(const float* __restrict__ partial, int slices, int C, float* __restrict__ out) {
  __shared__ float red[T / 64];
  const float a = ud_colsum_block<T, float>(partial, slices, C, blockIdx.x, red);
  if (threadIdx.x == 0) out[blockIdx.x] = a;
}

inline int ud_colsum_final(const float* partial, int slices, int C, float* out, hipStream_t stream) {
  if (slices > 128) k_colsum_final<256><<<C, 256, 0, stream>>>(partial, slices, C, out);
  else k_colsum_final<64><<<C, 64, 0, stream>>>(partial, slices, C, out);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

// out[g][c] += sum over the slices of partial[g][slice][c], in fp64 and in k_colsum_final's order: `groups` independent column
// sums in one launch (blockIdx.y), added to what out already holds -- a running total kept on the device (the depth metric of
// depth_metric.hip).
template <int T>
__global__ __launch_bounds__(T) void k_colsum_accum_f64(const double* __restrict__ partial, int slices, int C,
                                                        double* __restrict__ out) {
  __shared__ double red[T / 64];
  const int c = blockIdx.x, g = blockIdx.y;
  const double a = ud_colsum_block<T, double>(partial + (size_t)g * slices * C, slices, C, c, red);
  if (threadIdx.x == 0) out[(size_t)g * C + c] += a;
}

inline int ud_colsum_accum_f64(const double* partial, int groups, int slices, int C, double* out, hipStream_t stream) {
  if (slices > 128) k_colsum_accum_f64<256><<<dim3(C, groups), 256, 0, stream>>>(partial, slices, C, out);
  else k_colsum_accum_f64<64><<<dim3(C, groups), 64, 0, stream>>>(partial, slices, C, out);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

// partial[slice] = (sum, count) -> out = (sum / max(1, count), count): a masked mean whose divisor is this call's own count.
// One workgroup; thread t adds slices t, t + 256, ... in fp64, then a fixed tree, one division, one rounding to fp32: the
// scalar does not depend on how many slices the pass was cut into beyond the roundings of the partials themselves
// (the depth-supervision loss of depth_sup.hip).
__global__ __launch_bounds__(256) void k_mean_final(const float* __restrict__ partial, int slices, float* __restrict__ out) {
  __shared__ double red[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double a = 0.0, n = 0.0;
  for (int s = tid; s < slices; s += 256) {
    const float2 v = *reinterpret_cast<const float2*>(partial + (size_t)s * 2);
    a += (double)v.x;
    n += (double)v.y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o);
    n += __shfl_xor(n, o);
  }
  if (lane == 0) { red[wv][0] = a; red[wv][1] = n; }
  __syncthreads();
  if (tid != 0) return;
  a = red[0][0], n = red[0][1];
#pragma unroll
  for (int w = 1; w < 4; ++w) { a += red[w][0]; n += red[w][1]; }
  out[0] = (float)(a / (n < 1.0 ? 1.0 : n));
  out[1] = (float)n;
}

inline int ud_mean_final(const float* partial, int slices, float* out, hipStream_t stream) {
  k_mean_final<<<1, 256, 0, stream>>>(partial, slices, out);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

}  // namespace
#endif  // UD_REDUCE_H_
