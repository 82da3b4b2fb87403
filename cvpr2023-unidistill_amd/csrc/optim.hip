// Gradient-norm clip + decoupled-weight-decay AdamW over a whole parameter set in two launches.
//
// The set is cut into chunks of UD_OPTIM_CHUNK elements, each inside one tensor (host: ops/optim.py builds the table
// once per parameter set).  One workgroup per chunk, so the grid is the chunk count and nothing else.
//
// Determinism: an element's place in every sum is a function of its index inside its chunk alone (never of an
// address, of the grid or of arrival order), the squares are accumulated in fp64 (the square of an fp32 value is
// exact there), and the per-chunk partials are re-reduced by EVERY workgroup of the second launch in one fixed order:
// all workgroups derive the identical total_norm / coef / finite flag without a third launch or a grid barrier.
// No atomics anywhere.
#include "ud_common.h"
#include "ud_prof.h"
#include <math.h>

#define UD_OPTIM_CHUNK 65536
#define UD_OPTIM_THREADS 256

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Sum over the workgroup in a fixed order; every thread gets the total.  red: UD_OPTIM_THREADS / UD_WAVE doubles.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();                               // red may still be read from a previous call
  if (ud_lane() == 0) red[threadIdx.x / UD_WAVE] = v;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int w = 1; w < UD_OPTIM_THREADS / UD_WAVE; ++w) t += red[w];
  return t;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Four consecutive floats: one 16-byte access where the address allows (ALIGNED), four 4-byte ones otherwise.
template <bool ALIGNED>
__device__ __forceinline__ float4 ld4(const float* p) {
  if (ALIGNED) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
template <bool ALIGNED>
__device__ __forceinline__ void st4(float* p, const float4& v) {
  if (ALIGNED) {
    *reinterpret_cast<float4*>(p) = v;
  } else {
    p[0] = v.x;
    p[1] = v.y;
    p[2] = v.z;
    p[3] = v.w;
  }
}

// Thread t owns the float4 groups t, t + 256, ... of the chunk, and (t < len % 4) the tail element 4 * (len / 4) + t.
template <bool ALIGNED>
__device__ __forceinline__ double chunk_sqsum(const float* __restrict__ g, int len) {
  const int n4 = len >> 2;
  double ax = 0.0, ay = 0.0, az = 0.0, aw = 0.0;
  int i = threadIdx.x;
  for (; i + 3 * UD_OPTIM_THREADS < n4; i += 4 * UD_OPTIM_THREADS) {
    float4 r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = ld4<ALIGNED>(g + 4 * (size_t)(i + u * UD_OPTIM_THREADS));
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ax += (double)r[u].x * (double)r[u].x;
      ay += (double)r[u].y * (double)r[u].y;
      az += (double)r[u].z * (double)r[u].z;
      aw += (double)r[u].w * (double)r[u].w;
    }
  }
  for (; i < n4; i += UD_OPTIM_THREADS) {
    const float4 r = ld4<ALIGNED>(g + 4 * (size_t)i);
    ax += (double)r.x * (double)r.x;
    ay += (double)r.y * (double)r.y;
    az += (double)r.z * (double)r.z;
    aw += (double)r.w * (double)r.w;
  }
  double acc = (ax + ay) + (az + aw);
  const int tail = 4 * n4 + threadIdx.x;
  if (tail < len) acc += (double)g[tail] * (double)g[tail];
  return acc;
}

__global__ __launch_bounds__(UD_OPTIM_THREADS) void k_optim_sqnorm(const UdOptimChunk* __restrict__ chunks,
                                                                    const float* const* __restrict__ grads,
                                                                    double* __restrict__ partial,
                                                                    double* __restrict__ state) {
  __shared__ double red[UD_OPTIM_THREADS / UD_WAVE];
  const UdOptimChunk c = chunks[blockIdx.x];
  const float* gt = grads[c.tensor];
  if (blockIdx.x == 0 && threadIdx.x == 0) state[UD_OPTIM_ST_STEP_IN] = state[UD_OPTIM_ST_STEP];
  if (gt == nullptr) {                           // no gradient this step: nothing to the norm (uniform per workgroup)
    if (threadIdx.x == 0) partial[blockIdx.x] = 0.0;
    return;
  }
  const float* g = gt + c.offset;
  const double acc = aligned16(g) ? chunk_sqsum<true>(g, c.length) : chunk_sqsum<false>(g, c.length);
  const double tot = block_sum_f64(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

struct StepScalars {
  float coef, wd_mul, w1, beta2, omb2, step_size, bc2_sqrt, eps;
  int lerp_low;                                  // torch's lerp: a + w * (b - a) for w < 0.5, b - (b - a) * (1 - w) otherwise
  float beta1;
};

__device__ __forceinline__ void adamw_one(float& p, float& m, float& v, float g, const StepScalars& s) {
  const float gc = g * s.coef;
  p = p * s.wd_mul;
  const float d = gc - m;
  m = s.lerp_low ? m + s.w1 * d : gc - d * s.beta1;
  v = s.beta2 * v + (s.omb2 * gc) * gc;
  const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
  p = p - (s.step_size * m) / denom;
}

template <bool ALIGNED>
__device__ __forceinline__ void chunk_adamw(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                            const float* __restrict__ g, int len, const StepScalars& s) {
  const int n4 = len >> 2;
  for (int i = threadIdx.x; i < n4; i += UD_OPTIM_THREADS) {
    const size_t e = 4 * (size_t)i;
    const float4 g4 = ld4<ALIGNED>(g + e);
    float4 p4 = ld4<ALIGNED>(p + e), m4 = ld4<ALIGNED>(m + e), v4 = ld4<ALIGNED>(v + e);
    adamw_one(p4.x, m4.x, v4.x, g4.x, s);
    adamw_one(p4.y, m4.y, v4.y, g4.y, s);
    adamw_one(p4.z, m4.z, v4.z, g4.z, s);
    adamw_one(p4.w, m4.w, v4.w, g4.w, s);
    st4<ALIGNED>(p + e, p4);
    st4<ALIGNED>(m + e, m4);
    st4<ALIGNED>(v + e, v4);
  }
  const int tail = 4 * n4 + threadIdx.x;
  if (tail < len) {
    float pp = p[tail], mm = m[tail], vv = v[tail];
    adamw_one(pp, mm, vv, g[tail], s);
    p[tail] = pp;
    m[tail] = mm;
    v[tail] = vv;
  }
}

struct Hyper {
  double beta1, beta2, eps, weight_decay, max_norm;
  int skip_nonfinite;
};

__global__ __launch_bounds__(UD_OPTIM_THREADS) void k_optim_clip_adamw(
    const UdOptimChunk* __restrict__ chunks, int n_chunks, float* const* __restrict__ params,
    float* const* __restrict__ exp_avg, float* const* __restrict__ exp_avg_sq, const float* const* __restrict__ grads,
    const double* __restrict__ partial, double* __restrict__ state, const Hyper h) {
  __shared__ double red[UD_OPTIM_THREADS / UD_WAVE];
  __shared__ StepScalars sh;
  __shared__ int sh_skip;
  // the same total in every workgroup: thread t takes partials t, t + 256, ... in order, then the fixed block sum
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_chunks; i += UD_OPTIM_THREADS) acc += partial[i];
  const double sum = block_sum_f64(acc, red);
  if (threadIdx.x == 0) {
    const float total_norm = (float)sqrt(sum);
    const bool finite = isfinite(total_norm);
    // clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1.0, all in fp32
    float coef = (1.0f / (total_norm + 1e-6f)) * (float)h.max_norm;
    coef = coef > 1.0f ? 1.0f : coef;            // NaN stays NaN (torch.clamp keeps it too)
    const int skip = h.skip_nonfinite && !finite;
    const double lr = state[UD_OPTIM_ST_LR];
    const double step = state[UD_OPTIM_ST_STEP_IN] + 1.0;
    const double bc1 = 1.0 - pow(h.beta1, step);
    const double bc2 = 1.0 - pow(h.beta2, step);
    sh.coef = coef;
    sh.wd_mul = (float)(1.0 - lr * h.weight_decay);
    sh.w1 = (float)(1.0 - h.beta1);
    sh.beta1 = (float)h.beta1;
    sh.lerp_low = (1.0 - h.beta1) < 0.5;
    sh.beta2 = (float)h.beta2;
    sh.omb2 = (float)(1.0 - h.beta2);
    sh.step_size = (float)(lr / bc1);
    sh.bc2_sqrt = (float)sqrt(bc2);
    sh.eps = (float)h.eps;
    sh_skip = skip;
    if (blockIdx.x == 0) {                       // the state block has one writer; plain (vector) stores
      state[UD_OPTIM_ST_NORM] = (double)total_norm;
      state[UD_OPTIM_ST_COEF] = (double)coef;
      state[UD_OPTIM_ST_FINITE] = finite ? 1.0 : 0.0;
      if (skip)
        state[UD_OPTIM_ST_SKIPPED] = state[UD_OPTIM_ST_SKIPPED] + 1.0;
      else
        state[UD_OPTIM_ST_STEP] = step;
    }
  }
  __syncthreads();
  if (sh_skip) return;                           // guard: no workgroup touches p, m or v
  const UdOptimChunk c = chunks[blockIdx.x];
  const float* gt = grads[c.tensor];
  if (gt == nullptr) return;                     // a parameter without a gradient is left alone, as torch does
  const StepScalars s = sh;
  float* p = params[c.tensor] + c.offset;
  float* m = exp_avg[c.tensor] + c.offset;
  float* v = exp_avg_sq[c.tensor] + c.offset;
  const float* g = gt + c.offset;
  if (aligned16(p) && aligned16(m) && aligned16(v) && aligned16(g))
    chunk_adamw<true>(p, m, v, g, c.length, s);
  else
    chunk_adamw<false>(p, m, v, g, c.length, s);
}

}  // namespace

extern "C" int ud_optim_chunk_elems(void) { return UD_OPTIM_CHUNK; }

extern "C" int ud_optim_sqnorm(const UdOptimChunk* chunks, int n_chunks, const float* const* grads, double* partial,
                               double* state, ud_stream_t stream_) {
  if (n_chunks < 0 || (n_chunks > 0 && (!chunks || !grads || !partial)) || !state) return UD_ERR_INVALID_ARG;
  if (n_chunks == 0) return UD_OK;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("optim.k_sqnorm", stream);
  k_optim_sqnorm<<<n_chunks, UD_OPTIM_THREADS, 0, stream>>>(chunks, grads, partial, state);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

extern "C" int ud_optim_clip_adamw(const UdOptimChunk* chunks, int n_chunks, float* const* params,
                                   float* const* exp_avg, float* const* exp_avg_sq, const float* const* grads,
                                   const double* partial, double* state, double beta1, double beta2, double eps,
                                   double weight_decay, double max_norm, int skip_nonfinite, ud_stream_t stream_) {
  if (n_chunks < 0 || (n_chunks > 0 && (!chunks || !params || !exp_avg || !exp_avg_sq || !grads || !partial)) || !state)
    return UD_ERR_INVALID_ARG;
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(max_norm > 0.0))
    return UD_ERR_INVALID_ARG;
  if (n_chunks == 0) return UD_OK;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("optim.k_clip_adamw", stream);
  const Hyper h = {beta1, beta2, eps, weight_decay, max_norm, skip_nonfinite != 0};
  k_optim_clip_adamw<<<n_chunks, UD_OPTIM_THREADS, 0, stream>>>(chunks, n_chunks, params, exp_avg, exp_avg_sq, grads,
                                                               partial, state, h);
  UD_LAUNCH_CHECK();
  return UD_OK;
}
