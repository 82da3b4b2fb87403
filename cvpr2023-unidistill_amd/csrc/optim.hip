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
//
// Optional weight EMA (ud_optim_clip_adamw_ema): the update kernel carries a fifth stream e and, with the fresh p still in
// a register, does e = lerp(e, p, w).  w comes from the same device-side step count as the bias corrections, so a step the
// guard skips neither moves e nor advances a warm-up ramp.  ud_optim_swap exchanges two rows of tensors over the same table.
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
  float ema_w, ema_omw;                          // EMA: e = lerp(e, p, ema_w); ema_omw = 1 - ema_w in fp32, as torch forms it
  int ema_low;
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

// torch's lerp(e, p, w), with p the value about to be stored
__device__ __forceinline__ void ema_one(float& e, float p, const StepScalars& s) {
  const float d = p - e;
  e = s.ema_low ? e + s.ema_w * d : p - d * s.ema_omw;
}

// ea: the chunk's EMA stream (EMA only; otherwise never dereferenced)
template <bool ALIGNED, bool EMA>
__device__ __forceinline__ void chunk_adamw(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                            float* __restrict__ ea, const float* __restrict__ g, int len,
                                            const StepScalars& s) {
  const int n4 = len >> 2;
  for (int i = threadIdx.x; i < n4; i += UD_OPTIM_THREADS) {
    const size_t e = 4 * (size_t)i;
    const float4 g4 = ld4<ALIGNED>(g + e);
    float4 p4 = ld4<ALIGNED>(p + e), m4 = ld4<ALIGNED>(m + e), v4 = ld4<ALIGNED>(v + e);
    float4 e4;
    if (EMA) e4 = ld4<ALIGNED>(ea + e);
    adamw_one(p4.x, m4.x, v4.x, g4.x, s);
    adamw_one(p4.y, m4.y, v4.y, g4.y, s);
    adamw_one(p4.z, m4.z, v4.z, g4.z, s);
    adamw_one(p4.w, m4.w, v4.w, g4.w, s);
    st4<ALIGNED>(p + e, p4);
    st4<ALIGNED>(m + e, m4);
    st4<ALIGNED>(v + e, v4);
    if (EMA) {
      ema_one(e4.x, p4.x, s);
      ema_one(e4.y, p4.y, s);
      ema_one(e4.z, p4.z, s);
      ema_one(e4.w, p4.w, s);
      st4<ALIGNED>(ea + e, e4);
    }
  }
  const int tail = 4 * n4 + threadIdx.x;
  if (tail < len) {
    float pp = p[tail], mm = m[tail], vv = v[tail];
    adamw_one(pp, mm, vv, g[tail], s);
    p[tail] = pp;
    m[tail] = mm;
    v[tail] = vv;
    if (EMA) {
      float ee = ea[tail];
      ema_one(ee, pp, s);
      ea[tail] = ee;
    }
  }
}

// A tensor without a gradient is not stepped, but its average still moves towards its (unchanged) value.
template <bool ALIGNED>
__device__ __forceinline__ void chunk_ema(const float* __restrict__ p, float* __restrict__ ea, int len,
                                          const StepScalars& s) {
  const int n4 = len >> 2;
  for (int i = threadIdx.x; i < n4; i += UD_OPTIM_THREADS) {
    const size_t e = 4 * (size_t)i;
    const float4 p4 = ld4<ALIGNED>(p + e);
    float4 e4 = ld4<ALIGNED>(ea + e);
    ema_one(e4.x, p4.x, s);
    ema_one(e4.y, p4.y, s);
    ema_one(e4.z, p4.z, s);
    ema_one(e4.w, p4.w, s);
    st4<ALIGNED>(ea + e, e4);
  }
  const int tail = 4 * n4 + threadIdx.x;
  if (tail < len) {
    float ee = ea[tail];
    ema_one(ee, p[tail], s);
    ea[tail] = ee;
  }
}

// Exact exchange of two streams: moves only, no arithmetic.
template <bool ALIGNED>
__device__ __forceinline__ void chunk_swap(float* __restrict__ a, float* __restrict__ b, int len) {
  const int n4 = len >> 2;
  for (int i = threadIdx.x; i < n4; i += UD_OPTIM_THREADS) {
    const size_t e = 4 * (size_t)i;
    const float4 a4 = ld4<ALIGNED>(a + e), b4 = ld4<ALIGNED>(b + e);
    st4<ALIGNED>(a + e, b4);
    st4<ALIGNED>(b + e, a4);
  }
  const int tail = 4 * n4 + threadIdx.x;
  if (tail < len) {
    const float aa = a[tail], bb = b[tail];
    a[tail] = bb;
    b[tail] = aa;
  }
}

struct Hyper {
  double beta1, beta2, eps, weight_decay, max_norm;
  int skip_nonfinite;
  double ema_decay, ema_ramp;                    // EMA only; ema_ramp <= 0: constant decay
};

template <bool EMA>
__global__ __launch_bounds__(UD_OPTIM_THREADS) void k_optim_clip_adamw(
    const UdOptimChunk* __restrict__ chunks, int n_chunks, float* const* __restrict__ params,
    float* const* __restrict__ exp_avg, float* const* __restrict__ exp_avg_sq, float* const* __restrict__ ema,
    const float* const* __restrict__ grads, const double* __restrict__ partial, double* __restrict__ state,
    const Hyper h) {
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
    if (EMA) {
      // step counts APPLIED steps, this one included: a skipped step does not advance the ramp
      const double decay = h.ema_ramp > 0.0 ? h.ema_decay * (1.0 - exp(-step / h.ema_ramp)) : h.ema_decay;
      sh.ema_w = (float)(1.0 - decay);
      sh.ema_omw = 1.0f - sh.ema_w;
      sh.ema_low = sh.ema_w < 0.5f;
    }
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
  if (sh_skip) return;                           // guard: no workgroup touches p, m, v or the EMA
  const UdOptimChunk c = chunks[blockIdx.x];
  const float* gt = grads[c.tensor];
  const StepScalars s = sh;
  float* p = params[c.tensor] + c.offset;
  float* ea = EMA ? ema[c.tensor] + c.offset : nullptr;
  if (gt == nullptr) {                           // a parameter without a gradient is left alone, as torch does
    if (EMA) {
      if (aligned16(p) && aligned16(ea))
        chunk_ema<true>(p, ea, c.length, s);
      else
        chunk_ema<false>(p, ea, c.length, s);
    }
    return;
  }
  float* m = exp_avg[c.tensor] + c.offset;
  float* v = exp_avg_sq[c.tensor] + c.offset;
  const float* g = gt + c.offset;
  if (aligned16(p) && aligned16(m) && aligned16(v) && aligned16(g) && (!EMA || aligned16(ea)))
    chunk_adamw<true, EMA>(p, m, v, ea, g, c.length, s);
  else
    chunk_adamw<false, EMA>(p, m, v, ea, g, c.length, s);
}

__global__ __launch_bounds__(UD_OPTIM_THREADS) void k_optim_swap(const UdOptimChunk* __restrict__ chunks,
                                                                  float* const* __restrict__ a_ptrs,
                                                                  float* const* __restrict__ b_ptrs) {
  const UdOptimChunk c = chunks[blockIdx.x];
  float* a = a_ptrs[c.tensor] + c.offset;
  float* b = b_ptrs[c.tensor] + c.offset;
  if (aligned16(a) && aligned16(b))
    chunk_swap<true>(a, b, c.length);
  else
    chunk_swap<false>(a, b, c.length);
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
  const Hyper h = {beta1, beta2, eps, weight_decay, max_norm, skip_nonfinite != 0, 0.0, 0.0};
  k_optim_clip_adamw<false><<<n_chunks, UD_OPTIM_THREADS, 0, stream>>>(chunks, n_chunks, params, exp_avg, exp_avg_sq,
                                                                      nullptr, grads, partial, state, h);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

extern "C" int ud_optim_clip_adamw_ema(const UdOptimChunk* chunks, int n_chunks, float* const* params,
                                       float* const* exp_avg, float* const* exp_avg_sq, float* const* ema,
                                       const float* const* grads, const double* partial, double* state, double beta1,
                                       double beta2, double eps, double weight_decay, double max_norm,
                                       int skip_nonfinite, double ema_decay, double ema_ramp, ud_stream_t stream_) {
  if (n_chunks < 0 ||
      (n_chunks > 0 && (!chunks || !params || !exp_avg || !exp_avg_sq || !ema || !grads || !partial)) || !state)
    return UD_ERR_INVALID_ARG;
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(max_norm > 0.0))
    return UD_ERR_INVALID_ARG;
  if (!(ema_decay > 0.0 && ema_decay < 1.0) || ema_ramp != ema_ramp) return UD_ERR_INVALID_ARG;
  if (n_chunks == 0) return UD_OK;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("optim.k_clip_adamw_ema", stream);
  const Hyper h = {beta1, beta2, eps, weight_decay, max_norm, skip_nonfinite != 0, ema_decay, ema_ramp};
  k_optim_clip_adamw<true><<<n_chunks, UD_OPTIM_THREADS, 0, stream>>>(chunks, n_chunks, params, exp_avg, exp_avg_sq, ema,
                                                                     grads, partial, state, h);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

extern "C" int ud_optim_swap(const UdOptimChunk* chunks, int n_chunks, float* const* a_ptrs, float* const* b_ptrs,
                             ud_stream_t stream_) {
  if (n_chunks < 0 || (n_chunks > 0 && (!chunks || !a_ptrs || !b_ptrs))) return UD_ERR_INVALID_ARG;
  if (n_chunks == 0) return UD_OK;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("optim.k_swap", stream);
  k_optim_swap<<<n_chunks, UD_OPTIM_THREADS, 0, stream>>>(chunks, a_ptrs, b_ptrs);
  UD_LAUNCH_CHECK();
  return UD_OK;
}
