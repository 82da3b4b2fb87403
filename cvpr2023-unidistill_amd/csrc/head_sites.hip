// Work lists of the frozen distillation teacher's head (train.py: DistillStep.teacher).  The teacher's head output has one
// consumer, ResponseDistillLoss, which weights every site by the Gaussian box mask (csrc/distill.hip: k_resp): a few small blobs
// on the BEV map.  One launch turns mask f32[B][H][W] into
//   * the pixel blocks of the first head convolution (ud_conv3x3_wino4_units_nhwc_f32) that the tail will read at a mask site:
//     blocks whose rectangle, grown by one pixel (the tail is a 3x3 convolution), holds a site with mask > 0,
//   * the strips of the grouped tail (ud_head_tail_f32_bn_fwd_sites) that hold such a site, with the rows they span,
// both as (count, ascending indices) in device memory: no host read-back, and no grid depends on them.
#include "ud_common.h"
#include "ud_prof.h"

namespace {

struct SitesGeom {
  int B, H, W, bw, bh, bx, by, sw, sh, sx, sy, nblocks, nstrips;
};

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// flags[0 .. n) -> list[0] = count, list[1 ..] = the set indices, ascending (one workgroup of 256 threads)
__device__ void compact(const int* flags, int n, int* __restrict__ list, int* s_wave) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int run = 0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + tid;
    const bool f = i < n && ld_agent(flags + i) != 0;
    const unsigned long long m = __ballot(f);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int off = run;
    for (int k = 0; k < wave; ++k) off += s_wave[k];
    if (f) list[1 + off + __popcll(m & ((1ull << lane) - 1ull))] = i;
    run += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
  }
  if (tid == 0) list[0] = run;
}

// workgroup u < nblocks: convolution block u; else tail strip u - nblocks.  The workgroup that draws the last ticket compacts.
__global__ __launch_bounds__(256) void k_head_sites(const float* __restrict__ mask, SitesGeom g, int* __restrict__ conv_units,
                                                    int* __restrict__ tail_strips, int* __restrict__ tail_rows,
                                                    int* __restrict__ scratch) {
  __shared__ int s_lo, s_hi, s_last, s_wave[4];
  const int tid = threadIdx.x, u = blockIdx.x;
  const bool conv = u < g.nblocks;
  int r = conv ? u : u - g.nblocks;
  const int nx = conv ? g.bx : g.sx, ny = conv ? g.by : g.sy, w = conv ? g.bw : g.sw, h = conv ? g.bh : g.sh;
  const int ix = r % nx;
  r /= nx;
  const int iy = r % ny, b = r / ny;
  const int grow = conv ? 1 : 0;
  const int x0 = max(ix * w - grow, 0), x1 = min((ix + 1) * w + grow, g.W);
  const int y0 = max(iy * h - grow, 0), y1 = min((iy + 1) * h + grow, g.H);
  if (tid == 0) s_lo = 0x7fffffff, s_hi = -1;
  __syncthreads();
  const int ww = x1 - x0, n = ww * (y1 - y0);
  int lo = 0x7fffffff, hi = -1;
  for (int i = tid; i < n; i += 256) {
    const int yy = y0 + i / ww, xx = x0 + i % ww;
    if (mask[((size_t)b * g.H + yy) * g.W + xx] > 0.f) lo = min(lo, yy), hi = max(hi, yy);
  }
  if (hi >= 0) {
    atomicMin(&s_lo, lo);
    atomicMax(&s_hi, hi);
  }
  __syncthreads();
  if (tid == 0) {
    const bool any = s_hi >= 0;
    if (!conv) {
      tail_rows[2 * (u - g.nblocks)] = any ? s_lo : 0;
      tail_rows[2 * (u - g.nblocks) + 1] = any ? s_hi + 1 : 0;
    }
    st_agent(scratch + 1 + u, any ? 1 : 0);
    __threadfence();
    s_last = atomicAdd(scratch, 1) == g.nblocks + g.nstrips - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  compact(scratch + 1, g.nblocks, conv_units, s_wave);
  compact(scratch + 1 + g.nblocks, g.nstrips, tail_strips, s_wave);
}

}  // namespace

extern "C" int ud_head_sites_build(const float* mask, int B, int H, int W, int blk_w, int blk_h, int strip_w, int strip_h,
                                   int* conv_units, int* tail_strips, int* tail_rows, int* scratch, ud_stream_t stream_) {
  if (!mask || !conv_units || !tail_strips || !tail_rows || !scratch || B <= 0 || H <= 0 || W <= 0 || blk_w <= 0 || blk_h <= 0 ||
      strip_w <= 0 || strip_h <= 0)
    return UD_ERR_INVALID_ARG;
  SitesGeom g{B, H, W, blk_w, blk_h, ud_div_up(W, blk_w), ud_div_up(H, blk_h), strip_w, strip_h, ud_div_up(W, strip_w),
              ud_div_up(H, strip_h), 0, 0};
  const long long nb = (long long)B * g.bx * g.by, ns = (long long)B * g.sx * g.sy;
  if (nb + ns > 0x3fffffffll) return UD_ERR_UNSUPPORTED;
  g.nblocks = (int)nb, g.nstrips = (int)ns;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("head_sites.k_head_sites", stream);
  k_head_sites<<<(unsigned)(nb + ns), 256, 0, stream>>>(mask, g, conv_units, tail_strips, tail_rows, scratch);
  UD_LAUNCH_CHECK();
  return UD_OK;
}
