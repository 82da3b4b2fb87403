// LiDAR input chain after collate: the per-point half of the reference's det augmentor
// (unidistill/data/multisensorfusion/transforms3d.py) for a whole batch --
//   CollectLidarSweeps (:379-414)  sweep -> key frame, time lag into the last column when D == 5
//   BevAffineTransformation (:417-443)  the BDA matrix applied to the float32 result of the sweep transform
//   ObjectRangeFilter (:242-287)  x / y inside the range (z not tested, NaN fails), stable
// -- then collate_fn's fill_batch_tensor (nuscenes_multimodal.py:441-463): a contiguous zero-padded [B][Nmax][D].
//
// The raw clouds of the batch are staged contiguously: per sample a run of segments (key frame, then its sweeps).
// Three kernels, no atomics and no memset, so every output row is written exactly once and the result is bitwise
// reproducible:
//   k_lidar_count    one thread per input row: transforms + range test, __ballot + popcount per wave, one count per
//                    (sample, 256-row tile)
//   k_lidar_scan     per sample, an exclusive scan of its tile counts; the kept-row count of the sample
//   k_lidar_scatter  recomputes the test and writes each kept row at its rank (tile offset + earlier waves + mbcnt);
//                    the blocks past the tiles write the zero padding rows count_b .. Nmax.
// The host reads the counts back between the scan and the scatter to size Nmax.
//
// GT-sampling paste (ud_lidar_paste_count / ud_lidar_paste_compact) runs the same three kernels with a
// per-segment record (UdLidarPasteSeg) and per-sample removal boxes; the kernels are templates on that, so the plain
// entry points compile to the code they had.  A segment may read its rows from another buffer (the object database),
// is dropped whole when its gate byte is 0, and is an object or a scene segment.  A scene row is dropped when its
// float32 position after the segment transform, before BDA, lies inside a removal box whose accept byte is set:
//   sx = x - cx, sy = y - cy;  |z - cz| <= dz / 2;
//   lx = sx * cos(yaw) + sy * sin(yaw),  ly = -sx * sin(yaw) + sy * cos(yaw);  |lx| < dx / 2 + 1e-5, |ly| < dy / 2 + 1e-5
// in float32 (OpenPCDet's check_pt_in_box3d).  Every workgroup stages its sample's accepted boxes once in LDS as
// centre, half extents (+1e-5 on x / y) and sin / cos.
#include "ud_common.h"
#include "ud_prof.h"
#include "points_xform.h"
#include "box_inside.h"        // RmBox, in_rm_box: the inside test, shared with gt_database.hip

namespace {

constexpr int kTile = 256;               // input rows per block: 4 waves of 64
constexpr int kWaves = kTile / 64;
constexpr int kPadPerBlock = kTile * 4;  // padding floats per scatter block
constexpr int kMaxSeg = UD_LIDAR_MAX_SEGMENTS;

// seg_par[s]: see UD_LIDAR_SEG_PAR in unidistill_hip.h; smp_par[b]: UD_LIDAR_SMP_PAR.
constexpr int kSegMat = 0, kSegLast = 16, kSegXform = 17;
constexpr int kSmpBda = 0, kSmpRange = 16, kSmpHasBda = 22, kSmpHasRange = 23;

// The paste arguments of a launch (all NULL / 0 for a segment table alone).
struct PasteArgs {
  const UdLidarPasteSeg* seg;      // [S] or NULL
  const float* rm_boxes;           // [R][7]
  const int64_t* rm_off;           // [B + 1] or NULL: no removal boxes
  const uint8_t* rm_accept;        // box j of sample b: rm_accept[b * rm_stride + j]
  int64_t rm_stride;
};

// Stages sample b's accepted removal boxes in LDS, in order (wave 0; ends with a barrier).  -> their number.
__device__ __forceinline__ int stage_rm_boxes(const PasteArgs& pa, int b, RmBox* s_rm, int* s_nrm) {
  if (threadIdx.x < 64) {
    int n = 0;
    int64_t r0 = 0;
    if (pa.rm_off) {
      r0 = pa.rm_off[b];
      const int64_t n64 = pa.rm_off[b + 1] - r0;
      n = n64 < 0 ? 0 : (n64 > UD_GT_PASTE_MAX_CAND ? UD_GT_PASTE_MAX_CAND : (int)n64);          // host-checked
    }
    const int j = threadIdx.x;
    const bool on = j < n && pa.rm_accept[(int64_t)b * pa.rm_stride + j] != 0;
    const unsigned long long m = __ballot(on);
    if (on) {
      const float* q = pa.rm_boxes + (r0 + j) * 7;
      RmBox r;
      r.cx = q[0], r.cy = q[1], r.cz = q[2];
      r.hx = q[3] / 2 + 1e-5f, r.hy = q[4] / 2 + 1e-5f, r.hz = q[5] / 2;
      r.sn = sinf(q[6]), r.cs = cosf(q[6]);
      s_rm[__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = r;
    }
    if (j == 0) *s_nrm = __popcll(m);
  }
  __syncthreads();
  return *s_nrm;
}

struct SampleRows {
  int64_t row0, rows;
  int64_t seg0;
  int nseg;
};

// Loads the sample's segment row offsets into LDS (block-wide; ends with a barrier).
__device__ __forceinline__ SampleRows load_sample(const int64_t* __restrict__ seg, const int64_t* __restrict__ sseg,
                                                  int b, int64_t* s_off) {
  SampleRows r;
  r.seg0 = sseg[b];
  r.nseg = (int)(sseg[b + 1] - r.seg0);
  for (int i = threadIdx.x; i <= r.nseg; i += kTile) s_off[i] = seg[r.seg0 + i];
  __syncthreads();
  r.row0 = s_off[0];
  r.rows = s_off[r.nseg] - r.row0;
  return r;
}

// One input row through the chain: xyz after the sweep transform (a key-frame row is copied) and BDA, each rounded to
// float32; returns the range test.  sp / bp: the row's segment and sample parameters.
// With kPaste the row is dropped between the two transforms when its segment's gate is closed or, for a scene
// segment, when it lies inside one of the n_rm staged removal boxes.
template <bool kPaste>
__device__ __forceinline__ bool lidar_row(const float* __restrict__ p, const double* __restrict__ sp,
                                          const double* __restrict__ bp, float xyz[3],
                                          const UdLidarPasteSeg* ps = nullptr, const RmBox* s_rm = nullptr,
                                          int n_rm = 0) {
  xyz[0] = p[0], xyz[1] = p[1], xyz[2] = p[2];
  if (sp[kSegXform] != 0.0) {
    float t[3];
    ud_points_xform(sp + kSegMat, xyz[0], xyz[1], xyz[2], t);
    xyz[0] = t[0], xyz[1] = t[1], xyz[2] = t[2];
  }
  if (kPaste) {
    if (ps && ps->gate && *ps->gate == 0) return false;
    if (!ps || !ps->object)
      for (int j = 0; j < n_rm; ++j)
        if (in_rm_box(s_rm[j], xyz)) return false;
  }
  if (bp[kSmpHasBda] != 0.0) {
    float t[3];
    ud_points_xform(bp + kSmpBda, xyz[0], xyz[1], xyz[2], t);       // second rounding, as the reference
    xyz[0] = t[0], xyz[1] = t[1], xyz[2] = t[2];
  }
  if (bp[kSmpHasRange] == 0.0) return true;
  const double* rg = bp + kSmpRange;                                 // float32 values held exactly in float64
  return xyz[0] >= (float)rg[0] && xyz[0] <= (float)rg[3] && xyz[1] >= (float)rg[1] && xyz[1] <= (float)rg[4];
}

__device__ __forceinline__ int find_segment(const int64_t* s_off, int nseg, int64_t row) {
  int k = 0;
  while (k + 1 < nseg && row >= s_off[k + 1]) ++k;                   // skips empty segments
  return k;
}

// The row's source: the shared cloud, or the segment's own buffer (rows counted from the segment's first).
__device__ __forceinline__ const float* row_source(const float* __restrict__ pts, int D, const UdLidarPasteSeg* ps,
                                                   int64_t row, int64_t seg_row0) {
  return ps && ps->src ? ps->src + (row - seg_row0) * D : pts + row * D;
}

template <bool kPaste>
__global__ __launch_bounds__(kTile) void k_lidar_count(const float* __restrict__ pts, int D,
                                                       const int64_t* __restrict__ seg,
                                                       const int64_t* __restrict__ sseg,
                                                       const double* __restrict__ seg_par,
                                                       const double* __restrict__ smp_par,
                                                       int* __restrict__ tile_cnt, int64_t T, PasteArgs pa) {
  __shared__ int64_t s_off[kMaxSeg + 1];
  __shared__ int s_wave[kWaves];
  __shared__ RmBox s_rm[kPaste ? 64 : 1];
  __shared__ int s_nrm;
  const int b = blockIdx.y;
  const int64_t t = blockIdx.x;
  const SampleRows sr = load_sample(seg, sseg, b, s_off);
  const int n_rm = kPaste ? stage_rm_boxes(pa, b, s_rm, &s_nrm) : 0;
  const int64_t i = t * kTile + threadIdx.x;
  bool keep = false;
  if (i < sr.rows) {
    const int64_t row = sr.row0 + i;
    const int k = find_segment(s_off, sr.nseg, row);
    const UdLidarPasteSeg* ps = kPaste && pa.seg ? pa.seg + sr.seg0 + k : nullptr;
    float xyz[3];
    keep = lidar_row<kPaste>(kPaste ? row_source(pts, D, ps, row, s_off[k]) : pts + row * D,
                             seg_par + (sr.seg0 + k) * UD_LIDAR_SEG_PAR, smp_par + (int64_t)b * UD_LIDAR_SMP_PAR, xyz,
                             ps, s_rm, n_rm);
  }
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int w = 0; w < kWaves; ++w) c += s_wave[w];
    tile_cnt[(int64_t)b * T + t] = c;
  }
}

// One block per sample: tile_off[b][t] = sum of tile_cnt[b][0..t), counts[b] = the sample's kept rows.
__global__ __launch_bounds__(kTile) void k_lidar_scan(const int* __restrict__ tile_cnt, int64_t* __restrict__ tile_off,
                                                      int64_t* __restrict__ counts, int64_t T) {
  __shared__ int64_t sh[kTile];
  const int b = blockIdx.x;
  const int* c = tile_cnt + (int64_t)b * T;
  int64_t* o = tile_off + (int64_t)b * T;
  const int64_t chunk = (T + kTile - 1) / kTile;
  const int64_t lo = threadIdx.x * chunk, hi = lo + chunk < T ? lo + chunk : T;
  int64_t s = 0;
  for (int64_t j = lo; j < hi; ++j) s += c[j];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int d = 1; d < kTile; d <<= 1) {                              // inclusive Hillis-Steele scan of the chunk sums
    const int64_t v = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
    __syncthreads();
    sh[threadIdx.x] += v;
    __syncthreads();
  }
  int64_t run = sh[threadIdx.x] - s;
  for (int64_t j = lo; j < hi; ++j) {
    o[j] = run;
    run += c[j];
  }
  if (threadIdx.x == kTile - 1) counts[b] = sh[kTile - 1];
}

// blockIdx.x < T: tile t of sample b's input rows; blockIdx.x >= T: zero padding of sample b (padded output only).
// compact == 0: out [B][nmax][D], sample b at row b * nmax; compact == 1: samples back to back, no padding.
template <bool kPaste>
__global__ __launch_bounds__(kTile) void k_lidar_scatter(const float* __restrict__ pts, int D,
                                                         const int64_t* __restrict__ seg,
                                                         const int64_t* __restrict__ sseg,
                                                         const double* __restrict__ seg_par,
                                                         const double* __restrict__ smp_par,
                                                         const int64_t* __restrict__ tile_off,
                                                         const int64_t* __restrict__ counts, int64_t T, int64_t nmax,
                                                         int compact, float* __restrict__ out, int64_t out_rows,
                                                         PasteArgs pa) {
  __shared__ int64_t s_off[kMaxSeg + 1];
  __shared__ int64_t s_red[kTile];
  __shared__ int s_wave[kWaves];
  __shared__ RmBox s_rm[kPaste ? 64 : 1];
  __shared__ int s_nrm;
  const int b = blockIdx.y;
  const int64_t t = blockIdx.x;
  if (t >= T) {                                                      // block-uniform: no barrier below
    if (compact) return;
    const int64_t end = ((int64_t)b + 1) * nmax * D;
    const int64_t lim = out_rows * D;
    const int64_t e0 = ((int64_t)b * nmax + counts[b]) * D + (t - T) * kPadPerBlock + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kPadPerBlock / kTile; ++k) {
      const int64_t e = e0 + k * kTile;
      if (e >= 0 && e < end && e < lim) out[e] = 0.0f;
    }
    return;
  }
  const SampleRows sr = load_sample(seg, sseg, b, s_off);
  const int n_rm = kPaste ? stage_rm_boxes(pa, b, s_rm, &s_nrm) : 0;
  int64_t base = (int64_t)b * nmax;
  if (compact) {                                                     // rows kept by the samples before b
    int64_t s = 0;
    for (int j = threadIdx.x; j < b; j += kTile) s += counts[j];
    s_red[threadIdx.x] = s;
    __syncthreads();
    for (int d = kTile / 2; d > 0; d >>= 1) {
      if (threadIdx.x < d) s_red[threadIdx.x] += s_red[threadIdx.x + d];
      __syncthreads();
    }
    base = s_red[0];
  }
  const int64_t i = t * kTile + threadIdx.x;
  bool keep = false;
  float xyz[3] = {0.0f, 0.0f, 0.0f};
  int64_t row = 0;
  const double* sp = seg_par;
  const float* src = pts;
  if (i < sr.rows) {
    row = sr.row0 + i;
    const int k = find_segment(s_off, sr.nseg, row);
    sp = seg_par + (sr.seg0 + k) * UD_LIDAR_SEG_PAR;
    const UdLidarPasteSeg* ps = kPaste && pa.seg ? pa.seg + sr.seg0 + k : nullptr;
    src = kPaste ? row_source(pts, D, ps, row, s_off[k]) : pts + row * D;
    keep = lidar_row<kPaste>(src, sp, smp_par + (int64_t)b * UD_LIDAR_SMP_PAR, xyz, ps, s_rm, n_rm);
  }
  const unsigned long long m = __ballot(keep);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  int64_t rank = tile_off[(int64_t)b * T + t];
  for (int w = 0; w < wave; ++w) rank += s_wave[w];
  rank += __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
  const int64_t o = base + rank;
  if (o >= out_rows) return;                                         // cannot happen for a consistent plan
  float* dst = out + o * D;
  dst[0] = xyz[0];
  dst[1] = xyz[1];
  dst[2] = xyz[2];
  for (int c = 3; c < D; ++c) dst[c] = src[c];
  const double lv = sp[kSegLast];
  if (D > 3 && lv == lv) dst[D - 1] = (float)lv;                     // NaN = keep the column
}

int64_t tiles_of(const int64_t* seg_host, const int64_t* sseg_host, int B) {
  int64_t mx = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t rows = seg_host[sseg_host[b + 1]] - seg_host[sseg_host[b]];
    if (rows > mx) mx = rows;
  }
  return (mx + kTile - 1) / kTile;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

size_t ws_bytes_for(int64_t B, int64_t T) { return align16((size_t)(B * T) * 4) + (size_t)(B * T) * 8; }

// Pure host validation of the plan (nothing on the device is touched).
// pts == nullptr with need_pts == false: the offsets alone (workspace query).
int check_plan(const float* pts, int64_t rows, int D, const int64_t* seg_host, const int64_t* sseg_host, int S, int B,
               bool need_pts = true) {
  if (S < 0 || B < 0 || B > 65535 || D < 3 || D > 1024 || rows < 0) return UD_ERR_INVALID_ARG;
  if (need_pts && rows > 0 && !pts) return UD_ERR_INVALID_ARG;
  if (!seg_host || !sseg_host) return UD_ERR_INVALID_ARG;            // S + 1 and B + 1 entries: never empty
  if (seg_host[0] < 0 || seg_host[S] > rows) return UD_ERR_INVALID_ARG;
  for (int s = 0; s < S; ++s)
    if (seg_host[s + 1] < seg_host[s]) return UD_ERR_INVALID_ARG;
  if (sseg_host[0] != 0 || sseg_host[B] != S) return UD_ERR_INVALID_ARG;
  for (int b = 0; b < B; ++b)
    if (sseg_host[b + 1] < sseg_host[b] || sseg_host[b + 1] - sseg_host[b] > kMaxSeg) return UD_ERR_INVALID_ARG;
  return UD_OK;
}

int check_dev(const int64_t* seg_dev, const int64_t* sseg_dev, const double* seg_par, const double* smp_par, int S,
              int B) {
  if (B > 0 && (!seg_dev || !sseg_dev || !smp_par)) return UD_ERR_INVALID_ARG;
  if (S > 0 && !seg_par) return UD_ERR_INVALID_ARG;
  return UD_OK;
}


// Host validation of the paste arguments.  pa.seg may be NULL (no gates, no foreign sources, every segment a scene
// segment) and pa.rm_off NULL (no removal boxes).
int check_paste(const PasteArgs& pa, const int64_t* rm_off_host, int B) {
  if ((pa.rm_off == nullptr) != (rm_off_host == nullptr)) return UD_ERR_INVALID_ARG;
  if (!rm_off_host) return UD_OK;
  if (rm_off_host[0] < 0 || pa.rm_stride < 0) return UD_ERR_INVALID_ARG;
  for (int b = 0; b < B; ++b) {
    const int64_t n = rm_off_host[b + 1] - rm_off_host[b];
    if (n < 0 || n > UD_GT_PASTE_MAX_CAND || n > pa.rm_stride) return UD_ERR_INVALID_ARG;
  }
  if (B > 0 && rm_off_host[B] > rm_off_host[0] && (!pa.rm_boxes || !pa.rm_accept)) return UD_ERR_INVALID_ARG;
  return UD_OK;
}

// The two entry points' work; pa == nullptr: the plain chain.
int run_count(const float* pts, int64_t rows, int D, const int64_t* seg_host, const int64_t* sample_seg_host, int S, int B,
              const int64_t* seg_dev, const int64_t* sample_seg_dev, const double* seg_par, const double* smp_par,
              int64_t* counts, void* workspace, size_t workspace_bytes, hipStream_t stream, const PasteArgs* pa,
              const int64_t* rm_off_host) {
  int rc = check_plan(pts, rows, D, seg_host, sample_seg_host, S, B, !(pa && pa->seg));
  if (rc != UD_OK) return rc;
  if ((rc = check_dev(seg_dev, sample_seg_dev, seg_par, smp_par, S, B)) != UD_OK) return rc;
  if (pa && (rc = check_paste(*pa, rm_off_host, B)) != UD_OK) return rc;
  if (B == 0) return UD_OK;
  if (!counts) return UD_ERR_INVALID_ARG;
  const int64_t T = tiles_of(seg_host, sample_seg_host, B);
  if (T > 0x7fffffffLL) return UD_ERR_INVALID_ARG;
  const size_t need = ws_bytes_for(B, T);
  if (need > 0 && (!workspace || workspace_bytes < need)) return UD_ERR_WORKSPACE;
  int* tile_cnt = (int*)workspace;
  int64_t* tile_off = (int64_t*)((char*)workspace + align16((size_t)(B * T) * 4));
  if (T > 0) {
    UdProfScope prof(pa ? "input.k_lidar_count_paste" : "input.k_lidar_count", stream);
    if (pa)
      k_lidar_count<true><<<dim3((unsigned)T, B), kTile, 0, stream>>>(pts, D, seg_dev, sample_seg_dev, seg_par, smp_par,
                                                                        tile_cnt, T, *pa);
    else
      k_lidar_count<false><<<dim3((unsigned)T, B), kTile, 0, stream>>>(pts, D, seg_dev, sample_seg_dev, seg_par,
                                                                         smp_par, tile_cnt, T, PasteArgs{});
    UD_LAUNCH_CHECK();
  }
  UdProfScope prof("input.k_lidar_scan", stream);
  k_lidar_scan<<<B, kTile, 0, stream>>>(tile_cnt, tile_off, counts, T);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

int run_compact(const float* pts, int64_t rows, int D, const int64_t* seg_host, const int64_t* sample_seg_host, int S,
                int B, const int64_t* seg_dev, const int64_t* sample_seg_dev, const double* seg_par,
                const double* smp_par, const int64_t* counts_host, const int64_t* counts, int64_t nmax, int compact,
                float* out, int64_t out_rows, void* workspace, size_t workspace_bytes, hipStream_t stream,
                const PasteArgs* pa, const int64_t* rm_off_host) {
  int rc = check_plan(pts, rows, D, seg_host, sample_seg_host, S, B, !(pa && pa->seg));
  if (rc != UD_OK) return rc;
  if ((rc = check_dev(seg_dev, sample_seg_dev, seg_par, smp_par, S, B)) != UD_OK) return rc;
  if (pa && (rc = check_paste(*pa, rm_off_host, B)) != UD_OK) return rc;
  if (B == 0) return UD_OK;
  if (!counts_host || !counts || nmax < 0 || out_rows < 0 || (out_rows > 0 && !out)) return UD_ERR_INVALID_ARG;
  int64_t total = 0, lo = nmax;
  for (int b = 0; b < B; ++b) {
    const int64_t c = counts_host[b];
    const int64_t srows = seg_host[sample_seg_host[b + 1]] - seg_host[sample_seg_host[b]];
    if (c < 0 || c > srows || (!compact && c > nmax)) return UD_ERR_INVALID_ARG;
    total += c;
    if (c < lo) lo = c;
  }
  if (compact ? out_rows < total : out_rows < (int64_t)B * nmax) return UD_ERR_INVALID_ARG;
  const int64_t T = tiles_of(seg_host, sample_seg_host, B);
  const size_t need = ws_bytes_for(B, T);
  if (need > 0 && (!workspace || workspace_bytes < need)) return UD_ERR_WORKSPACE;
  const int64_t P = compact ? 0 : ((nmax - lo) * D + kPadPerBlock - 1) / kPadPerBlock;
  if (T + P == 0) return UD_OK;
  if (T + P > 0x7fffffffLL) return UD_ERR_INVALID_ARG;
  const int64_t* tile_off = (const int64_t*)((const char*)workspace + align16((size_t)(B * T) * 4));
  UdProfScope prof(pa ? "input.k_lidar_scatter_paste" : "input.k_lidar_scatter", stream);
  if (pa)
    k_lidar_scatter<true><<<dim3((unsigned)(T + P), B), kTile, 0, stream>>>(
        pts, D, seg_dev, sample_seg_dev, seg_par, smp_par, tile_off, counts, T, nmax, compact ? 1 : 0, out, out_rows, *pa);
  else
    k_lidar_scatter<false><<<dim3((unsigned)(T + P), B), kTile, 0, stream>>>(
        pts, D, seg_dev, sample_seg_dev, seg_par, smp_par, tile_off, counts, T, nmax, compact ? 1 : 0, out, out_rows,
        PasteArgs{});
  UD_LAUNCH_CHECK();
  return UD_OK;
}

}  // namespace

extern "C" size_t ud_lidar_prep_workspace_bytes(const int64_t* seg_host, const int64_t* sample_seg_host, int S,
                                                int B) {
  if (check_plan(nullptr, seg_host && S >= 0 ? seg_host[S] : 0, 3, seg_host, sample_seg_host, S, B, false) != UD_OK)
    return 0;
  return ws_bytes_for(B, tiles_of(seg_host, sample_seg_host, B));
}

extern "C" int ud_lidar_prep_count(const float* pts, int64_t rows, int D, const int64_t* seg_host,
                                   const int64_t* sample_seg_host, int S, int B, const int64_t* seg_dev,
                                   const int64_t* sample_seg_dev, const double* seg_par, const double* smp_par,
                                   int64_t* counts, void* workspace, size_t workspace_bytes, ud_stream_t stream_) {
  return run_count(pts, rows, D, seg_host, sample_seg_host, S, B, seg_dev, sample_seg_dev, seg_par, smp_par, counts,
                   workspace, workspace_bytes, (hipStream_t)stream_, nullptr, nullptr);
}

extern "C" int ud_lidar_prep_compact(const float* pts, int64_t rows, int D, const int64_t* seg_host,
                                     const int64_t* sample_seg_host, int S, int B, const int64_t* seg_dev,
                                     const int64_t* sample_seg_dev, const double* seg_par, const double* smp_par,
                                     const int64_t* counts_host, const int64_t* counts, int64_t nmax, int compact,
                                     float* out, int64_t out_rows, void* workspace, size_t workspace_bytes,
                                     ud_stream_t stream_) {
  return run_compact(pts, rows, D, seg_host, sample_seg_host, S, B, seg_dev, sample_seg_dev, seg_par, smp_par,
                     counts_host, counts, nmax, compact, out, out_rows, workspace, workspace_bytes, (hipStream_t)stream_,
                     nullptr, nullptr);
}

extern "C" int ud_lidar_paste_count(const float* pts, int64_t rows, int D, const int64_t* seg_host,
                                    const int64_t* sample_seg_host, int S, int B, const int64_t* seg_dev,
                                    const int64_t* sample_seg_dev, const double* seg_par, const double* smp_par,
                                    const UdLidarPasteSeg* seg_paste, const float* rm_boxes, const int64_t* rm_off_host,
                                    const int64_t* rm_off_dev, const uint8_t* rm_accept, int64_t rm_stride,
                                    int64_t* counts, void* workspace, size_t workspace_bytes, ud_stream_t stream_) {
  const PasteArgs pa{seg_paste, rm_boxes, rm_off_dev, rm_accept, rm_stride};
  return run_count(pts, rows, D, seg_host, sample_seg_host, S, B, seg_dev, sample_seg_dev, seg_par, smp_par, counts,
                   workspace, workspace_bytes, (hipStream_t)stream_, &pa, rm_off_host);
}

extern "C" int ud_lidar_paste_compact(const float* pts, int64_t rows, int D, const int64_t* seg_host,
                                      const int64_t* sample_seg_host, int S, int B, const int64_t* seg_dev,
                                      const int64_t* sample_seg_dev, const double* seg_par, const double* smp_par,
                                      const UdLidarPasteSeg* seg_paste, const float* rm_boxes,
                                      const int64_t* rm_off_host, const int64_t* rm_off_dev, const uint8_t* rm_accept,
                                      int64_t rm_stride, const int64_t* counts_host, const int64_t* counts, int64_t nmax,
                                      int compact, float* out, int64_t out_rows, void* workspace, size_t workspace_bytes,
                                      ud_stream_t stream_) {
  const PasteArgs pa{seg_paste, rm_boxes, rm_off_dev, rm_accept, rm_stride};
  return run_compact(pts, rows, D, seg_host, sample_seg_host, S, B, seg_dev, sample_seg_dev, seg_par, smp_par,
                     counts_host, counts, nmax, compact, out, out_rows, workspace, workspace_bytes, (hipStream_t)stream_,
                     &pa, rm_off_host);
}
