// Building the GT-sampling object database on the device: OpenPCDet's create_groundtruth_database for
// whole scenes -- points_in_boxes_gpu, then per box ``gt_points = points[owner == i]; gt_points[:, :3] -= box[:3]``.
//
//   ud_points_in_boxes   k_points_in_boxes: one thread per row, 256-row tiles per sample.  The sample's boxes go through
//                        LDS in chunks of 64, in order, as centre / half extents / sin / cos (RmBox of box_inside.h, the
//                        paste's own inside test); a row stops at its first hit, so the lowest box index wins, across
//                        chunks too.  Every lane of a wave reads the same staged box: an LDS broadcast, no bank conflict.
//   ud_gt_db_count       k_db_tile_count  hits (owner >= 0) per 256-row tile: __ballot + popcount per wave
//                        k_db_scan        one workgroup: exclusive scan of the tile counts, the total, counts[] zeroed
//                        k_db_list        the compact hit list in row order, (global box id, row) at tile offset + earlier
//                                         waves + mbcnt; one integer atomic per hit into counts[box]
//   ud_gt_db_extract     rs_sort_pairs    stable radix sort of the hit list by box id (radix_sort.h): position j of the
//                                         order is output row j, objects in (sample, box) order, rows ascending inside
//                        k_db_gather      one thread per output row: xyz minus the box's float32 centre, the rest copied
// Only a few per cent of a scene's rows are hits, so everything after the tile count works on the short list.  Integer
// counting only: no floating-point atomics, every output row is written once by one thread, and neither the counts nor
// the order depend on the launch geometry.  Zeroing is done by k_db_scan, not a memset node.
#include "ud_common.h"
#include "ud_prof.h"
#include "box_inside.h"
#include "radix_sort.h"

namespace {

constexpr int kTile = 256;               // rows per block: 4 waves of 64, as the chain
constexpr int kWaves = kTile / 64;
constexpr int kBoxChunk = 64;            // boxes staged in LDS at a time: 2 KiB
constexpr int64_t kMaxBoxes = 1 << 18;   // boxes of one call: the sort key has at most 18 bits = two 9-bit passes

// Staged form of box q[0..7): a box with a non-finite entry gets negative half extents and contains nothing.
__device__ __forceinline__ RmBox stage_box(const float* __restrict__ q) {
  RmBox r;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 7; ++k) ok = ok && isfinite(q[k]);
  r.cx = q[0], r.cy = q[1], r.cz = q[2];
  r.hx = q[3] / 2 + 1e-5f, r.hy = q[4] / 2 + 1e-5f, r.hz = q[5] / 2;
  r.sn = sinf(q[6]), r.cs = cosf(q[6]);
  if (!ok) r = RmBox{0.f, 0.f, 0.f, -1.f, -1.f, -1.f, 0.f, 1.f};
  return r;
}

// Block (t, b): rows t * 256 .. of sample b.
__global__ __launch_bounds__(kTile) void k_points_in_boxes(const float* __restrict__ pts, int64_t pts_stride,
                                                           const int64_t* __restrict__ seg,
                                                           const float* __restrict__ boxes, int64_t box_stride,
                                                           const int64_t* __restrict__ box_off,
                                                           int32_t* __restrict__ owner) {
  __shared__ RmBox s_box[kBoxChunk];
  const int b = blockIdx.y;
  const int64_t row0 = seg[b], n = seg[b + 1] - row0;
  if ((int64_t)blockIdx.x * kTile >= n) return;                      // block-uniform: before any barrier
  const int64_t m0 = box_off[b];
  const int64_t m = box_off[b + 1] - m0;
  const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;
  const bool live = i < n;
  float xyz[3] = {0.f, 0.f, 0.f};
  bool open = false;                                                 // still looking for its first box
  if (live) {
    const float* p = pts + (row0 + i) * pts_stride;
    xyz[0] = p[0], xyz[1] = p[1], xyz[2] = p[2];
    open = isfinite(xyz[0]) && isfinite(xyz[1]) && isfinite(xyz[2]);
  }
  int32_t own = -1;
  for (int64_t c0 = 0; c0 < m; c0 += kBoxChunk) {                    // m is block-uniform
    const int nb = m - c0 < kBoxChunk ? (int)(m - c0) : kBoxChunk;
    __syncthreads();                                                 // the previous chunk has been read
    if (threadIdx.x < nb) s_box[threadIdx.x] = stage_box(boxes + (m0 + c0 + threadIdx.x) * box_stride);
    __syncthreads();
    if (open)
      for (int j = 0; j < nb; ++j)
        if (in_rm_box(s_box[j], xyz)) {
          own = (int32_t)(c0 + j);
          open = false;
          break;
        }
  }
  if (live) owner[row0 + i] = own;
}

// The global box id of a row's owner, or -1: the row's sample is the last b with seg[b] <= row (empty samples are
// skipped); an owner outside the sample's boxes is no hit.
__device__ __forceinline__ int64_t hit_box(const int32_t* __restrict__ owner, int64_t row,
                                           const int64_t* __restrict__ seg, const int64_t* __restrict__ box_off, int B) {
  const int32_t o = owner[row];
  if (o < 0) return -1;
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg[mid] <= row) lo = mid;
    else hi = mid - 1;
  }
  const int64_t m0 = box_off[lo];
  return o < box_off[lo + 1] - m0 ? m0 + o : -1;
}

__global__ __launch_bounds__(kTile) void k_db_tile_count(const int32_t* __restrict__ owner, int64_t rows,
                                                         const int64_t* __restrict__ seg,
                                                         const int64_t* __restrict__ box_off, int B,
                                                         int* __restrict__ tile_cnt) {
  __shared__ int s_wave[kWaves];
  const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;
  const bool hit = i < rows && hit_box(owner, i, seg, box_off, B) >= 0;
  const unsigned long long mk = __ballot(hit);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(mk);
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int w = 0; w < kWaves; ++w) c += s_wave[w];
    tile_cnt[blockIdx.x] = c;
  }
}

// One workgroup: tile_off[t] = sum of tile_cnt[0..t), counts[0..n_boxes) = 0, counts[n_boxes] = the number of hits.
__global__ __launch_bounds__(kTile) void k_db_scan(const int* __restrict__ tile_cnt, int* __restrict__ tile_off, int64_t NT,
                                                   int64_t* __restrict__ counts, int64_t n_boxes) {
  __shared__ int64_t sh[kTile];
  for (int64_t g = threadIdx.x; g < n_boxes; g += kTile) counts[g] = 0;
  const int64_t chunk = (NT + kTile - 1) / kTile;
  const int64_t lo = threadIdx.x * chunk < NT ? threadIdx.x * chunk : NT, hi = lo + chunk < NT ? lo + chunk : NT;
  int64_t s = 0;
  for (int64_t j = lo; j < hi; ++j) s += tile_cnt[j];
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
    tile_off[j] = (int)run;                                          // hits <= rows < 2^31
    run += tile_cnt[j];
  }
  if (threadIdx.x == kTile - 1) counts[n_boxes] = sh[kTile - 1];
}

__global__ __launch_bounds__(kTile) void k_db_list(const int32_t* __restrict__ owner, int64_t rows,
                                                   const int64_t* __restrict__ seg, const int64_t* __restrict__ box_off,
                                                   int B, const int* __restrict__ tile_off, unsigned* __restrict__ keys,
                                                   int32_t* __restrict__ hrow, int64_t* __restrict__ counts) {
  __shared__ int s_wave[kWaves];
  const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;
  const int64_t g = i < rows ? hit_box(owner, i, seg, box_off, B) : -1;
  const unsigned long long mk = __ballot(g >= 0);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_wave[wave] = __popcll(mk);
  __syncthreads();
  if (g < 0) return;
  int64_t rank = tile_off[blockIdx.x];
  for (int w = 0; w < wave; ++w) rank += s_wave[w];
  rank += __builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
  if (rank >= rows) return;                                          // cannot happen: hits <= rows
  keys[rank] = (unsigned)g;
  hrow[rank] = (int32_t)i;
  atomicAdd((unsigned long long*)(counts + g), 1ull);                // integer: the sum does not depend on the order
}

// Output row j = hit order[j] of the list: the row's D columns, xyz minus its box's centre (one float32 subtraction).
__global__ __launch_bounds__(kTile) void k_db_gather(const float* __restrict__ pts, int D, int64_t pts_stride,
                                                     int64_t rows, const float* __restrict__ boxes, int64_t box_stride,
                                                     int64_t n_boxes, const unsigned* __restrict__ keys,
                                                     const int32_t* __restrict__ hrow, const int32_t* __restrict__ order,
                                                     int64_t hits, float* __restrict__ out, int64_t out_rows) {
  const int64_t j = (int64_t)blockIdx.x * kTile + threadIdx.x;
  if (j >= hits || j >= out_rows) return;
  const int32_t h = order[j];
  if (h < 0 || h >= hits) return;                                    // cannot happen: order is a permutation of 0 .. hits
  const int64_t g = keys[h], row = hrow[h];
  if (g >= n_boxes || row < 0 || row >= rows) return;                // cannot happen for the list k_db_list wrote
  const float* src = pts + row * pts_stride;
  const float* box = boxes + g * box_stride;
  float* dst = out + j * D;
  dst[0] = src[0] - box[0];
  dst[1] = src[1] - box[1];
  dst[2] = src[2] - box[2];
  for (int c = 3; c < D; ++c) dst[c] = src[c];
}

// Pure host validation of the offsets (nothing on the device is touched).  -> the number of boxes in *n_boxes.
int check_offsets(int64_t rows, const int64_t* seg_host, const int64_t* box_off_host, int B, int64_t* n_boxes) {
  *n_boxes = 0;
  if (B < 0 || B > 65535 || rows < 0 || rows > 0x7fffffffLL) return UD_ERR_INVALID_ARG;
  if (B == 0) return rows == 0 ? UD_OK : UD_ERR_INVALID_ARG;
  if (!seg_host || !box_off_host) return UD_ERR_INVALID_ARG;
  if (seg_host[0] != 0 || seg_host[B] != rows || box_off_host[0] != 0) return UD_ERR_INVALID_ARG;
  for (int b = 0; b < B; ++b) {
    if (seg_host[b + 1] < seg_host[b] || box_off_host[b + 1] < box_off_host[b]) return UD_ERR_INVALID_ARG;
    if (box_off_host[b + 1] - box_off_host[b] > 0x7fffffffLL) return UD_ERR_INVALID_ARG;
  }
  if (box_off_host[B] > kMaxBoxes) return UD_ERR_INVALID_ARG;
  *n_boxes = box_off_host[B];
  return UD_OK;
}

int sort_bits(int64_t n_boxes) {
  int bits = 0;
  while ((1LL << bits) < n_boxes) ++bits;
  return bits;
}

// The workspace of ud_gt_db_count / ud_gt_db_extract, carved the same way by both.
struct DbWorkspace {
  int *tile_cnt, *tile_off;
  unsigned *keys, *ktmp[2], *hist, *dtot;
  int32_t *hrow, *order, *vtmp[2];
  size_t used;
  bool ok;
  DbWorkspace(void* p, size_t cap, int64_t rows, int64_t n_boxes) {
    UdArena a(p, cap);
    const size_t nt = (size_t)((rows + kTile - 1) / kTile), r = (size_t)rows;
    tile_cnt = a.take<int>(nt), tile_off = a.take<int>(nt);
    keys = a.take<unsigned>(r), hrow = a.take<int32_t>(r), order = a.take<int32_t>(r);
    const bool two = sort_bits(n_boxes) > 9;                         // a second pass needs one pair of buffers
    ktmp[0] = two ? a.take<unsigned>(r) : nullptr, vtmp[0] = two ? a.take<int32_t>(r) : nullptr;
    ktmp[1] = nullptr, vtmp[1] = nullptr;
    hist = a.take<unsigned>((size_t)kRsBinsMax * (size_t)ud_div_up(rows, kRsChunk));
    dtot = a.take<unsigned>(kRsBinsMax);
    used = a.used;
    ok = a.ok();
  }
};

}  // namespace

extern "C" int ud_points_in_boxes(const float* pts, int64_t rows, int D, int64_t pts_stride, const int64_t* seg_host,
                                  const int64_t* seg_dev, const float* boxes, int W, int64_t box_stride,
                                  const int64_t* box_off_host, const int64_t* box_off_dev, int B, int32_t* owner,
                                  ud_stream_t stream_) {
  int64_t n_boxes = 0;
  if (D < 3 || W < 7 || pts_stride < D || box_stride < W) return UD_ERR_INVALID_ARG;
  const int rc = check_offsets(rows, seg_host, box_off_host, B, &n_boxes);
  if (rc != UD_OK) return rc;
  if (rows == 0) return UD_OK;
  if (!pts || !owner || !seg_dev || !box_off_dev || (n_boxes > 0 && !boxes)) return UD_ERR_INVALID_ARG;
  int64_t mx = 0;
  for (int b = 0; b < B; ++b) mx = seg_host[b + 1] - seg_host[b] > mx ? seg_host[b + 1] - seg_host[b] : mx;
  const int64_t T = (mx + kTile - 1) / kTile;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("input.k_points_in_boxes", stream);
  k_points_in_boxes<<<dim3((unsigned)T, B), kTile, 0, stream>>>(pts, pts_stride, seg_dev, boxes, box_stride, box_off_dev,
                                                                owner);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

extern "C" size_t ud_gt_db_workspace_bytes(int64_t rows, int64_t n_boxes) {
  if (rows <= 0 || rows > 0x7fffffffLL || n_boxes < 0 || n_boxes > kMaxBoxes) return 0;
  return DbWorkspace(nullptr, 0, rows, n_boxes).used;
}

extern "C" int ud_gt_db_count(const int32_t* owner, int64_t rows, const int64_t* seg_host, const int64_t* seg_dev,
                              const int64_t* box_off_host, const int64_t* box_off_dev, int B, int64_t* counts,
                              void* workspace, size_t workspace_bytes, ud_stream_t stream_) {
  int64_t n_boxes = 0;
  const int rc = check_offsets(rows, seg_host, box_off_host, B, &n_boxes);
  if (rc != UD_OK) return rc;
  if (B == 0) return UD_OK;
  if (!counts || !seg_dev || !box_off_dev) return UD_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t NT = (rows + kTile - 1) / kTile;
  DbWorkspace ws(workspace, workspace_bytes, rows, n_boxes);
  if (rows > 0) {
    if (!owner) return UD_ERR_INVALID_ARG;
    if (!ws.ok) return UD_ERR_WORKSPACE;
    UdProfScope prof("input.k_db_tile_count", stream);
    k_db_tile_count<<<(unsigned)NT, kTile, 0, stream>>>(owner, rows, seg_dev, box_off_dev, B, ws.tile_cnt);
    UD_LAUNCH_CHECK();
  }
  {
    UdProfScope prof("input.k_db_scan", stream);
    k_db_scan<<<1, kTile, 0, stream>>>(ws.tile_cnt, ws.tile_off, NT, counts, n_boxes);
    UD_LAUNCH_CHECK();
  }
  if (rows > 0 && n_boxes > 0) {
    UdProfScope prof("input.k_db_list", stream);
    k_db_list<<<(unsigned)NT, kTile, 0, stream>>>(owner, rows, seg_dev, box_off_dev, B, ws.tile_off, ws.keys, ws.hrow,
                                                  counts);
    UD_LAUNCH_CHECK();
  }
  return UD_OK;
}

extern "C" int ud_gt_db_extract(const float* pts, int64_t rows, int D, int64_t pts_stride, const float* boxes, int W,
                                int64_t box_stride, int64_t n_boxes, const int64_t* counts_host, float* out,
                                int64_t out_rows, void* workspace, size_t workspace_bytes, ud_stream_t stream_) {
  if (D < 3 || W < 7 || pts_stride < D || box_stride < W) return UD_ERR_INVALID_ARG;
  if (rows < 0 || rows > 0x7fffffffLL || n_boxes < 0 || n_boxes > kMaxBoxes || out_rows < 0) return UD_ERR_INVALID_ARG;
  if (rows == 0 || n_boxes == 0) return UD_OK;
  if (!counts_host) return UD_ERR_INVALID_ARG;
  int64_t total = 0;
  for (int64_t g = 0; g < n_boxes; ++g) {
    if (counts_host[g] < 0 || counts_host[g] > rows) return UD_ERR_INVALID_ARG;
    total += counts_host[g];
  }
  if (total != counts_host[n_boxes] || total > rows || out_rows < total) return UD_ERR_INVALID_ARG;
  if (total == 0) return UD_OK;
  if (!pts || !boxes || !out) return UD_ERR_INVALID_ARG;
  DbWorkspace ws(workspace, workspace_bytes, rows, n_boxes);
  if (!ws.ok) return UD_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  {
    UdProfScope prof("input.db_sort", stream);
    const int rc = rs_sort_pairs<unsigned>(ws.keys, (int)total, sort_bits(n_boxes), ws.order, ws.ktmp, ws.vtmp, ws.hist,
                                           ws.dtot, stream);
    if (rc != UD_OK) return rc;
  }
  UdProfScope prof("input.k_db_gather", stream);
  k_db_gather<<<(unsigned)((total + kTile - 1) / kTile), kTile, 0, stream>>>(
      pts, D, pts_stride, rows, boxes, box_stride, n_boxes, ws.keys, ws.hrow, ws.order, total, out, out_rows);
  UD_LAUNCH_CHECK();
  return UD_OK;
}
