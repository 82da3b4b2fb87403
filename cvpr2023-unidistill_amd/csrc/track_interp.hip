// Linear interpolation of ground-truth and predicted tracks across missed frames, the step the nuScenes devkit runs between its
// filters and its tracking metric.  The normative text is in include/unidistill_hip.h (ud_track_interp_count);
// tests/track_interp_reference.py restates it.
//
//   k_ti_walk<false> : count call.  One 512-thread workgroup per (scene, side), frames in order, one thread per row of the frame:
//                      kept test (track_kept.h), at most one row per key and frame, and per key the last kept (frame, row) in the
//                      scene's workspace slice (indexed by key).  A kept row whose key was last seen more than one frame ago closes
//                      a hole: its thread adds one to the counter of every frame of the hole (integer atomics).  At the end: rows
//                      per sample = kept + interpolated, the interpolated total, the GT rows per class.
//   k_ti_walk<true>  : fill call.  The same walk; the thread that closes a hole leaves one entry (key, L row, R row, L frame, R
//                      frame) per frame of the hole, in the order the integer atomics happen to give.
//   k_ti_emit        : fill call.  One workgroup per (frame, side): the kept rows compacted in row order (lds_sort.h), then the
//                      frame's entries ranked by key (unique within a frame), each interpolated row computed by one thread from
//                      its two endpoints.
//
// No floating-point atomics, no inter-workgroup communication, nothing waits on the host inside a call.
#include "ud_common.h"
#include "ud_prof.h"
#include "lds_sort.h"
#include "track_kept.h"
#include <climits>
#include <cmath>

namespace {

constexpr int kThreads = UD_TM_MAX_FRAME_ROWS;     // one thread per row of a frame
constexpr int kWaves = kThreads / UD_WAVE;
constexpr int kEntryInts = 5;
static_assert(kThreads % UD_WAVE == 0 && kThreads <= 1024, "one workgroup holds a frame's rows");

struct Side {
  const double* vals;            // [rows][cols]
  const int* cls;
  const int* key;
  const int* npts;               // GT only
  const unsigned char* keep;     // GT only
  const long long* start;        // predictions: row_start; GT: gt_off (count == nullptr: count = start[s + 1] - start[s])
  const long long* count;
  long long rows, slots;         // keys lie in key_min .. slots - 1
  int cols, key_min, max_boxes;
  int* last_frame;               // workspace [NS][slots]
  int* last_row;
  int* kept_cnt;                 // workspace [F]
  int* cursor;                   // workspace [F]: interpolated rows of the frame
  long long* w_count;            // count call: [S]
  unsigned long long* w_interp;  // count call: [1]
  unsigned long long* w_cls;     // count call: [UD_NUS_MAX_CLASSES] or nullptr
  const long long* out_start;    // fill call
  const long long* out_count;
  long long out_rows;
  int* entry;                    // workspace [kEntryInts][out_rows]
  double* out_vals;
  int* out_cls;
  int* out_key;
  int* out_src;
};

struct Params {
  int C, mode;
  long long S, F, NS;
  unsigned char tracked[UD_NUS_MAX_CLASSES + 1];
  double range[UD_NUS_MAX_CLASSES];
  const double* ego;
  const long long* frame_sample;
  const long long* scene_off;
  const long long* frame_ts;
  int* status;
  Side side[2];
};

// the rows of frame fi on one side, checked against the inputs; false: the frame is treated as empty
__device__ __forceinline__ bool side_rows(const Params& prm, const Side& sd, long long fi, long long& sample, long long& r0,
                                          int& rn, int& st) {
  sample = prm.frame_sample[fi];
  r0 = 0, rn = 0;
  if (sample < 0 || sample >= prm.S) { st |= UD_TI_ST_RANGE; return false; }
  const long long s0 = sd.start[sample], n = sd.count ? sd.count[sample] : sd.start[sample + 1] - s0;
  if (n < 0 || n > kThreads || s0 < 0 || s0 > sd.rows - n) { st |= UD_TI_ST_RANGE; return false; }
  r0 = s0, rn = (int)n;
  return true;
}

// step 1 of the definition for one row
__device__ __forceinline__ bool side_kept(const Params& prm, const Side& sd, long long row, long long sample, int& key, int& c,
                                          int& st) {
  c = sd.cls[row];
  key = sd.key[row];
  const bool candidate = sd.keep ? (sd.keep[row] != 0 && sd.npts[row] > 0) : key > 0;
  if (!ud_tm_row_kept(candidate, c, prm.C, prm.tracked, prm.range, sd.vals + row * sd.cols, sd.cols, prm.ego + sample * 3,
                      UD_TI_ST_NONFINITE, st))
    return false;
  if (key < sd.key_min || key >= sd.slots) { st |= UD_TI_ST_KEY; return false; }
  return true;
}

template <bool kFill>
__global__ __launch_bounds__(kThreads) void k_ti_walk(Params prm) {
  __shared__ int s_key[kThreads];
  __shared__ int s_cls[UD_NUS_MAX_CLASSES];
  const Side& sd = prm.side[blockIdx.y];
  const int tid = threadIdx.x;
  const long long sc = blockIdx.x;
  int* lf = sd.last_frame + sc * sd.slots;
  int* lr = sd.last_row + sc * sd.slots;
  int st = 0;
  long long f0 = prm.scene_off[sc], f1 = prm.scene_off[sc + 1];
  if (f0 < 0 || f1 > prm.F || f1 < f0 || f1 - f0 > INT_MAX) { st |= UD_TI_ST_RANGE; f1 = f0; }
  for (long long i = tid; i < sd.slots; i += kThreads) lf[i] = -1;
  for (long long fi = f0 + tid; fi < f1; fi += kThreads) { sd.cursor[fi] = 0; sd.kept_cnt[fi] = 0; }
  if (tid < UD_NUS_MAX_CLASSES) s_cls[tid] = 0;
  __syncthreads();

  for (long long fi = f0; fi < f1; ++fi) {
    const int fidx = (int)(fi - f0);
    long long sample, r0;
    int rn;
    side_rows(prm, sd, fi, sample, r0, rn, st);
    bool kept = false;
    int key = 0, c = 0;
    const long long row = r0 + tid;
    if (tid < rn) kept = side_kept(prm, sd, row, sample, key, c, st);
    s_key[tid] = kept ? key : INT_MIN;
    const int nkept = __syncthreads_count(kept);
    if (nkept > sd.max_boxes) st |= UD_TI_ST_BOXES;
    if (kept) {
      bool first = true;
      for (int j = 0; j < tid; ++j)
        if (s_key[j] == key) { first = false; break; }
      if (!first) {
        st |= UD_TI_ST_DUPLICATE;
      } else {
        const int pf = lf[key], pr = lr[key];          // this key's slot is touched by this thread alone in this frame
        lf[key] = fidx;
        lr[key] = (int)row;
        if (pf >= 0 && fidx - pf > 1) {                // a hole: frames pf + 1 .. fidx - 1
          for (int g = pf + 1; g < fidx; ++g) {
            const int slot = atomicAdd(&sd.cursor[f0 + g], 1);
            if (kFill) {
              const long long sg = prm.frame_sample[f0 + g];
              if (sg < 0 || sg >= prm.S) continue;     // reported by the walk when it passed the frame
              const long long at = (long long)sd.kept_cnt[f0 + g] + slot;
              if (at >= sd.out_count[sg] || sd.out_start[sg] < 0 || sd.out_start[sg] > sd.out_rows - sd.out_count[sg]) {
                st |= UD_TI_ST_RANGE;
                continue;
              }
              int* e = sd.entry + sd.out_start[sg] + at;
              e[0] = key;
              e[sd.out_rows] = pr;
              e[2 * sd.out_rows] = (int)row;
              e[3 * sd.out_rows] = (int)(f0 + pf);
              e[4 * sd.out_rows] = (int)fi;
            }
          }
          if (!kFill && sd.w_cls) atomicAdd(&s_cls[c], fidx - pf - 1);   // an interpolated row takes the class of R
        }
      }
      if (!kFill && sd.w_cls) atomicAdd(&s_cls[c], 1);
    }
    if (tid == 0) sd.kept_cnt[fi] = nkept;
    __syncthreads();
  }

  if (!kFill) {
    unsigned long long interp = 0;
    for (long long fi = f0 + tid; fi < f1; fi += kThreads) {
      const long long sample = prm.frame_sample[fi];
      if (sample < 0 || sample >= prm.S) continue;
      sd.w_count[sample] = (long long)sd.kept_cnt[fi] + sd.cursor[fi];
      interp += (unsigned long long)sd.cursor[fi];
    }
    if (interp) atomicAdd(sd.w_interp, interp);
    if (sd.w_cls && tid < prm.C && s_cls[tid]) atomicAdd(&sd.w_cls[tid], (unsigned long long)s_cls[tid]);
  }
  if (st) atomicOr(prm.status, st);
}

// (1 - w) * a + w * b: 1 - w is rounded by the caller; two rounded products, one rounded sum
__device__ __forceinline__ double lerp_rn(double omw, double w, double a, double b) {
  return __dadd_rn(__dmul_rn(omw, a), __dmul_rn(w, b));
}

__global__ __launch_bounds__(kThreads) void k_ti_emit(Params prm) {
  __shared__ int s_key[kThreads];
  __shared__ int s_wsum[kWaves];
  const Side& sd = prm.side[blockIdx.y];
  const int tid = threadIdx.x;
  const long long fi = blockIdx.x;
  int st = 0;
  long long sample, r0;
  int rn;
  if (!side_rows(prm, sd, fi, sample, r0, rn, st)) {       // uniform over the workgroup
    if (st && tid == 0) atomicOr(prm.status, st);
    return;
  }
  const long long o0 = sd.out_start[sample], on = sd.out_count[sample];
  if (on < 0 || on > kThreads || o0 < 0 || o0 > sd.out_rows - on) {
    if (tid == 0) atomicOr(prm.status, UD_TI_ST_RANGE);
    return;
  }
  // ---- the kept rows, in row order
  bool kept = false;
  int key = 0, c = 0;
  const long long row = r0 + tid;
  if (tid < rn) kept = side_kept(prm, sd, row, sample, key, c, st);
  const UdBlockRank cr = ud_block_rank<kWaves>(kept, s_wsum);
  const int nkept = cr.total;
  if (kept) {
    const int pos = cr.rank();
    if (pos < on) {
      const double* v = sd.vals + row * sd.cols;
      double* o = sd.out_vals + (o0 + pos) * sd.cols;
      for (int i = 0; i < sd.cols; ++i) o[i] = v[i];
      sd.out_cls[o0 + pos] = c;
      sd.out_key[o0 + pos] = key;
      sd.out_src[o0 + pos] = (int)row;
    }
  }
  // ---- the frame's interpolated rows, in ascending key
  long long want = on - nkept;
  const int have = sd.cursor[fi];
  if (want != have) st |= UD_TI_ST_RANGE;                  // the inputs give other counts than the layout holds
  if (want > have) want = have;
  const int n = want < 0 ? 0 : (int)want;
  const int* e = sd.entry + o0 + nkept;
  int k = INT_MAX;
  if (tid < n) k = e[tid];
  s_key[tid] = k;
  __syncthreads();
  if (tid < n) {
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += s_key[j] < k;
    const long long L = e[tid + sd.out_rows], R = e[tid + 2 * sd.out_rows];
    const long long fL = e[tid + 3 * sd.out_rows], fR = e[tid + 4 * sd.out_rows];
    if (L < 0 || L >= sd.rows || R < 0 || R >= sd.rows || fL < 0 || fL >= prm.F || fR < 0 || fR >= prm.F) {
      st |= UD_TI_ST_RANGE;
    } else {
      const long long tL = prm.frame_ts[fL], tR = prm.frame_ts[fR], tf = prm.frame_ts[fi];
      double w = 0.0;
      if (tR - tL > 0) w = (double)(prm.mode == UD_TI_MODE_DEVKIT ? tR - tf : tf - tL) / (double)(tR - tL);
      else st |= UD_TI_ST_RANGE;
      const double omw = __dsub_rn(1.0, w);
      const double* a = sd.vals + L * sd.cols;
      const double* b = sd.vals + R * sd.cols;
      const long long at = o0 + nkept + rank;
      double* o = sd.out_vals + at * sd.cols;
      for (int i = 0; i < sd.cols; ++i) {
        if (i == 6) {                                      // yaw (predictions): the shorter arc, not re-wrapped
          const double d = remainder(__dsub_rn(b[6], a[6]), 6.283185307179586);
          o[6] = __dadd_rn(a[6], __dmul_rn(w, d));
        } else {
          o[i] = lerp_rn(omw, w, a[i], b[i]);
        }
      }
      sd.out_cls[at] = sd.cls[R];
      sd.out_key[at] = k;
      sd.out_src[at] = -1;
    }
  }
  if (st) atomicOr(prm.status, st);
}

struct Plan {
  long long slots[2];
};

bool plan_of(const UdTrackInterpCfg& cfg, Plan& p) {
  if (cfg.num_classes < 1 || cfg.num_classes > UD_NUS_MAX_CLASSES) return false;
  if (cfg.mode != UD_TI_MODE_DEVKIT && cfg.mode != UD_TI_MODE_LINEAR) return false;
  if (cfg.num_scenes < 1 || cfg.num_scenes > (1 << 20) || cfg.num_samples < 1 || cfg.num_frames < 0) return false;
  if (cfg.num_frames > 0x7FFFFFFFll || cfg.num_samples > 0x7FFFFFFFll) return false;
  if (cfg.num_rows < 0 || cfg.num_rows > 0x7FFFFFFFll || cfg.num_gt < 0 || cfg.num_gt > 0x7FFFFFFFll) return false;
  if (cfg.max_frame_rows < 0 || cfg.max_frame_rows > kThreads || cfg.max_boxes_per_sample < 1) return false;
  if (cfg.max_scene_rows < 0 || cfg.max_scene_rows > cfg.num_rows) return false;
  if (cfg.max_gt_keys < 0 || cfg.max_gt_keys > UD_TI_MAX_GT_KEYS) return false;
  if (cfg.num_out_pred < 0 || cfg.num_out_pred > 0x7FFFFFFFll / kEntryInts) return false;
  if (cfg.num_out_gt < 0 || cfg.num_out_gt > 0x7FFFFFFFll / kEntryInts) return false;
  bool any = false;
  for (int c = 0; c < cfg.num_classes; ++c) {
    if (!cfg.track_class[c]) continue;
    any = true;
    if (!(cfg.class_range[c] >= 0.0)) return false;
  }
  if (!any) return false;
  p.slots[0] = cfg.max_scene_rows + 1;
  p.slots[1] = std::max<long long>(cfg.max_gt_keys, 1);
  return true;
}

struct Scratch {
  int *last_frame[2], *last_row[2], *kept_cnt[2], *cursor[2], *entry[2];
};

size_t carve(const UdTrackInterpCfg& cfg, const Plan& p, void* ws, size_t bytes, Scratch* s) {
  UdArena ar(ws, bytes);
  const long long out[2] = {cfg.num_out_pred, cfg.num_out_gt};
  const size_t F = (size_t)std::max<long long>(cfg.num_frames, 1);
  Scratch x;
  for (int i = 0; i < 2; ++i) {
    x.last_frame[i] = ar.take<int>((size_t)cfg.num_scenes * p.slots[i]);
    x.last_row[i] = ar.take<int>((size_t)cfg.num_scenes * p.slots[i]);
    x.kept_cnt[i] = ar.take<int>(F);
    x.cursor[i] = ar.take<int>(F);
    x.entry[i] = ar.take<int>((size_t)kEntryInts * std::max<long long>(out[i], 1));
  }
  if (s) *s = x;
  return ar.used;
}

// everything the two calls share; 0 or an error code
int setup(const double* pred_rec, const int32_t* pred_cls, const int32_t* track_id, const int64_t* row_start,
          const int64_t* row_count, const double* gt_xyz, const int32_t* gt_cls, const int32_t* gt_num_pts, const uint8_t* gt_keep,
          const int32_t* gt_key, const int64_t* gt_off, const double* ego, const int64_t* frame_sample, const int64_t* scene_off,
          const int64_t* frame_ts, const UdTrackInterpCfg* cfg_host, int32_t* status, void* workspace, size_t workspace_bytes,
          Params& prm) {
  if (!cfg_host) return UD_ERR_INVALID_ARG;
  const UdTrackInterpCfg& cfg = *cfg_host;
  Plan p;
  if (!plan_of(cfg, p)) return UD_ERR_INVALID_ARG;
  if (!row_start || !row_count || !gt_off || !ego || !frame_sample || !scene_off || !frame_ts || !status) return UD_ERR_INVALID_ARG;
  if (cfg.num_rows > 0 && (!pred_rec || !pred_cls || !track_id)) return UD_ERR_INVALID_ARG;
  if (cfg.num_gt > 0 && (!gt_xyz || !gt_cls || !gt_num_pts || !gt_keep || !gt_key)) return UD_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < carve(cfg, p, nullptr, 0, nullptr)) return UD_ERR_WORKSPACE;
  Scratch s;
  carve(cfg, p, workspace, workspace_bytes, &s);
  prm = {};
  prm.C = cfg.num_classes;
  prm.mode = cfg.mode;
  prm.S = cfg.num_samples, prm.F = cfg.num_frames, prm.NS = cfg.num_scenes;
  for (int c = 0; c < cfg.num_classes; ++c) {
    prm.tracked[c] = cfg.track_class[c] != 0;
    prm.range[c] = cfg.class_range[c];
  }
  prm.ego = ego;
  prm.frame_sample = (const long long*)frame_sample, prm.scene_off = (const long long*)scene_off;
  prm.frame_ts = (const long long*)frame_ts;
  prm.status = status;
  Side& a = prm.side[0];
  a.vals = pred_rec, a.cols = UD_NUS_PRED_COLS, a.cls = pred_cls, a.key = track_id;
  a.npts = nullptr, a.keep = nullptr;
  a.start = (const long long*)row_start, a.count = (const long long*)row_count;
  a.rows = cfg.num_rows, a.key_min = 1, a.max_boxes = cfg.max_boxes_per_sample;
  Side& b = prm.side[1];
  b.vals = gt_xyz, b.cols = 3, b.cls = gt_cls, b.key = gt_key;
  b.npts = gt_num_pts, b.keep = gt_keep;
  b.start = (const long long*)gt_off, b.count = nullptr;
  b.rows = cfg.num_gt, b.key_min = 0, b.max_boxes = INT_MAX;
  for (int i = 0; i < 2; ++i) {
    Side& sd = prm.side[i];
    sd.slots = p.slots[i];
    sd.last_frame = s.last_frame[i], sd.last_row = s.last_row[i], sd.kept_cnt = s.kept_cnt[i], sd.cursor = s.cursor[i];
    sd.entry = s.entry[i];
  }
  return UD_OK;
}

}  // namespace

extern "C" {

size_t ud_track_interp_workspace_bytes(const UdTrackInterpCfg* cfg) {
  Plan p;
  if (!cfg || !plan_of(*cfg, p)) return 0;
  return carve(*cfg, p, nullptr, 0, nullptr);
}

int ud_track_interp_count(const double* pred_rec, const int32_t* pred_cls, const int32_t* track_id, const int64_t* row_start,
                          const int64_t* row_count, const double* gt_xyz, const int32_t* gt_cls, const int32_t* gt_num_pts,
                          const uint8_t* gt_keep, const int32_t* gt_key, const int64_t* gt_off, const double* ego,
                          const int64_t* frame_sample, const int64_t* scene_off, const int64_t* frame_ts,
                          const UdTrackInterpCfg* cfg_host, int64_t* counts, int32_t* status, void* workspace,
                          size_t workspace_bytes, ud_stream_t stream_) {
  Params prm;
  if (!counts) return UD_ERR_INVALID_ARG;
  if (const int e = setup(pred_rec, pred_cls, track_id, row_start, row_count, gt_xyz, gt_cls, gt_num_pts, gt_keep, gt_key, gt_off,
                          ego, frame_sample, scene_off, frame_ts, cfg_host, status, workspace, workspace_bytes, prm))
    return e;
  const long long S = cfg_host->num_samples;
  for (int i = 0; i < 2; ++i) {
    prm.side[i].w_count = (long long*)counts + i * S;
    prm.side[i].w_interp = (unsigned long long*)counts + 2 * S + i;
  }
  prm.side[0].w_cls = nullptr;
  prm.side[1].w_cls = (unsigned long long*)counts + 2 * S + 2;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("track_interp_count", stream);
  UD_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)(2 * S + 2 + UD_NUS_MAX_CLASSES) * sizeof(int64_t), stream));
  k_ti_walk<false><<<dim3((unsigned)cfg_host->num_scenes, 2), kThreads, 0, stream>>>(prm);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

int ud_track_interp_fill(const double* pred_rec, const int32_t* pred_cls, const int32_t* track_id, const int64_t* row_start,
                         const int64_t* row_count, const double* gt_xyz, const int32_t* gt_cls, const int32_t* gt_num_pts,
                         const uint8_t* gt_keep, const int32_t* gt_key, const int64_t* gt_off, const double* ego,
                         const int64_t* frame_sample, const int64_t* scene_off, const int64_t* frame_ts,
                         const UdTrackInterpCfg* cfg_host, const int64_t* pred_out_start, const int64_t* pred_out_count,
                         const int64_t* gt_out_start, const int64_t* gt_out_count, double* out_rec, int32_t* out_pred_cls,
                         int32_t* out_pred_key, int32_t* out_pred_src, double* out_xyz, int32_t* out_gt_cls,
                         int32_t* out_gt_key, int32_t* out_gt_src, int32_t* status, void* workspace, size_t workspace_bytes,
                         ud_stream_t stream_) {
  Params prm;
  if (!pred_out_start || !pred_out_count || !gt_out_start || !gt_out_count) return UD_ERR_INVALID_ARG;
  if (cfg_host && cfg_host->num_out_pred > 0 && (!out_rec || !out_pred_cls || !out_pred_key || !out_pred_src)) return UD_ERR_INVALID_ARG;
  if (cfg_host && cfg_host->num_out_gt > 0 && (!out_xyz || !out_gt_cls || !out_gt_key || !out_gt_src)) return UD_ERR_INVALID_ARG;
  if (const int e = setup(pred_rec, pred_cls, track_id, row_start, row_count, gt_xyz, gt_cls, gt_num_pts, gt_keep, gt_key, gt_off,
                          ego, frame_sample, scene_off, frame_ts, cfg_host, status, workspace, workspace_bytes, prm))
    return e;
  Side& a = prm.side[0];
  a.out_start = (const long long*)pred_out_start, a.out_count = (const long long*)pred_out_count;
  a.out_rows = cfg_host->num_out_pred;
  a.out_vals = out_rec, a.out_cls = out_pred_cls, a.out_key = out_pred_key, a.out_src = out_pred_src;
  Side& b = prm.side[1];
  b.out_start = (const long long*)gt_out_start, b.out_count = (const long long*)gt_out_count;
  b.out_rows = cfg_host->num_out_gt;
  b.out_vals = out_xyz, b.out_cls = out_gt_cls, b.out_key = out_gt_key, b.out_src = out_gt_src;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("track_interp_fill", stream);
  k_ti_walk<true><<<dim3((unsigned)cfg_host->num_scenes, 2), kThreads, 0, stream>>>(prm);
  UD_LAUNCH_CHECK();
  if (cfg_host->num_frames > 0) {
    k_ti_emit<<<dim3((unsigned)cfg_host->num_frames, 2), kThreads, 0, stream>>>(prm);
    UD_LAUNCH_CHECK();
  }
  return UD_OK;
}

}  // extern "C"
