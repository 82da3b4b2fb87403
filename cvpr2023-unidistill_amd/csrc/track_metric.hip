// The nuScenes tracking metric (AMOTA, AMOTP, MOTA, IDS ...) over the rows of NuScenesTracker.  The normative
// algorithm is in include/unidistill_hip.h (ud_track_metric); tests/track_metric_reference.py restates it.
//
//   k_tm_scores     : one 512-thread workgroup per scene, frames in order: the kept flag of every prediction row and the mean
//                     detection score of its track, summed in (frame, row) order in the scene's workspace slice (indexed by id).
//   k_tm_walk       : ONE WAVE per problem (scene, class, pass); launched twice: the all-boxes pass, then the K threshold passes.
//                     Per frame: ordered compaction of the class's GT rows and hypotheses into LDS (xy, ids, instance numbers),
//                     re-establish (GT row order, the lanes scan the hypotheses), gate (objects and hypotheses without an
//                     admissible partner leave), a shortest-augmenting-path assignment over the rest with distances recomputed
//                     from the coordinates (forbidden pairs cost `big`), then the events and the per-instance counters in LDS.
//   k_tm_keys + rs_sort_pairs + k_tm_thresholds : the all-boxes pass's MATCH scores, sorted descending over all classes at once
//                     (radix_sort.h), split per class by an ordered compaction, and interpolated at the recall thresholds.
//   k_tm_finalize   : per (class, pass) the per-scene partials summed in scene order.
//
// No inter-workgroup communication, no spinning, no floating-point atomics; the only atomic is the OR into *status.  Nothing
// waits on the host: the launches above are enqueued back to back.
#include "ud_common.h"
#include "ud_prof.h"
#include "lds_sort.h"
#include "radix_sort.h"
#include <cmath>

namespace {

constexpr int kCap = UD_TM_MAX_FRAME_ROWS;       // kept rows of one side of one frame
constexpr int kParts = UD_TM_COUNTS;             // integers of one problem's partial
constexpr int kScoreThreads = kCap;
constexpr double kInf = 1e300;
enum { kFrames, kObjects, kMatches, kSwitches, kFp, kMiss, kMt, kMl, kFrag, kTid, kLgd, kInst };
constexpr int kEver = 1, kGap = 2;
static_assert(kParts == 12 && kCap % 64 == 0 && kCap <= 65535, "partials and the 16-bit row numbers");

struct Params {
  int C, T, K, cap, inst_cap, max_boxes, events_pass;
  long long P, G, S, F, NS, slots;
  double dist_th, big;
  int cls_of[UD_NUS_MAX_CLASSES];                // tracked slot -> class
  unsigned char tracked[UD_NUS_MAX_CLASSES + 1];
  double range[UD_NUS_MAX_CLASSES];              // by class
  long long seg[UD_NUS_MAX_CLASSES + 1];         // tracked slot -> first entry of its sorted MATCH scores
};

struct Ptrs {
  const double* rec;
  const int* cls;
  const int* track_id;
  const long long* row_start;
  const long long* row_count;
  const double* gt_xyz;
  const int* gt_cls;
  const int* gt_npts;
  const unsigned char* gt_keep;
  const int* gt_inst;
  const long long* gt_off;
  const double* ego;
  const long long* frame_sample;
  const long long* scene_off;
  const double* recall;
  double* acc_sum;
  int* acc_cnt;
  double* hscore;          // [P] the track's mean score, NaN: the row is not kept
  double* mscore;          // [G] all-boxes pass: the hypothesis score of a MATCH, NaN otherwise
  double* sorted;          // [G] per class segment: MATCH scores descending
  int* order;
  int* part_i;
  double* part_d;
  double* thresholds;
  long long* nscores;
  long long* counts;
  double* dist;
  int* valid;
  int* ev_type;
  int* ev_row;
  int* status;
};

__host__ __device__ inline size_t walk_lds_bytes(int cap, int ic) {
  return (size_t)cap * (8 * sizeof(double) + 5 * sizeof(int) + 4 * sizeof(unsigned short) + 4) + (size_t)ic * (sizeof(int) + 8 * sizeof(unsigned short));
}

__device__ __forceinline__ bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// a frame's sample and its two row ranges, checked against the inputs; false: the frame is treated as empty
__device__ __forceinline__ bool frame_rows(const Ptrs& a, const Params& prm, long long fi, int cap, long long& sample,
                                           long long& g0, int& gn, long long& p0, int& pn, int& st) {
  sample = a.frame_sample[fi];
  g0 = p0 = 0;
  gn = pn = 0;
  if (sample < 0 || sample >= prm.S) { st |= UD_TM_ST_RANGE; return false; }
  const long long gs = a.gt_off[sample], gc = a.gt_off[sample + 1] - gs;
  const long long ps = a.row_start[sample], pc = a.row_count[sample];
  if (gc < 0 || gc > cap || gs < 0 || gs > prm.G - gc || pc < 0 || pc > cap || ps < 0 || ps > prm.P - pc) {
    st |= UD_TM_ST_RANGE;
    return false;
  }
  g0 = gs, gn = (int)gc, p0 = ps, pn = (int)pc;
  return true;
}

// ---- kept flags and track mean scores ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScoreThreads) void k_tm_scores(Ptrs a, Params prm) {
  __shared__ int s_id[kCap];
  __shared__ double s_sc[kCap];
  const int tid = threadIdx.x;
  const long long sc = blockIdx.x;
  double* sum = a.acc_sum + sc * prm.slots;
  int* cnt = a.acc_cnt + sc * prm.slots;
  for (long long i = tid; i < prm.slots; i += kScoreThreads) { sum[i] = 0.0; cnt[i] = 0; }
  int st = 0;
  long long f0 = a.scene_off[sc], f1 = a.scene_off[sc + 1];
  if (f0 < 0 || f1 > prm.F || f1 < f0) { st |= UD_TM_ST_RANGE; f1 = f0; }
  __syncthreads();
  for (long long fi = f0; fi < f1; ++fi) {
    long long sample, g0, p0;
    int gn, pn;
    frame_rows(a, prm, fi, kCap, sample, g0, gn, p0, pn, st);
    bool kept = false;
    int id = 0;
    double score = 0.0;
    if (tid < pn) {
      const long long row = p0 + tid;
      const int c = a.cls[row];
      id = a.track_id[row];
      if (id > 0 && c >= 0 && c < prm.C && prm.tracked[c]) {
        const double* r = a.rec + row * UD_NUS_PRED_COLS;
        score = r[9];
        if (!finite3(r[0], r[1], r[2]) || !isfinite(score)) {
          st |= UD_TM_ST_NONFINITE;
        } else {
          kept = ud_dist_xy(r[0], r[1], a.ego[sample * 3], a.ego[sample * 3 + 1]) <= prm.range[c];
          if (kept && id >= prm.slots) { st |= UD_TM_ST_ID; kept = false; }
        }
      }
      a.hscore[row] = kept ? 1.0 : __longlong_as_double(0x7FF8000000000000ll);
    }
    s_id[tid] = kept ? id : 0;
    s_sc[tid] = score;
    const int nkept = __syncthreads_count(kept);
    if (nkept > prm.max_boxes) st |= UD_TM_ST_BOXES;
    if (kept) {
      bool first = true;
      for (int j = 0; j < tid; ++j)
        if (s_id[j] == id) { first = false; break; }
      if (first) {                                   // the id's rows of this frame in row order, after its earlier frames
        double s = sum[id];
        int n = cnt[id];
        for (int j = tid; j < pn; ++j)
          if (s_id[j] == id) { s = s + s_sc[j]; ++n; }
        sum[id] = s;
        cnt[id] = n;
      }
    }
    __syncthreads();
  }
  for (long long fi = f0; fi < f1; ++fi) {
    long long sample, g0, p0;
    int gn, pn, ignore = 0;
    frame_rows(a, prm, fi, kCap, sample, g0, gn, p0, pn, ignore);
    if (tid < pn) {
      const long long row = p0 + tid;
      if (a.hscore[row] == 1.0) {
        const int id = a.track_id[row];
        a.hscore[row] = sum[id] / (double)cnt[id];
      }
    }
  }
  if (st) atomicOr(a.status, st);
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_tm_walk(Ptrs a, Params prm, int threshold_passes) {
  extern __shared__ double s_dyn[];
  const int cap = prm.cap, ic = prm.inst_cap, lane = threadIdx.x;
  double* s_ox = s_dyn;
  double* s_oy = s_ox + cap;
  double* s_hx = s_oy + cap;
  double* s_hy = s_hx + cap;
  double* s_u = s_hy + cap;
  double* s_v = s_u + cap;
  double* s_minv = s_v + cap;
  double* s_od = s_minv + cap;
  int* s_hid = reinterpret_cast<int*>(s_od + cap);
  int* s_oinst = s_hid + cap;
  int* s_omatch = s_oinst + cap;
  int* s_way = s_omatch + cap;
  int* s_p = s_way + cap;
  int* s_m = s_p + cap;                                  // [ic] instance -> the track id last matched to it, 0 = none
  unsigned short* s_ri = reinterpret_cast<unsigned short*>(s_m + ic);
  unsigned short* s_ci = s_ri + cap;
  unsigned short* s_orow = s_ci + cap;
  unsigned short* s_hrow = s_orow + cap;
  unsigned short* s_app = s_hrow + cap;                  // [ic] each: appearances, tracked appearances, first appearance,
  unsigned short* s_trk = s_app + ic;                    // frames to the first tracked one, current and longest MISS run,
  unsigned short* s_first = s_trk + ic;                  // fragmentations, flags
  unsigned short* s_tid = s_first + ic;
  unsigned short* s_run = s_tid + ic;
  unsigned short* s_maxrun = s_run + ic;
  unsigned short* s_frag = s_maxrun + ic;
  unsigned short* s_flags = s_frag + ic;
  unsigned char* s_used = reinterpret_cast<unsigned char*>(s_flags + ic);
  unsigned char* s_hcl = s_used + cap;                   // the hypothesis is claimed
  unsigned char* s_hadm = s_hcl + cap;
  unsigned char* s_oadm = s_hadm + cap;

  const long long b = blockIdx.x;
  int k = -1, t;
  long long sc;
  if (!threshold_passes) {
    t = (int)(b % prm.T);
    sc = b / prm.T;
  } else {
    k = (int)(b % prm.K);
    t = (int)((b / prm.K) % prm.T);
    sc = b / ((long long)prm.K * prm.T);
  }
  const long long q = (sc * prm.T + t) * (prm.K + 1) + (k + 1);
  const int c = prm.cls_of[t];
  int* part = a.part_i + q * kParts;
  double theta = 0.0;
  if (k >= 0) {
    theta = a.thresholds[t * prm.K + k];
    if (theta != theta) {                                  // the pass is not run
      if (lane < kParts) part[lane] = 0;
      if (lane == 0) a.part_d[q] = 0.0;
      return;
    }
  }
  const bool events = prm.events_pass == k && a.ev_type != nullptr;
  const double th = prm.dist_th, big = prm.big, range = prm.range[c];
  const unsigned long long below = (1ull << lane) - 1ull;

  for (int i = lane; i < ic; i += 64) {
    s_m[i] = 0;
    s_app[i] = s_trk[i] = s_tid[i] = s_run[i] = s_maxrun[i] = s_frag[i] = s_flags[i] = 0;
    s_first[i] = 0xFFFF;
  }
  int st = 0, n_match = 0, n_switch = 0, n_miss = 0;      // per lane
  int frames = 0, objects = 0, fp = 0;                    // the same in every lane
  double dist_sum = 0.0;
  long long f0 = a.scene_off[sc], f1 = a.scene_off[sc + 1];
  if (f0 < 0 || f1 > prm.F || f1 < f0 || f1 - f0 > 65534) { st |= UD_TM_ST_RANGE; f1 = f0; }
  __syncthreads();

  for (long long fi = f0; fi < f1; ++fi) {
    const int fidx = (int)(fi - f0);
    long long sample, g0, p0;
    int gn, pn;
    frame_rows(a, prm, fi, cap, sample, g0, gn, p0, pn, st);
    double ex = 0.0, ey = 0.0;
    if (gn > 0) { ex = a.ego[sample * 3]; ey = a.ego[sample * 3 + 1]; }

    // ---- 1: rows in play, in row order
    int no = 0, nh = 0;
    for (int c0 = 0; c0 < gn; c0 += 64) {
      const int r = c0 + lane;
      bool ok = false;
      double x = 0.0, y = 0.0;
      int inst = 0;
      if (r < gn) {
        const long long row = g0 + r;
        if (a.gt_cls[row] == c && a.gt_keep[row] && a.gt_npts[row] > 0) {
          x = a.gt_xyz[row * 3];
          y = a.gt_xyz[row * 3 + 1];
          inst = a.gt_inst[row];
          if (!finite3(x, y, a.gt_xyz[row * 3 + 2])) st |= UD_TM_ST_NONFINITE;
          else if (inst < 0 || inst >= ic) st |= UD_TM_ST_RANGE;
          else ok = ud_dist_xy(x, y, ex, ey) <= range;
        }
      }
      const unsigned long long bal = __ballot(ok);
      if (ok) {
        const int pos = no + __popcll(bal & below);
        s_ox[pos] = x;
        s_oy[pos] = y;
        s_oinst[pos] = inst;
        s_orow[pos] = (unsigned short)r;
        s_omatch[pos] = -1;
      }
      no += __popcll(bal);
    }
    for (int c0 = 0; c0 < pn; c0 += 64) {
      const int r = c0 + lane;
      bool ok = false;
      if (r < pn && a.cls[p0 + r] == c) {
        const double s = a.hscore[p0 + r];
        ok = s == s && (k < 0 || s >= theta);
      }
      const unsigned long long bal = __ballot(ok);
      if (ok) {
        const int pos = nh + __popcll(bal & below);
        const double* rr = a.rec + (p0 + r) * UD_NUS_PRED_COLS;
        s_hx[pos] = rr[0];
        s_hy[pos] = rr[1];
        s_hid[pos] = a.track_id[p0 + r];
        s_hrow[pos] = (unsigned short)r;
        s_hcl[pos] = 0;
        s_hadm[pos] = 0;
      }
      nh += __popcll(bal);
    }
    if (no == 0 && nh == 0) continue;                      // not a frame of this pass
    ++frames;
    objects += no;
    __syncthreads();

    // ---- 2: re-establish, objects in GT row order
    for (int o0 = 0; o0 < no && nh > 0; o0 += 64) {
      const int o = o0 + lane;
      const int want = o < no ? s_m[s_oinst[o]] : 0;
      unsigned long long mask = __ballot(want > 0);
      while (mask) {
        const int src = __builtin_ctzll(mask);
        mask &= mask - 1;
        const int oo = o0 + src, wid = __shfl(want, src);
        const double x0 = s_ox[oo], y0 = s_oy[oo];
        int best = 0x7FFFFFFF;
        for (int h = lane; h < nh; h += 64)
          if (s_hid[h] == wid && !s_hcl[h] && ud_dist_xy(x0, y0, s_hx[h], s_hy[h]) < th) { best = h; break; }
        best = ud_wave_min(best);
        if (best != 0x7FFFFFFF && lane == 0) {
          s_hcl[best] = 1;
          s_omatch[oo] = best;
          s_od[oo] = ud_dist_xy(x0, y0, s_hx[best], s_hy[best]);
        }
        __syncthreads();
      }
    }

    // ---- 3: gate, then assign what is left
    for (int o = lane; o < no; o += 64) {
      int deg = 0;
      if (s_omatch[o] < 0) {
        const double x0 = s_ox[o], y0 = s_oy[o];
        for (int h = 0; h < nh; ++h)
          if (!s_hcl[h] && ud_dist_xy(x0, y0, s_hx[h], s_hy[h]) < th) { deg = 1; s_hadm[h] = 1; }
      }
      s_oadm[o] = (unsigned char)deg;
    }
    __syncthreads();
    int n1 = 0, n2 = 0;                                     // contested objects -> s_ri, contested hypotheses -> s_ci
    for (int c0 = 0; c0 < no; c0 += 64) {
      const int o = c0 + lane;
      const bool ok = o < no && s_oadm[o];
      const unsigned long long bal = __ballot(ok);
      if (ok) s_ri[n1 + __popcll(bal & below)] = (unsigned short)o;
      n1 += __popcll(bal);
    }
    for (int c0 = 0; c0 < nh; c0 += 64) {
      const int h = c0 + lane;
      const bool ok = h < nh && s_hadm[h];
      const unsigned long long bal = __ballot(ok);
      if (ok) s_ci[n2 + __popcll(bal & below)] = (unsigned short)h;
      n2 += __popcll(bal);
    }
    __syncthreads();
    if (n1 > 0 && n2 > 0) {
      // rows = the smaller side, so that every row is assigned; costs d if d < th, else big
      const bool obj_rows = n1 <= n2;
      const int na = obj_rows ? n1 : n2, nb = obj_rows ? n2 : n1;
      const unsigned short* ri = obj_rows ? s_ri : s_ci;
      const unsigned short* ci = obj_rows ? s_ci : s_ri;
      const double* rx = obj_rows ? s_ox : s_hx;
      const double* ry = obj_rows ? s_oy : s_hy;
      const double* cx = obj_rows ? s_hx : s_ox;
      const double* cy = obj_rows ? s_hy : s_oy;
      for (int j = lane; j < nb; j += 64) { s_v[j] = 0.0; s_p[j] = -1; }
      for (int i = lane; i < na; i += 64) s_u[i] = 0.0;
      __syncthreads();
      for (int i = 0; i < na; ++i) {
        for (int j = lane; j < nb; j += 64) { s_minv[j] = kInf; s_used[j] = 0; }
        int j0 = -1;
        bool found = false;
        for (int it = 0; it <= nb; ++it) {                 // each trip adds one column to the tree
          const int i0 = j0 < 0 ? i : s_p[j0];
          if (j0 >= 0 && (j0 & 63) == lane) s_used[j0] = 1;  // read back by this lane only
          const double ui0 = s_u[i0], x0 = rx[ri[i0]], y0 = ry[ri[i0]];
          double bestv = kInf;
          int bestj = 0x7FFFFFFF;
          for (int j = lane; j < nb; j += 64) {
            if (s_used[j]) continue;
            const double d = ud_dist_xy(x0, y0, cx[ci[j]], cy[ci[j]]);
            const double cur = (d < th ? d : big) - ui0 - s_v[j];
            double mv = s_minv[j];
            if (cur < mv) { mv = cur; s_minv[j] = cur; s_way[j] = j0; }
            if (mv < bestv) { bestv = mv; bestj = j; }
          }
          ud_wave_min_pair(bestv, bestj);                    // equal reduced costs: the lowest column
          if (bestj == 0x7FFFFFFF) break;
          const double delta = bestv;
          for (int j = lane; j < nb; j += 64) {
            if (s_used[j]) { s_u[s_p[j]] += delta; s_v[j] -= delta; }
            else s_minv[j] -= delta;
          }
          if (lane == 0) s_u[i] += delta;
          j0 = bestj;
          __syncthreads();
          if (s_p[j0] < 0) { found = true; break; }
        }
        if (!found) { st |= UD_TM_ST_INTERNAL; __syncthreads(); continue; }
        if (lane == 0) {
          for (int it = 0; it <= nb && j0 >= 0; ++it) {
            const int j1 = s_way[j0];
            s_p[j0] = j1 < 0 ? i : s_p[j1];
            j0 = j1;
          }
        }
        __syncthreads();
      }
      for (int j = lane; j < nb; j += 64) {
        const int i = s_p[j];
        if (i < 0) continue;
        const double d = ud_dist_xy(rx[ri[i]], ry[ri[i]], cx[ci[j]], cy[ci[j]]);
        if (d < th) {
          const int o = obj_rows ? ri[i] : ci[j], h = obj_rows ? ci[j] : ri[i];
          s_omatch[o] = h;
          s_od[o] = d;
          s_hcl[h] = 1;
        }
      }
      __syncthreads();
    }

    // ---- 4: events and counters
    for (int o = lane; o < no; o += 64) {
      const int inst = s_oinst[o], h = s_omatch[o];
      int type = 0;
      if (h >= 0) {
        const int id = s_hid[h], prev = s_m[inst];
        type = (prev != 0 && prev != id) ? 2 : 1;
        s_m[inst] = id;
        if (type == 1) ++n_match; else ++n_switch;
      } else {
        ++n_miss;
      }
      s_app[inst] += 1;
      if (s_first[inst] == 0xFFFF) s_first[inst] = (unsigned short)fidx;
      unsigned short fl = s_flags[inst];
      if (h >= 0) {
        s_trk[inst] += 1;
        if (!(fl & kEver)) { fl |= kEver; s_tid[inst] = (unsigned short)(fidx - s_first[inst]); }
        if (fl & kGap) { s_frag[inst] += 1; fl &= ~kGap; }
        s_run[inst] = 0;
      } else {
        const unsigned short run = s_run[inst] + 1;
        s_run[inst] = run;
        if (run > s_maxrun[inst]) s_maxrun[inst] = run;
        if (fl & kEver) fl |= kGap;
      }
      s_flags[inst] = fl;
      const long long grow = g0 + s_orow[o];
      if (events) {
        a.ev_type[grow] = type;
        a.ev_row[grow] = h >= 0 ? (int)(p0 + s_hrow[h]) : -1;
      }
      if (k < 0 && type == 1) a.mscore[grow] = a.hscore[p0 + s_hrow[h]];
    }
    int pairs = 0;
    for (int c0 = 0; c0 < nh; c0 += 64) pairs += __popcll(__ballot(c0 + lane < nh && s_hcl[c0 + lane]));
    fp += nh - pairs;
    for (int o = 0; o < no; ++o)
      if (s_omatch[o] >= 0) dist_sum = dist_sum + s_od[o];   // GT row order
    __syncthreads();
  }

  int mt = 0, ml = 0, frag = 0, tid = 0, lgd = 0, ninst = 0;
  for (int i = lane; i < ic; i += 64) {
    const int app = s_app[i];
    if (!app) continue;
    const double ratio = (double)s_trk[i] / (double)app;
    mt += ratio >= 0.8;
    ml += ratio < 0.2;
    frag += s_frag[i];
    if (s_flags[i] & kEver) { tid += s_tid[i]; lgd += s_maxrun[i]; ++ninst; }
  }
  const int vals[kParts] = {frames, objects, ud_wave_sum_i(n_match), ud_wave_sum_i(n_switch), fp, ud_wave_sum_i(n_miss),
                            ud_wave_sum_i(mt), ud_wave_sum_i(ml), ud_wave_sum_i(frag), ud_wave_sum_i(tid), ud_wave_sum_i(lgd),
                            ud_wave_sum_i(ninst)};
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kParts; ++i) part[i] = vals[i];
    a.part_d[q] = dist_sum;
  }
  if (st) atomicOr(a.status, st);
}

// ---- thresholds ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tm_keys(const double* __restrict__ mscore, long long G, unsigned long long* __restrict__ keys) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  const double s = mscore[g];
  keys[g] = s == s ? ud_desc_bits(s + 0.0) : ~0ull;
}

__global__ __launch_bounds__(256) void k_tm_thresholds(Ptrs a, Params prm) {
  __shared__ int s_wsum[4];
  __shared__ long long s_P;
  const int t = blockIdx.x, c = prm.cls_of[t], tid = threadIdx.x;
  const long long base = prm.seg[t], room = prm.seg[t + 1] - base;
  double* s = a.sorted + base;
  long long n = 0;
  int st = 0;
  for (long long i0 = 0; i0 < prm.G; i0 += 256) {          // the sorted order, this class's MATCH scores kept in order
    const long long i = i0 + tid;
    bool ok = false;
    double v = 0.0;
    if (i < prm.G) {
      const int g = a.order[i];
      if (g >= 0 && g < prm.G && a.gt_cls[g] == c) {
        v = a.mscore[g];
        ok = v == v;
      }
    }
    const UdBlockRank cr = ud_block_rank<4>(ok, s_wsum);
    if (ok) {
      const long long pos = n + cr.rank();
      if (pos < room) s[pos] = v;
      else st |= UD_TM_ST_RANGE;
    }
    n += cr.total;
    __syncthreads();
  }
  if (n > room) n = room;
  if (tid == 0) {
    long long P = 0;
    for (long long sc = 0; sc < prm.NS; ++sc) P += a.part_i[((sc * prm.T + t) * (prm.K + 1)) * kParts + kObjects];
    s_P = P;
    a.nscores[t] = n;
  }
  __syncthreads();                                         // also: the segment is written
  if (tid < prm.K) {
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double P = (double)s_P, r = a.recall[tid];
    double theta = nan;
    if (n > 0 && s_P > 0 && !(r > (double)n / P)) {
      if (r <= 1.0 / P) {
        theta = s[0];
      } else {
        long long lo = 0, hi = n - 1;                      // the last knot at or below r
        while (lo < hi) {
          const long long mid = (lo + hi + 1) / 2;
          if ((double)(mid + 1) / P <= r) lo = mid; else hi = mid - 1;
        }
        const double rj = (double)(lo + 1) / P;
        if (rj == r || lo == n - 1) theta = s[lo];
        else theta = s[lo] + ((s[lo + 1] - s[lo]) / ((double)(lo + 2) / P - rj)) * (r - rj);
      }
    }
    a.thresholds[t * prm.K + tid] = theta;
  }
  if (st) atomicOr(a.status, st);
}

// ---- per (class, pass): the scenes' partials in scene order ------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_tm_finalize(Ptrs a, Params prm) {
  const int i = blockIdx.x * 64 + threadIdx.x, passes = prm.K + 1;
  if (i >= prm.T * passes) return;
  const int t = i / passes, pass = i - t * passes;
  long long sums[kParts] = {};
  double d = 0.0;
  for (long long sc = 0; sc < prm.NS; ++sc) {
    const long long q = (sc * prm.T + t) * passes + pass;
#pragma unroll
    for (int j = 0; j < kParts; ++j) sums[j] += a.part_i[q * kParts + j];
    d = d + a.part_d[q];
  }
#pragma unroll
  for (int j = 0; j < kParts; ++j) a.counts[(long long)i * kParts + j] = sums[j];
  a.dist[i] = d;
  const double theta = pass ? a.thresholds[t * prm.K + pass - 1] : 0.0;
  a.valid[i] = theta == theta;
}

struct Plan {
  int T, cap, ic, nblk;
  long long NQ, slots;
};

bool plan_of(const UdTrackMetricCfg& cfg, Plan& p) {
  if (cfg.num_classes < 1 || cfg.num_classes > UD_NUS_MAX_CLASSES) return false;
  if (cfg.num_thresholds < 1 || cfg.num_thresholds > UD_TM_MAX_THRESHOLDS) return false;
  if (cfg.num_scenes < 1 || cfg.num_scenes > (1 << 20) || cfg.num_samples < 1 || cfg.num_frames < 0) return false;
  if (cfg.num_rows < 0 || cfg.num_rows > 0x7FFFFFFFll || cfg.num_gt < 0 || cfg.num_gt > 0x7FFFFFFFll) return false;
  if (cfg.max_frame_rows < 0 || cfg.max_frame_rows > kCap) return false;
  if (cfg.max_instances < 0 || cfg.max_instances > UD_TM_MAX_INSTANCES) return false;
  if (cfg.max_scene_rows < 0 || cfg.max_scene_rows > cfg.num_rows) return false;
  p.T = 0;
  for (int c = 0; c < cfg.num_classes; ++c) p.T += cfg.track_class[c] != 0;
  if (p.T < 1) return false;
  p.cap = std::max(64, (cfg.max_frame_rows + 63) / 64 * 64);
  p.ic = std::max(8, (cfg.max_instances + 7) / 8 * 8);
  p.nblk = ud_div_up(std::max<long long>(cfg.num_gt, 1), kRsChunk);
  p.NQ = cfg.num_scenes * p.T * (cfg.num_thresholds + 1);
  p.slots = cfg.max_scene_rows + 1;
  return p.NQ <= 0x7FFFFFFFll / kParts;
}

struct Scratch {
  double *acc_sum, *hscore, *mscore, *sorted, *part_d;
  int *acc_cnt, *order, *part_i;
  unsigned long long *keys, *ktmp[2];
  int32_t* vtmp[2];
  unsigned *hist, *dtot;
};

size_t carve(const UdTrackMetricCfg& cfg, const Plan& p, void* ws, size_t bytes, Scratch* s) {
  UdArena ar(ws, bytes);
  const size_t G = (size_t)std::max<long long>(cfg.num_gt, 1), P = (size_t)std::max<long long>(cfg.num_rows, 1);
  Scratch x;
  x.acc_sum = ar.take<double>((size_t)cfg.num_scenes * p.slots);
  x.acc_cnt = ar.take<int>((size_t)cfg.num_scenes * p.slots);
  x.hscore = ar.take<double>(P);
  x.mscore = ar.take<double>(G);
  x.sorted = ar.take<double>(G);
  x.part_d = ar.take<double>((size_t)p.NQ);
  x.part_i = ar.take<int>((size_t)p.NQ * kParts);
  x.order = ar.take<int>(G);
  x.keys = ar.take<unsigned long long>(G);
  x.ktmp[0] = ar.take<unsigned long long>(G);
  x.ktmp[1] = ar.take<unsigned long long>(G);
  x.vtmp[0] = ar.take<int32_t>(G);
  x.vtmp[1] = ar.take<int32_t>(G);
  x.hist = ar.take<unsigned>((size_t)kRsBinsMax * p.nblk);
  x.dtot = ar.take<unsigned>(kRsBinsMax);
  if (s) *s = x;
  return ar.used;
}

}  // namespace

extern "C" {

size_t ud_track_metric_workspace_bytes(const UdTrackMetricCfg* cfg) {
  Plan p;
  if (!cfg || !plan_of(*cfg, p)) return 0;
  return carve(*cfg, p, nullptr, 0, nullptr);
}

int ud_track_metric(const double* pred_rec, const int32_t* pred_cls, const int32_t* track_id, const int64_t* row_start,
                    const int64_t* row_count, const double* gt_xyz, const int32_t* gt_cls, const int32_t* gt_num_pts,
                    const uint8_t* gt_keep, const int32_t* gt_inst, const int64_t* gt_off, const double* ego,
                    const int64_t* frame_sample, const int64_t* scene_off, const double* recall,
                    const UdTrackMetricCfg* cfg_host, int64_t* counts, double* dist_sum, int32_t* valid, double* thresholds,
                    int64_t* num_scores, int32_t* events_type, int32_t* events_row, int32_t* status, void* workspace,
                    size_t workspace_bytes, ud_stream_t stream_) {
  if (!cfg_host) return UD_ERR_INVALID_ARG;
  const UdTrackMetricCfg& cfg = *cfg_host;
  Plan p;
  if (!plan_of(cfg, p)) return UD_ERR_INVALID_ARG;
  if (!(cfg.dist_th_tp > 0.0) || !std::isfinite(cfg.dist_th_tp) || cfg.max_boxes_per_sample < 1) return UD_ERR_INVALID_ARG;
  if (cfg.events_pass < -2 || cfg.events_pass >= cfg.num_thresholds) return UD_ERR_INVALID_ARG;
  if (cfg.events_pass != -2 && (!events_type || !events_row)) return UD_ERR_INVALID_ARG;
  if (!row_start || !row_count || !gt_off || !ego || !frame_sample || !scene_off || !recall || !counts || !dist_sum ||
      !valid || !thresholds || !num_scores || !status)
    return UD_ERR_INVALID_ARG;
  if (cfg.num_rows > 0 && (!pred_rec || !pred_cls || !track_id)) return UD_ERR_INVALID_ARG;
  if (cfg.num_gt > 0 && (!gt_xyz || !gt_cls || !gt_num_pts || !gt_keep || !gt_inst)) return UD_ERR_INVALID_ARG;
  Params prm = {};
  prm.C = cfg.num_classes;
  prm.T = p.T;
  prm.K = cfg.num_thresholds;
  prm.cap = p.cap;
  prm.inst_cap = p.ic;
  prm.max_boxes = cfg.max_boxes_per_sample;
  prm.events_pass = cfg.events_pass;
  prm.P = cfg.num_rows;
  prm.G = cfg.num_gt;
  prm.S = cfg.num_samples;
  prm.F = cfg.num_frames;
  prm.NS = cfg.num_scenes;
  prm.slots = p.slots;
  prm.dist_th = cfg.dist_th_tp;
  prm.big = (double)kCap * cfg.dist_th_tp + 1.0;             // above the total of any kCap admissible pairs
  int t = 0;
  long long at = 0;
  for (int c = 0; c < cfg.num_classes; ++c) {
    prm.tracked[c] = cfg.track_class[c] != 0;
    prm.range[c] = cfg.class_range[c];
    if (!prm.tracked[c]) continue;
    if (!(cfg.class_range[c] >= 0.0) || cfg.class_gt[c] < 0 || cfg.class_gt[c] > cfg.num_gt) return UD_ERR_INVALID_ARG;
    prm.cls_of[t] = c;
    prm.seg[t] = at;
    at += cfg.class_gt[c];
    ++t;
  }
  prm.seg[t] = at;
  if (at > std::max<long long>(cfg.num_gt, 1)) return UD_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < ud_track_metric_workspace_bytes(cfg_host)) return UD_ERR_WORKSPACE;
  Scratch s;
  carve(cfg, p, workspace, workspace_bytes, &s);
  const size_t lds = walk_lds_bytes(p.cap, p.ic);
  static UdDeviceOnce once;
  if (const int e = ud_allow_dyn_lds(once, (int)walk_lds_bytes(kCap, UD_TM_MAX_INSTANCES), k_tm_walk)) return e;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("track_metric", stream);

  Ptrs a = {};
  a.rec = pred_rec, a.cls = pred_cls, a.track_id = track_id;
  a.row_start = (const long long*)row_start, a.row_count = (const long long*)row_count;
  a.gt_xyz = gt_xyz, a.gt_cls = gt_cls, a.gt_npts = gt_num_pts, a.gt_keep = gt_keep, a.gt_inst = gt_inst;
  a.gt_off = (const long long*)gt_off, a.ego = ego;
  a.frame_sample = (const long long*)frame_sample, a.scene_off = (const long long*)scene_off, a.recall = recall;
  a.acc_sum = s.acc_sum, a.acc_cnt = s.acc_cnt, a.hscore = s.hscore, a.mscore = s.mscore, a.sorted = s.sorted;
  a.order = s.order, a.part_i = s.part_i, a.part_d = s.part_d;
  a.thresholds = thresholds, a.nscores = (long long*)num_scores, a.counts = (long long*)counts, a.dist = dist_sum;
  a.valid = valid, a.ev_type = cfg.events_pass != -2 ? events_type : nullptr, a.ev_row = events_row, a.status = status;

  if (cfg.num_gt > 0) {
    UD_HIP_TRY(hipMemsetAsync(s.mscore, 0xFF, (size_t)cfg.num_gt * sizeof(double), stream));       // NaN: no MATCH
    if (a.ev_type) {
      UD_HIP_TRY(hipMemsetAsync(events_type, 0xFF, (size_t)cfg.num_gt * sizeof(int32_t), stream));  // -1: the row is not kept
      UD_HIP_TRY(hipMemsetAsync(events_row, 0xFF, (size_t)cfg.num_gt * sizeof(int32_t), stream));
    }
  }
  k_tm_scores<<<(unsigned)cfg.num_scenes, kScoreThreads, 0, stream>>>(a, prm);
  UD_LAUNCH_CHECK();
  k_tm_walk<<<(unsigned)(cfg.num_scenes * p.T), 64, lds, stream>>>(a, prm, 0);
  UD_LAUNCH_CHECK();
  if (cfg.num_gt > 0) {
    k_tm_keys<<<ud_div_up(cfg.num_gt, 256), 256, 0, stream>>>(s.mscore, cfg.num_gt, s.keys);
    UD_LAUNCH_CHECK();
    if (const int e = rs_sort_pairs<unsigned long long>(s.keys, (int)cfg.num_gt, 64, s.order, s.ktmp, s.vtmp, s.hist, s.dtot,
                                                        stream))
      return e;
  }
  k_tm_thresholds<<<p.T, 256, 0, stream>>>(a, prm);
  UD_LAUNCH_CHECK();
  k_tm_walk<<<(unsigned)(cfg.num_scenes * p.T * cfg.num_thresholds), 64, lds, stream>>>(a, prm, 1);
  UD_LAUNCH_CHECK();
  k_tm_finalize<<<ud_div_up((long long)p.T * (cfg.num_thresholds + 1), 64), 64, 0, stream>>>(a, prm);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

}  // extern "C"
