// Multi-object tracking of the validation predictions: CenterPoint's greedy, velocity-compensated centre
// association over the evaluator's global-frame rows, all scenes in ONE launch.
//
//   k_track_scenes : one 1024-thread workgroup per scene, the scene's frames walked in order inside it.  Per frame:
//     A  the live tracks coast (ct += v * dt); one thread per row: the candidate test, ordered compaction, (descending score,
//        row) keys, a bitonic sort of (key, row) pairs in LDS (lds_sort.h; the row in the high bits of the second word, so
//        equal scores order by row whatever the classes);
//     B  one wave per class: the class's candidates in order; per candidate the 64 lanes scan the live tracks of that class
//        (d2 = dx * dx + dy * dy, no square root), a lexicographic (d2, slot) minimum across the wave (ud_wave_min_pair), the
//        accept test, and the owner lane of the winning slot retires it.  Classes never share a track, so the waves do not
//        interact;
//     C  one thread per candidate: the matched track's id and hits (or the next ids, by a prefix count of the unmatched),
//        barrier, then the new generation and the two outputs are written.
//
// The track list is never compacted.  The issue's list -- this frame's candidates in order, then the unclaimed old tracks in
// their old order -- is always sorted by (age, candidate position in the frame that last saw the track), so a track stays
// where its frame put it: generation (frame % max_age), position = candidate rank.  A claimed track is dead from then on (its
// successor is the candidate's new entry); a generation is overwritten exactly when its survivors would reach max_age.
// "Lowest slot" is "lowest (age, position)", which is the order the lanes scan in.
//
// LDS (dynamic, by max_age; 160 KiB per CU): centres 2 x f64 and class u8 per slot (17 B x max_age x 1024), the frame's keys
// u64[1024], rows and matches i32[1024] each: 67 KiB at max_age 3, 152 KiB at max_age 8; one workgroup per CU either way (76
// VGPRs at 16 waves per workgroup).  Velocity, id and hits are touched once per frame and live in the scene's slice of the
// workspace (24 B per slot).
//
// No inter-workgroup communication, no spinning, no floating-point atomics; the only atomic is the OR into *status.
#include "ud_common.h"
#include "ud_prof.h"
#include "lds_sort.h"
#include <cmath>

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kGen = UD_NUS_MAX_BOXES;            // slots of one generation: the candidates of one frame
constexpr int kMaxAge = UD_TRACK_MAX_AGE;
constexpr int kDead = 0xFF;
constexpr unsigned long long kPadKey = ~0ull;
constexpr int kClsBits = 4, kClsMask = (1 << kClsBits) - 1;
static_assert(kGen == kThreads, "one thread per row of a frame");
static_assert(UD_NUS_MAX_CLASSES <= kWaves && UD_NUS_MAX_CLASSES <= kClsMask, "one wave per class; the class fits its bits");

struct Params {
  int num_classes, max_age;
  double score_threshold;
  double max_dist2[UD_NUS_MAX_CLASSES];
  unsigned char track_class[16];
  long long P, S, F;
};

__host__ __device__ inline size_t lds_bytes(int max_age) {
  return (size_t)max_age * kGen * (2 * sizeof(double) + 1) + kGen * (sizeof(unsigned long long) + 2 * sizeof(int));
}

// the workspace slice of one scene: vx[cap] vy[cap] f64, id[cap] hits[cap] i32, cap = max_age * kGen
__host__ __device__ inline size_t scene_bytes(int max_age) { return (size_t)max_age * kGen * 24; }

__global__ __launch_bounds__(kThreads) void k_track_scenes(
    const double* __restrict__ rec, const int* __restrict__ cls, const long long* __restrict__ row_start,
    const long long* __restrict__ row_count, const long long* __restrict__ frame_sample,
    const long long* __restrict__ scene_off, const double* __restrict__ frame_dt, Params prm, int* __restrict__ track_id,
    int* __restrict__ track_hits, int* __restrict__ status, char* __restrict__ ws) {
  extern __shared__ double s_dyn[];
  __shared__ int s_wsum[kWaves];
  __shared__ int s_ngen[kMaxAge];
  const int cap = prm.max_age * kGen;
  double* s_ctx = s_dyn;
  double* s_cty = s_ctx + cap;
  unsigned long long* s_key = reinterpret_cast<unsigned long long*>(s_cty + cap);
  int* s_row = reinterpret_cast<int*>(s_key + kGen);          // sorted position -> row within the frame << 4 | class: the
                                                              // sort's second key, so equal scores order by row alone
  int* s_match = s_row + kGen;                                // sorted position -> age * kGen + position of the track, -1
  unsigned char* s_cls = reinterpret_cast<unsigned char*>(s_match + kGen);
  char* slice = ws + (size_t)blockIdx.x * scene_bytes(prm.max_age);
  double* w_vx = reinterpret_cast<double*>(slice);
  double* w_vy = w_vx + cap;
  int* w_id = reinterpret_cast<int*>(w_vy + cap);
  int* w_hits = w_id + cap;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < kMaxAge) s_ngen[tid] = 0;
  int next_id = 0, st = 0;
  long long f0 = scene_off[blockIdx.x], f1 = scene_off[blockIdx.x + 1];
  if (f0 < 0 || f1 > prm.F || f1 < f0) { st |= UD_TRACK_ST_RANGE; f1 = f0; }
  __syncthreads();

  for (long long fi = f0; fi < f1; ++fi) {
    const int fno = (int)((fi - f0) % prm.max_age);           // this frame's generation; the frame before it is fno - 1
    const long long sample = frame_sample[fi];
    const double dt = frame_dt[fi];
    long long start = 0, cnt = 0;
    if (sample < 0 || sample >= prm.S) {
      st |= UD_TRACK_ST_RANGE;
    } else {
      start = row_start[sample];
      cnt = row_count[sample];
      if (cnt > kGen) { st |= UD_TRACK_ST_COUNT; cnt = 0; }
      if (cnt < 0 || start < 0 || start > prm.P - cnt) { st |= UD_TRACK_ST_RANGE; cnt = 0; }
    }

    // ---- A: candidates, their order, and the coast of the live tracks
    bool ok = false;
    double score = 0.0;
    int c = -1;
    if (tid < cnt) {
      const long long row = start + tid;
      c = cls[row];
      if (c >= 0 && c < prm.num_classes && prm.track_class[c]) {
        const double* r = rec + row * UD_NUS_PRED_COLS;
        score = r[9];
        const bool finite = isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]) && isfinite(r[7]) && isfinite(r[8]) &&
                            isfinite(score);
        if (!finite) st |= UD_TRACK_ST_NONFINITE;
        ok = finite && score >= prm.score_threshold;
      }
    }
    for (int slot = tid; slot < cap; slot += kThreads) {
      const int g = slot / kGen;
      if ((slot - g * kGen) < s_ngen[g] && s_cls[slot] != kDead) {
        s_ctx[slot] = s_ctx[slot] + w_vx[slot] * dt;
        s_cty[slot] = s_cty[slot] + w_vy[slot] * dt;
      }
    }
    const UdBlockRank cr = ud_block_rank<kWaves>(ok, s_wsum);          // its barrier also stands behind the coast
    const int ncand = cr.total;
    int npow2 = 1;
    while (npow2 < ncand) npow2 <<= 1;
    if (ok) {
      const int pos = cr.rank();
      s_key[pos] = ud_desc_bits(score + 0.0);
      s_row[pos] = (tid << kClsBits) | c;
    }
    if (tid >= ncand && tid < npow2) { s_key[tid] = kPadKey; s_row[tid] = 0x7FFFFFFF; }
    __syncthreads();
    __builtin_assume(npow2 <= kThreads);                               // one element per thread: the sort's loop runs once
    ud_bitonic_sort<kThreads>(s_key, s_row, npow2);

    // ---- B: greedy match, one wave per class
    if (wave < prm.num_classes && prm.track_class[wave]) {
      const double md2 = prm.max_dist2[wave];
      const int ages = (int)min((long long)prm.max_age, fi - f0);      // generations that exist before this frame
      for (int c0 = 0; c0 < ncand; c0 += 64) {
        const int i = c0 + lane;
        unsigned long long mine = __ballot(i < ncand && (s_row[i] & kClsMask) == wave);
        while (mine) {
          const int ci = c0 + __builtin_ctzll(mine);
          mine &= mine - 1;
          const long long row = start + (s_row[ci] >> kClsBits);
          const double cx = rec[row * UD_NUS_PRED_COLS], cy = rec[row * UD_NUS_PRED_COLS + 1];
          double best = INFINITY;
          int bslot = 0x7FFFFFFF;
          for (int a = 0; a < ages; ++a) {
            const int g = (fno - 1 - a + 2 * prm.max_age) % prm.max_age;
            const int n = s_ngen[g];
            for (int p = lane; p < n; p += 64) {
              const int slot = g * kGen + p;
              if (s_cls[slot] == wave) {
                const double dx = cx - s_ctx[slot], dy = cy - s_cty[slot];
                const double d2 = dx * dx + dy * dy;
                if (d2 < best) { best = d2; bslot = a * kGen + p; }
              }
            }
          }
          ud_wave_min_pair(best, bslot);
          const bool hit = bslot != 0x7FFFFFFF && best <= md2;
          if (hit) {
            const int a = bslot / kGen, p = bslot - a * kGen;
            const int g = (fno - 1 - a + 2 * prm.max_age) % prm.max_age;
            if (lane == (p & 63)) s_cls[g * kGen + p] = kDead;         // the lane that scans this slot retires it
          }
          if (lane == 0) s_match[ci] = hit ? bslot : -1;
        }
      }
    }
    __syncthreads();

    // ---- C: ids and hits, then the new generation
    const bool cand = tid < ncand;
    int m = -1, id = 0, hits = 1;
    if (cand) {
      m = s_match[tid];
      if (m >= 0) {
        const int a = m / kGen, p = m - a * kGen;
        const int g = (fno - 1 - a + 2 * prm.max_age) % prm.max_age;
        id = w_id[g * kGen + p];
        hits = a == 0 ? w_hits[g * kGen + p] + 1 : 1;                  // a rematch after a miss restarts at 1
      }
    }
    const UdBlockRank fr = ud_block_rank<kWaves>(cand && m < 0, s_wsum);   // its barrier: every read of the old generation is done
    if (cand) {
      if (m < 0) id = next_id + fr.rank() + 1;
      const int packed = s_row[tid];
      const long long row = start + (packed >> kClsBits);
      const double* r = rec + row * UD_NUS_PRED_COLS;
      const int slot = fno * kGen + tid;
      s_ctx[slot] = r[0];
      s_cty[slot] = r[1];
      s_cls[slot] = (unsigned char)(packed & kClsMask);
      w_vx[slot] = r[7];
      w_vy[slot] = r[8];
      w_id[slot] = id;
      w_hits[slot] = hits;
      track_id[row] = id;
      track_hits[row] = hits;
    }
    if (tid == 0) s_ngen[fno] = ncand;
    next_id += fr.total;
    __syncthreads();
  }
  if (st) atomicOr(status, st);
}

bool sizes_ok(long long num_scenes, int max_age) {
  return num_scenes >= 1 && num_scenes <= 0x7FFFFFFFll / 2 && max_age >= 1 && max_age <= kMaxAge;
}

}  // namespace

extern "C" {

size_t ud_track_workspace_bytes(int64_t num_scenes, int max_age) {
  if (!sizes_ok(num_scenes, max_age)) return 0;
  return (size_t)num_scenes * scene_bytes(max_age);
}

int ud_track_scenes(const double* rec, const int32_t* cls, const int64_t* row_start, const int64_t* row_count,
                    const int64_t* frame_sample, const int64_t* scene_off, const double* frame_dt,
                    const UdTrackCfg* cfg_host, int32_t* track_id, int32_t* track_hits, int32_t* status, void* workspace,
                    size_t workspace_bytes, ud_stream_t stream_) {
  if (!cfg_host) return UD_ERR_INVALID_ARG;
  const UdTrackCfg& cfg = *cfg_host;
  if (!sizes_ok(cfg.num_scenes, cfg.max_age)) return UD_ERR_INVALID_ARG;
  if (cfg.num_classes < 1 || cfg.num_classes > UD_NUS_MAX_CLASSES) return UD_ERR_INVALID_ARG;
  if (cfg.num_rows < 0 || cfg.num_rows > 0x7FFFFFFFll || cfg.num_samples < 1 || cfg.num_frames < 0) return UD_ERR_INVALID_ARG;
  if (std::isnan(cfg.score_threshold)) return UD_ERR_INVALID_ARG;
  if (!row_start || !row_count || !frame_sample || !scene_off || !frame_dt || !track_id || !track_hits || !status)
    return UD_ERR_INVALID_ARG;
  if (cfg.num_rows > 0 && (!rec || !cls)) return UD_ERR_INVALID_ARG;
  Params prm;
  prm.num_classes = cfg.num_classes;
  prm.max_age = cfg.max_age;
  prm.score_threshold = cfg.score_threshold;
  prm.P = cfg.num_rows;
  prm.S = cfg.num_samples;
  prm.F = cfg.num_frames;
  for (int c = 0; c < UD_NUS_MAX_CLASSES; ++c) {
    const bool on = c < cfg.num_classes && cfg.track_class[c] != 0;
    if (on && !(cfg.max_dist[c] >= 0.0)) return UD_ERR_INVALID_ARG;       // NaN or negative
    prm.track_class[c] = on ? 1 : 0;
    prm.max_dist2[c] = on ? cfg.max_dist[c] * cfg.max_dist[c] : 0.0;
  }
  prm.track_class[15] = 0;
  if (!workspace || workspace_bytes < ud_track_workspace_bytes(cfg.num_scenes, cfg.max_age)) return UD_ERR_WORKSPACE;
  static UdDeviceOnce once;
  if (const int e = ud_allow_dyn_lds(once, (int)lds_bytes(kMaxAge), k_track_scenes)) return e;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("track_scenes", stream);
  // a row that is no candidate of any listed frame reads 0 in both outputs
  if (cfg.num_rows > 0) {
    UD_HIP_TRY(hipMemsetAsync(track_id, 0, (size_t)cfg.num_rows * sizeof(int32_t), stream));
    UD_HIP_TRY(hipMemsetAsync(track_hits, 0, (size_t)cfg.num_rows * sizeof(int32_t), stream));
  }
  k_track_scenes<<<(unsigned)cfg.num_scenes, kThreads, lds_bytes(cfg.max_age), stream>>>(
      rec, cls, (const long long*)row_start, (const long long*)row_count, (const long long*)frame_sample,
      (const long long*)scene_off, frame_dt, prm, track_id, track_hits, status, (char*)workspace);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

}  // extern "C"
