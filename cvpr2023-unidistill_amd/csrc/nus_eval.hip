// nuScenes detection metric, detection_cvpr_2019: the devkit's DetectionEval behind the reference's
// validation_epoch_end (nuscenes_multimodal.py:336-393, eval_utils.py), in float64, restated by tests/nus_eval_reference.py.
//
//   k_nus_pred_prep   one thread per prediction of a batch: LiDAR -> global box, velocity, yaw, attribute
//   k_nus_match       one workgroup per sample: filters; the sample's kept predictions ranked in LDS by
//                     (class, descending score, descending box); wave w matches them greedily at dist_th[w] (the taken
//                     mask lives in the lanes' registers: lane l owns GT l, l + 64, ...); the dist_th_tp wave writes the
//                     matched GT and the five TP errors; per prediction the global sort key
//   rs_sort_pairs     stable radix sort (radix_sort.h) of (class, descending score) over the (sample, box) positions
//                     taken in reverse: equal keys come out in descending (sample, box) order, the documented tie rule
//   k_nus_tp_scan     one workgroup per (class, threshold): inclusive integer cumsum of the TP flags in sorted order
//   k_nus_err_scan    one workgroup per (class, error): NaN-aware running sum / count over the matches, compacted to the
//                     match list with its confidences
//   k_nus_curves      one workgroup per class: numpy.interp of precision and confidence (4 thresholds) and of the errors
// Float64 throughout, no contraction (-ffp-contract=off): every expression is evaluated as the oracle writes it.
#include "ud_common.h"
#include "ud_prof.h"
#include "lds_sort.h"
#include "radix_sort.h"

namespace {

constexpr int kMaxBoxes = UD_NUS_MAX_BOXES;
constexpr int kCols = UD_NUS_PRED_COLS, kGtCols = UD_NUS_GT_COLS, kPts = UD_NUS_POINTS;
constexpr int kErrs = 5;
constexpr int kSortBits = 36;                 // 4 class bits above 32 score bits
constexpr double kPi = 3.141592653589793;     // numpy.pi

struct AttrTab {
  int moving[UD_NUS_MAX_CLASSES], still[UD_NUS_MAX_CLASSES];   // attribute id per class when speed > 0.2 / otherwise
};

__global__ __launch_bounds__(256) void k_nus_pred_prep(const float* __restrict__ boxes, int64_t n, int ncol,
                                                       const float* __restrict__ scores,
                                                       const int64_t* __restrict__ labels,
                                                       const int32_t* __restrict__ batch_off, int B,
                                                       const double* __restrict__ l2g, int C, AttrTab tab,
                                                       double* __restrict__ rec, int32_t* __restrict__ cls,
                                                       int32_t* __restrict__ attr, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int b = 0;
  while (b + 1 < B && i >= batch_off[b + 1]) ++b;
  const double* M = l2g + 16 * b;
  const float* bx = boxes + i * ncol;
  const double x = bx[0], y = bx[1], z = bx[2], rot = bx[6];
  double* r = rec + i * kCols;
  r[0] = M[0] * x + M[1] * y + M[2] * z + M[3];
  r[1] = M[4] * x + M[5] * y + M[6] * z + M[7];
  r[2] = M[8] * x + M[9] * y + M[10] * z + M[11];
  r[3] = (double)bx[4];                                   // wlh = (dy, dx, dz)
  r[4] = (double)bx[3];
  r[5] = (double)bx[5];
  const double c = cos(rot), s = sin(rot);
  r[6] = atan2(M[4] * c + M[5] * s, M[0] * c + M[1] * s);
  double vx = __builtin_nan(""), vy = vx;
  if (ncol >= 9) {
    const double ux = bx[7], uy = bx[8];
    vx = M[0] * ux + M[1] * uy;
    vy = M[4] * ux + M[5] * uy;
  }
  r[7] = vx;
  r[8] = vy;
  r[9] = (double)scores[i];
  const int64_t lab = labels[i] - 1;
  int k = -1, a = -1;
  if (lab >= 0 && lab < C) {
    k = (int)lab;
    a = sqrt(vx * vx + vy * vy) > 0.2 ? tab.moving[k] : tab.still[k];   // a NaN velocity takes the second branch
  } else {
    atomicOr(status, UD_NUS_ST_CLASS);
  }
  cls[i] = k;
  attr[i] = a;
}

// Python's float % (floored modulo), as numpy's remainder on float64
__device__ __forceinline__ double py_mod(double a, double p) {
  double m = fmod(a, p);
  if (m != 0.0) {
    if ((p < 0.0) != (m < 0.0)) m += p;
  } else {
    m = copysign(0.0, p);
  }
  return m;
}

__global__ __launch_bounds__(256) void k_nus_match(UdNusCfg cfg, UdNusEvalIo io, int64_t P,
                                                   unsigned long long* __restrict__ skey, double* __restrict__ err) {
  __shared__ double s_gx[kMaxBoxes], s_gy[kMaxBoxes];
  __shared__ int s_gc[kMaxBoxes];                          // class of a kept GT, -1 otherwise
  __shared__ unsigned long long s_key[kMaxBoxes];
  __shared__ short s_ord[kMaxBoxes];
  __shared__ int s_cnt[2][UD_NUS_MAX_CLASSES + 1];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int C = cfg.num_classes;
  const int64_t g0 = io.gt_off[s], p0 = io.pred_src[s], q0 = io.pred_off[s];
  const int ng = (int)(io.gt_off[s + 1] - g0), np_ = (int)(io.pred_off[s + 1] - q0);
  if (ng > kMaxBoxes || np_ > kMaxBoxes || ng < 0 || np_ < 0) {
    if (tid == 0) atomicOr(io.status, UD_NUS_ST_COUNT);
    return;
  }
  const double ex = io.ego[3 * s], ey = io.ego[3 * s + 1];
  if (tid < 2 * (UD_NUS_MAX_CLASSES + 1)) s_cnt[tid / (UD_NUS_MAX_CLASSES + 1)][tid % (UD_NUS_MAX_CLASSES + 1)] = 0;
  __syncthreads();
  for (int j = tid; j < ng; j += 256) {
    const double* g = io.gt_rec + (g0 + j) * kGtCols;
    const int c = io.gt_cls[g0 + j];
    bool keep = false;
    if (c >= 0 && c < C) {
      keep = io.gt_keep[g0 + j] != 0 && io.gt_num_pts[g0 + j] != 0 && ud_dist_xy(g[0], g[1], ex, ey) < cfg.class_range[c];
    } else {
      atomicOr(io.status, UD_NUS_ST_CLASS);
    }
    s_gx[j] = g[0];
    s_gy[j] = g[1];
    s_gc[j] = keep ? c : -1;
    if (keep) atomicAdd(&s_cnt[1][c], 1);
  }
  for (int i = tid; i < np_; i += 256) {
    const double* p = io.pred_rec + (p0 + i) * kCols;
    const int c = io.pred_cls[p0 + i];
    const bool keep = c >= 0 && c < C && ud_dist_xy(p[0], p[1], ex, ey) < cfg.class_range[c];
    const unsigned desc = ud_desc_bits((float)p[9]);
    s_key[i] = keep ? ((unsigned long long)c << 42) | ((unsigned long long)desc << 10) | (unsigned)(kMaxBoxes - 1 - i)
                    : (15ull << 42) | (unsigned)i;
    const int64_t q = q0 + i;
    skey[P - 1 - q] = keep ? ((unsigned long long)c << 32) | desc : (15ull << 32);
    if (keep) {
      atomicAdd(&s_cnt[0][c], 1);
    } else {
      for (int w = 0; w < 4; ++w) io.tp[w * P + q] = 0;
      io.match_gt[q] = -1;
    }
  }
  __syncthreads();
  for (int i = tid; i < np_; i += 256) {                 // rank = number of smaller keys (keys are distinct)
    const unsigned long long k = s_key[i];
    int r = 0;
    for (int j = 0; j < np_; ++j) r += s_key[j] < k;
    s_ord[r] = (short)i;
  }
  int nk = 0;
  for (int c = 0; c < C; ++c) nk += s_cnt[0][c];
  __syncthreads();
  if (tid < C) {
    if (s_cnt[0][tid]) atomicAdd(&io.counts[tid], s_cnt[0][tid]);
    if (s_cnt[1][tid]) atomicAdd(&io.counts[C + tid], s_cnt[1][tid]);
  }
  // wave wv = threshold wv; kept predictions come first in s_ord (the filtered ones carry class 15)
  const double th = cfg.dist_th[wv];
  const bool tp_wave = wv == cfg.dist_th_tp_index;
  unsigned taken = 0u;                                   // bit k: GT k * 64 + lane taken at this threshold
  const int nchunk = (ng + 63) / 64;
  for (int r = 0; r < nk; ++r) {
    const int i = s_ord[r];
    const double* p = io.pred_rec + (p0 + i) * kCols;
    const int c = io.pred_cls[p0 + i];
    const double px = p[0], py = p[1];
    double bd = __builtin_inf();
    int bj = 0x7fffffff;
    for (int k = 0; k < nchunk; ++k) {                   // first minimum of the lane's GT (ascending index)
      const int j = k * 64 + lane;
      if (j < ng && s_gc[j] == c && !((taken >> k) & 1u)) {
        const double d = ud_dist_xy(px, py, s_gx[j], s_gy[j]);
        if (d < bd) bd = d, bj = j;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                   // smallest distance, then smallest index
      const double od = __shfl_xor(bd, o);
      const int oj = __shfl_xor(bj, o);
      if (od < bd || (od == bd && oj < bj)) bd = od, bj = oj;
    }
    const bool match = bd < th;
    if (match && (bj & 63) == lane) taken |= 1u << (bj >> 6);
    const int64_t q = q0 + i;
    if (lane == 0) {
      io.tp[wv * P + q] = match ? 1 : 0;
      if (tp_wave) {
        io.match_gt[q] = match ? (int32_t)(g0 + bj) : -1;
        double e[kErrs];
        const double nan = __builtin_nan("");
        for (int m = 0; m < kErrs; ++m) e[m] = nan;
        if (match) {
          const double* g = io.gt_rec + (g0 + bj) * kGtCols;
          e[0] = bd;
          const double aw = g[3], al = g[4], ah = g[5], bw = p[3], bl = p[4], bh = p[5];
          if (!(aw > 0.0 && al > 0.0 && ah > 0.0 && bw > 0.0 && bl > 0.0 && bh > 0.0)) atomicOr(io.status, UD_NUS_ST_SIZE);
          const double mw = bw < aw ? bw : aw, ml = bl < al ? bl : al, mh = bh < ah ? bh : ah;
          const double va = aw * al * ah, vr = bw * bl * bh, inter = mw * ml * mh;
          e[1] = 1.0 - inter / (va + vr - inter);
          const double period = c == cfg.pi_period_class ? kPi : 2.0 * kPi;
          double diff = py_mod(g[6] - p[6] + period / 2.0, period) - period / 2.0;
          if (diff > kPi) diff = diff - 2.0 * kPi;
          e[2] = fabs(diff);
          const double dvx = p[7] - g[7], dvy = p[8] - g[8];
          e[3] = sqrt(dvx * dvx + dvy * dvy);
          const int ga = io.gt_attr[g0 + bj];
          e[4] = ga < 0 ? nan : 1.0 - (ga == io.pred_attr[p0 + i] ? 1.0 : 0.0);
        }
        for (int m = 0; m < kErrs; ++m) err[q * kErrs + m] = e[m];
      }
    }
  }
}

// class segment starts of the sorted order: classes in ascending id, kept predictions only
__device__ __forceinline__ int64_t class_base(const int32_t* counts, int c) {
  int64_t b = 0;
  for (int k = 0; k < c; ++k) b += counts[k];
  return b;
}

// inclusive scan over a 1024-thread workgroup; s_w: 16 slots
template <typename T>
__device__ __forceinline__ T block_scan(T v, T* s_w, T& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T a = __shfl_up(v, o);
    if (lane >= o) v += a;
  }
  if (lane == 63) s_w[wv] = v;
  __syncthreads();
  T pre = T(0);
  for (int w = 0; w < wv; ++w) pre += s_w[w];
  total = T(0);
  for (int w = 0; w < 16; ++w) total += s_w[w];
  __syncthreads();
  return pre + v;
}

__global__ __launch_bounds__(1024) void k_nus_tp_scan(const int32_t* __restrict__ sorted_j, const uint8_t* __restrict__ tp,
                                                      const int32_t* __restrict__ counts, int64_t P,
                                                      int32_t* __restrict__ tpc, int32_t* __restrict__ order) {
  __shared__ int s_w[16];
  const int c = blockIdx.x, w = blockIdx.y;
  const int64_t n = counts[c], base = class_base(counts, c);
  int carry = 0;
  for (int64_t k0 = 0; k0 < n; k0 += 1024) {
    const int64_t k = k0 + threadIdx.x;
    int v = 0;
    if (k < n) {
      const int64_t q = P - 1 - sorted_j[base + k];
      v = tp[w * P + q];
      if (w == 0) order[base + k] = (int32_t)q;
    }
    int total;
    const int inc = block_scan<int>(v, s_w, total);
    if (k < n) tpc[w * P + base + k] = carry + inc;
    carry += total;
  }
}

__global__ __launch_bounds__(1024) void k_nus_err_scan(const int32_t* __restrict__ sorted_j, const uint8_t* __restrict__ tp,
                                                       const int32_t* __restrict__ tpc, const double* __restrict__ err,
                                                       const double* __restrict__ pred_conf_rows,
                                                       const int32_t* __restrict__ counts, int64_t P, int wtp,
                                                       double* __restrict__ mconf, double* __restrict__ mcm,
                                                       int32_t* __restrict__ mtot) {
  __shared__ double s_ws[16];
  __shared__ int s_wc[16];
  const int c = blockIdx.x, m = blockIdx.y;
  const int64_t n = counts[c], base = class_base(counts, c);
  double carry = 0.0;
  int ccarry = 0;
  for (int64_t k0 = 0; k0 < n; k0 += 1024) {
    const int64_t k = k0 + threadIdx.x;
    bool matched = false;
    double v = 0.0;
    int64_t q = 0;
    if (k < n) {
      q = P - 1 - sorted_j[base + k];
      matched = tp[wtp * P + q] != 0;
      if (matched) v = err[q * kErrs + m];
    }
    const bool num = matched && v == v;
    double tot;
    int ctot;
    const double sum = block_scan<double>(num ? v : 0.0, s_ws, tot);
    const int cnt = block_scan<int>(num ? 1 : 0, s_wc, ctot);
    if (matched) {
      const int64_t rank = tpc[wtp * P + base + k] - 1;
      const double cs = carry + sum;
      const int cc = ccarry + cnt;
      mcm[m * P + base + rank] = cc != 0 ? cs / (double)cc : 0.0;
      if (m == 0) mconf[base + rank] = pred_conf_rows[q];
    }
    carry += tot;
    ccarry += ctot;
  }
  if (threadIdx.x == 0) mtot[c * kErrs + m] = ccarry;
}

// numpy.interp(x, xp, fp, left, right) for nondecreasing xp of n >= 1 entries (numpy/core/src/multiarray/compiled_base.c)
template <typename XP, typename FP>
__device__ double np_interp(double x, int64_t n, XP xp, FP fp, double left, double right) {
  if (x != x) return x;
  if (x > xp(n - 1)) return right;
  if (x < xp(0)) return left;
  int64_t lo = 0, hi = n;                                // j = last index with xp[j] <= x
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (x >= xp(mid)) lo = mid + 1;
    else hi = mid;
  }
  const int64_t j = lo - 1;
  if (j == n - 1) return fp(j);
  const double xj = xp(j);
  if (xj == x) return fp(j);
  const double xj1 = xp(j + 1), fj = fp(j), fj1 = fp(j + 1);
  const double slope = (fj1 - fj) / (xj1 - xj);
  double r = slope * (x - xj) + fj;
  if (r != r) {
    r = slope * (x - xj1) + fj1;
    if (r != r && fj == fj1) r = fj;
  }
  return r;
}

__global__ __launch_bounds__(128) void k_nus_curves(UdNusCfg cfg, const int32_t* __restrict__ order,
                                                    const int32_t* __restrict__ tpc, const double* __restrict__ conf_q,
                                                    const double* __restrict__ mconf, const double* __restrict__ mcm,
                                                    const int32_t* __restrict__ mtot, const int32_t* __restrict__ counts,
                                                    int64_t P, double* __restrict__ prec_out,
                                                    double* __restrict__ conf_out, double* __restrict__ err_out) {
  __shared__ double s_conf[kPts];
  const int c = blockIdx.x, t = threadIdx.x, C = cfg.num_classes, wtp = cfg.dist_th_tp_index;
  const int64_t n = counts[c], npos = counts[C + c], base = class_base(counts, c);
  const double dpos = (double)npos;
  int64_t nmatch = 0;
  for (int w = 0; w < 4; ++w) {
    const int32_t* cum = tpc + w * P + base;
    const int64_t ntp = n > 0 ? cum[n - 1] : 0;
    if (w == wtp) nmatch = npos > 0 ? ntp : 0;
    if (t < kPts) {
      double pr = 0.0, cf = 0.0;
      if (npos > 0 && ntp > 0) {
        const double x = cfg.rec_pts[t];
        auto rec = [&](int64_t j) { return (double)cum[j] / dpos; };
        auto pre = [&](int64_t j) { return (double)cum[j] / (double)(j + 1); };
        auto cnf = [&](int64_t j) { return conf_q[order[base + j]]; };
        pr = np_interp(x, n, rec, pre, pre(0), 0.0);
        cf = np_interp(x, n, rec, cnf, cnf(0), 0.0);
      }
      prec_out[(c * 4 + w) * kPts + t] = pr;
      conf_out[(c * 4 + w) * kPts + t] = cf;
      if (w == wtp) s_conf[t] = cf;
    }
  }
  __syncthreads();
  if (t >= kPts) return;
  for (int m = 0; m < kErrs; ++m) {
    double v = 1.0;                                      // no predictions, or every value NaN: ones
    if (nmatch > 0 && mtot[c * kErrs + m] > 0) {
      const double* mc = mconf + base;
      const double* cm = mcm + m * P + base;
      auto xp = [&](int64_t j) { return mc[nmatch - 1 - j]; };   // the match list reversed: ascending confidence
      auto fp = [&](int64_t j) { return cm[nmatch - 1 - j]; };
      v = np_interp(s_conf[t], nmatch, xp, fp, fp(0), fp(nmatch - 1));
    }
    err_out[(c * kErrs + m) * kPts + t] = v;
  }
}

struct EvalWs {
  unsigned long long* skey;
  unsigned long long* ktmp[2];
  int32_t* vtmp[2];
  unsigned* hist;
  unsigned* dtot;
  int32_t* sorted_j;
  int32_t* tpc;
  double* err;
  double* conf_q;
  double* mconf;
  double* mcm;
  int32_t* mtot;
  size_t total_bytes;
};

EvalWs carve_eval(void* ws, int64_t P, int C) {
  UdArena a(ws, (size_t)-1);
  EvalWs w;
  const size_t n = (size_t)(P > 0 ? P : 1);
  w.skey = a.take<unsigned long long>(n);
  w.ktmp[0] = a.take<unsigned long long>(n);
  w.ktmp[1] = a.take<unsigned long long>(n);
  w.vtmp[0] = a.take<int32_t>(n);
  w.vtmp[1] = a.take<int32_t>(n);
  w.hist = a.take<unsigned>((size_t)kRsBinsMax * ud_div_up((long long)n, kRsChunk));
  w.dtot = a.take<unsigned>(kRsBinsMax);
  w.sorted_j = a.take<int32_t>(n);
  w.tpc = a.take<int32_t>(4 * n);
  w.err = a.take<double>(kErrs * n);
  w.conf_q = a.take<double>(n);
  w.mconf = a.take<double>(n);
  w.mcm = a.take<double>(kErrs * n);
  w.mtot = a.take<int32_t>((size_t)C * kErrs);
  w.total_bytes = a.used;
  return w;
}

// score of each (sample, box) position, for the confidence curves
__global__ __launch_bounds__(256) void k_nus_conf(UdNusEvalIo io, int S, double* __restrict__ conf_q) {
  const int s = blockIdx.x;
  const int64_t p0 = io.pred_src[s], q0 = io.pred_off[s], np_ = io.pred_off[s + 1] - q0;
  for (int64_t i = threadIdx.x; i < np_; i += 256) conf_q[q0 + i] = io.pred_rec[(p0 + i) * kCols + 9];
}

constexpr int64_t kMaxRows = (int64_t)1 << 28;           // int32 positions with room for 5 errors per row

}  // namespace

extern "C" int ud_nus_pred_to_global(const float* boxes, int64_t n, int ncol, const float* scores, const int64_t* labels,
                                     const int32_t* batch_off, int B, const double* l2g, int num_classes,
                                     const int32_t* attr_moving_host, const int32_t* attr_still_host, double* rec,
                                     int32_t* cls, int32_t* attr, int32_t* status, ud_stream_t stream_) {
  if (n < 0 || n > kMaxRows || (ncol != 7 && ncol != 9) || B < 1 || num_classes < 1 ||
      num_classes > UD_NUS_MAX_CLASSES || !attr_moving_host || !attr_still_host || !status)
    return UD_ERR_INVALID_ARG;
  if (n == 0) return UD_OK;
  if (!boxes || !scores || !labels || !batch_off || !l2g || !rec || !cls || !attr) return UD_ERR_INVALID_ARG;
  AttrTab tab = {};
  for (int c = 0; c < num_classes; ++c) tab.moving[c] = attr_moving_host[c], tab.still[c] = attr_still_host[c];
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("nus_eval.k_nus_pred_prep", stream);
  k_nus_pred_prep<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(
      boxes, n, ncol, scores, labels, batch_off, B, l2g, num_classes, tab, rec, cls, attr, status);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

extern "C" size_t ud_nus_eval_workspace_bytes(int64_t P, int num_classes) {
  if (P < 0 || P > kMaxRows || num_classes < 1 || num_classes > UD_NUS_MAX_CLASSES) return 0;
  return carve_eval(nullptr, P, num_classes).total_bytes;
}

extern "C" int ud_nus_eval(const UdNusCfg* cfg_host, const UdNusEvalIo* io_host, int S, int64_t P, void* workspace,
                           size_t workspace_bytes, ud_stream_t stream_) {
  if (!cfg_host || !io_host || S < 1 || P < 0 || P > kMaxRows) return UD_ERR_INVALID_ARG;
  const UdNusCfg cfg = *cfg_host;
  const UdNusEvalIo io = *io_host;
  const int C = cfg.num_classes;
  if (C < 1 || C > UD_NUS_MAX_CLASSES || cfg.dist_th_tp_index < 0 || cfg.dist_th_tp_index > 3) return UD_ERR_INVALID_ARG;
  if (!io.pred_src || !io.pred_off || !io.gt_rec || !io.gt_cls || !io.gt_attr || !io.gt_num_pts || !io.gt_keep ||
      !io.gt_off || !io.ego || !io.prec || !io.conf || !io.tp_err || !io.counts || !io.status)
    return UD_ERR_INVALID_ARG;
  if (P > 0 && (!io.pred_rec || !io.pred_cls || !io.pred_attr || !io.tp || !io.match_gt || !io.order))
    return UD_ERR_INVALID_ARG;
  const size_t need = ud_nus_eval_workspace_bytes(P, C);
  if (!workspace || workspace_bytes < need) return UD_ERR_WORKSPACE;
  EvalWs w = carve_eval(workspace, P, C);
  hipStream_t stream = (hipStream_t)stream_;
  UD_HIP_TRY(hipMemsetAsync(io.counts, 0, 2 * C * sizeof(int32_t), stream));
  {
    UdProfScope prof("nus_eval.k_nus_match", stream);
    k_nus_match<<<S, 256, 0, stream>>>(cfg, io, P, w.skey, w.err);
    UD_LAUNCH_CHECK();
  }
  if (P > 0) {
    UdProfScope prof("nus_eval.sort", stream);
    k_nus_conf<<<S, 256, 0, stream>>>(io, S, w.conf_q);
    UD_LAUNCH_CHECK();
    const int rc = rs_sort_pairs<unsigned long long>(w.skey, (int)P, kSortBits, w.sorted_j, w.ktmp, w.vtmp, w.hist,
                                                     w.dtot, stream);
    if (rc != UD_OK) return rc;
  }
  {
    UdProfScope prof("nus_eval.scans", stream);
    if (P > 0) {
      k_nus_tp_scan<<<dim3(C, 4), 1024, 0, stream>>>(w.sorted_j, io.tp, io.counts, P, w.tpc, io.order);
      UD_LAUNCH_CHECK();
      k_nus_err_scan<<<dim3(C, kErrs), 1024, 0, stream>>>(w.sorted_j, io.tp, w.tpc, w.err, w.conf_q, io.counts, P,
                                                          cfg.dist_th_tp_index, w.mconf, w.mcm, w.mtot);
      UD_LAUNCH_CHECK();
    }
  }
  UdProfScope prof("nus_eval.k_nus_curves", stream);
  k_nus_curves<<<C, 128, 0, stream>>>(cfg, io.order, w.tpc, w.conf_q, w.mconf, w.mcm, w.mtot, io.counts, P, io.prec,
                                      io.conf, io.tp_err);
  UD_LAUNCH_CHECK();
  return UD_OK;
}
