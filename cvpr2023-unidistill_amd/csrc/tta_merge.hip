// Flip test-time augmentation: the head maps of V flipped views of a scene, un-flipped and averaged in the head's own
// parametrisation, every task and every head in ONE launch.
//
// Input and output tensors come as the proposal layer's descriptors (csrc/proposals.hip): a device pointer and
// (batch, channel, pixel) element strides of a logical fp32 [rows, c, H, W] tensor, so NCHW planes and channel slices of
// the packed channels-last head output are read where they lie.  View v of sample b is input row v * B + b.
//
// One thread per output element.  The channels of all present heads of all tasks form one list of J entries (task by
// task, hm reg height dim rot vel iou inside a task); an element index enumerates (sample, pixel, entry) with the entry
// fastest when the tensors are channels-last and (sample, entry, pixel) with the pixel fastest when they are planes, so
// the 64 lanes of a wave read -- per view -- and write consecutive addresses in either layout (an x flip only reverses
// the lanes inside a row).  Every input element is read once per view; the sum runs over the views in their given order
// and is scaled by 1 / V once: no atomics, nothing depends on the schedule, the result is bitwise reproducible.
#include "ud_common.h"
#include "ud_prof.h"

namespace {

constexpr int kMaxTasks = 8;
constexpr int kMaxViews = 4;
constexpr int kHeads = 7;            // hm, reg, height, dim, rot, vel, iou
constexpr int kMaxEntries = 256;     // channels of all heads of all tasks
constexpr int kThreads = 256;

enum Head { kHm = 0, kReg, kHeight, kDim, kRot, kVel, kIou };

struct Desc {                        // one head: source [V*B, c, H*W] and destination [B, c, H*W] through their strides
  const float* src;
  float* dst;
  long long sb, sc, sp;
  int db, dc, dp;
};
struct Params {
  Desc d[kMaxTasks * kHeads];
  unsigned char head_of[kMaxEntries];    // entry -> index into d
  unsigned char chan_of[kMaxEntries];    // entry -> channel inside that head
  int B, V, H, W, J, no_log, entry_fastest;
  unsigned total;
  int flip_dx[kMaxViews], flip_dy[kMaxViews];
};

__global__ __launch_bounds__(kThreads) void k_tta_merge(const Params P) {
  const unsigned idx = blockIdx.x * (unsigned)kThreads + threadIdx.x;
  if (idx >= P.total) return;
  const unsigned HW = (unsigned)(P.H * P.W), J = (unsigned)P.J;
  unsigned b, pix, e;
  if (P.entry_fastest) {
    e = idx % J;
    const unsigned r = idx / J;
    pix = r % HW;
    b = r / HW;
  } else {
    pix = idx % HW;
    const unsigned r = idx / HW;
    e = r % J;
    b = r / J;
  }
  const int k = P.head_of[e], c = P.chan_of[e], head = k % kHeads;
  const Desc& d = P.d[k];
  const int y = (int)(pix / (unsigned)P.W), x = (int)(pix - (unsigned)y * (unsigned)P.W);
  // what a flip does to this channel: r -> 1 - r, r -> -r, or nothing
  const bool one_minus_dx = head == kReg && c == 0, one_minus_dy = head == kReg && c == 1;
  const bool neg_dx = (head == kRot && c == 1) || (head == kVel && c == 0);
  const bool neg_dy = (head == kRot && c == 0) || (head == kVel && c == 1);
  const bool is_hm = head == kHm, is_log = head == kDim && !P.no_log;
  const float* src = d.src + (long long)c * d.sc;
  // hm and dim are averaged as probability / size: those sums, and the way back, are carried in double and rounded to float
  // once, so the device adds no error of its own to the float32 inputs; the linear heads stay in float, step by step
  const bool wide = is_hm || is_log;
  float acc = 0.f;
  double accw = 0.0;
  for (int v = 0; v < P.V; ++v) {
    const int fx = P.flip_dx[v], fy = P.flip_dy[v];
    const int ys = fy ? P.H - 1 - y : y, xs = fx ? P.W - 1 - x : x;
    float t = src[(long long)(v * P.B + (int)b) * d.sb + (long long)(ys * P.W + xs) * d.sp];
    if ((one_minus_dx && fx) || (one_minus_dy && fy)) t = 1.0f - t;
    if ((neg_dx && fx) || (neg_dy && fy)) t = -t;
    if (wide) {
      const double w = is_hm ? 1.0 / (1.0 + exp(-(double)t)) : exp((double)t);
      accw = v == 0 ? w : accw + w;
    } else {
      acc = v == 0 ? t : acc + t;
    }
  }
  if (wide) {
    // back into the head's parametrisation.  logit(m) = log m - log1p(-m): -inf at m == 0, +inf at m == 1, never NaN
    accw *= 1.0 / (double)P.V;
    acc = (float)(is_hm ? log(accw) - log1p(-accw) : log(accw));
  } else {
    acc *= 1.0f / (float)P.V;
  }
  d.dst[(long long)b * d.db + (long long)c * d.dc + (long long)pix * d.dp] = acc;
}

const int kChannels[kHeads] = {0, 2, 1, 3, 2, 2, 1};   // hm: the task's class count

}  // namespace

extern "C" int ud_tta_merge(const float* const* heads, const long long* strides, float* const* outs,
                            const long long* out_strides, const int* num_classes, const int* flips, int V, int B, int T,
                            int H, int W, int no_log, ud_stream_t stream_) {
  if (V < 1 || V > kMaxViews || B <= 0 || T <= 0 || T > kMaxTasks || H <= 0 || W <= 0) return UD_ERR_INVALID_ARG;
  if (!heads || !strides || !outs || !out_strides || !num_classes || !flips) return UD_ERR_INVALID_ARG;
  if ((long long)H * W > 0x7FFFFFFFll) return UD_ERR_INVALID_ARG;
  Params P;
  int J = 0;
  for (int t = 0; t < T; ++t) {
    if (num_classes[t] <= 0 || !heads[t * kHeads + kHm]) return UD_ERR_INVALID_ARG;
    for (int j = 0; j < kHeads; ++j) {
      const int k = t * kHeads + j;
      Desc& d = P.d[k];
      d.src = heads[k];
      d.dst = outs[k];
      d.sb = strides[k * 3]; d.sc = strides[k * 3 + 1]; d.sp = strides[k * 3 + 2];
      if (!d.src) { d.dst = nullptr; d.db = d.dc = d.dp = 0; continue; }      // an absent head
      if (!d.dst) return UD_ERR_INVALID_ARG;
      const int nc = j == kHm ? num_classes[t] : kChannels[j];
      // the largest output offset must fit the int strides and the int pixel index
      const long long db = out_strides[k * 3], dc = out_strides[k * 3 + 1], dp = out_strides[k * 3 + 2];
      if (db < 0 || dc < 0 || dp < 0 || d.sb < 0 || d.sc < 0 || d.sp < 0) return UD_ERR_INVALID_ARG;
      if (db > 0x7FFFFFFFll || dc > 0x7FFFFFFFll || dp > 0x7FFFFFFFll) return UD_ERR_UNSUPPORTED;
      d.db = (int)db; d.dc = (int)dc; d.dp = (int)dp;
      if (J + nc > kMaxEntries) return UD_ERR_UNSUPPORTED;
      for (int c = 0; c < nc; ++c, ++J) {
        P.head_of[J] = (unsigned char)k;
        P.chan_of[J] = (unsigned char)c;
      }
    }
  }
  for (int v = 0; v < V; ++v) {
    P.flip_dx[v] = flips[2 * v] != 0;
    P.flip_dy[v] = flips[2 * v + 1] != 0;
  }
  const long long total = (long long)B * H * W * J;
  if (total > 0x7FFFFFFFll || (long long)V * B > 0x7FFFFFFFll) return UD_ERR_UNSUPPORTED;
  // planes have a pixel stride of 1: the pixel runs fastest; anything else is taken as channels-last, the entry runs fastest
  P.entry_fastest = P.d[kHm].sp != 1;
  P.B = B; P.V = V; P.H = H; P.W = W; P.J = J; P.no_log = no_log != 0; P.total = (unsigned)total;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("tta.merge", stream);
  k_tta_merge<<<ud_div_up(total, kThreads), kThreads, 0, stream>>>(P);
  UD_LAUNCH_CHECK();
  return UD_OK;
}
