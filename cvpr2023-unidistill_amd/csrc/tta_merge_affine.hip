// Rotation / scale / flip test-time augmentation: the head maps of V views of a scene, each view the scene under the BEV
// transform A_v = F S R (no translation), resampled bilinearly onto the unrotated grid, their VALUES brought back into the
// original frame, and averaged over the views that cover a pixel -- every task and every head in ONE launch.
// The flip-only merge (tta_merge.hip) stays what it was; this kernel is the general case beside it.
//
// Descriptors, view-major rows and the index order are those of tta_merge.hip: one thread per output element, the entry
// fastest for channels-last tensors and the pixel fastest for planes, so writes (and channels-last reads) are coalesced;
// rotated reads of planes walk an oblique line through rows that neighbouring waves read too, and lean on the L2.
//
// Geometry in double.  Cell (x, y) covers [x, x+1) x [y, y+1) in cell units u.  T_v (2x3, from the host) takes
// original-frame u to view-frame u; output pixel p samples view v at q = T_v (p + 1/2): g = q - 1/2, i0 = floor(g),
// f = g - i0, neighbours i0, i0 + 1 per axis with weights 1 - f, f.  A flip or a multiple of 90 degrees on a square
// symmetric grid gives integer g: one neighbour, weight exactly 1.  A view contributes only where every neighbour of
// non-zero weight is inside the map; view 0 is a flip or the identity that maps the grid onto itself (checked on the
// host), so n(p) >= 1.
//
// Values.  Each neighbour's value is brought into the original frame, the (up to) four terms are blended, the views are
// added in their given order starting from the first that contributes, and the sum is divided by n(p).  No atomics:
// bitwise reproducible.  hm (as a probability) and a logarithmic dim (as a size) are carried in double, weights
// included, and rounded once; the other heads are fp32 one operation at a time (the build has -ffp-contract=off):
//   w_n = (float)(wy * wx);  term_n = m0 * a0 [+ m1 * a1] [cn +];  blend = w_00 t_00 + w_01 t_01 + w_10 t_10 + w_11 t_11
// (zero-weight neighbours skipped), with a0, a1 the head's channels 0 and 1 at the neighbour and, per view,
//   height, dim under no_log  m0 = (float)(1 / s)                                    iou  m0 = 1
//   reg[i]   m = row i of Ti (inverse of T's linear part), cn = (float)(Ti (n - T's offset) - p)_i   -- Ti (n + reg - t) - p
//   vel[i]   m = row i of Li = L^-1 in metres: Li_ij = Ti_ij cell_i / cell_j
//   rot      (cos, sin) <- s Li (cos, sin); channel 0 is sin, 1 is cos; not renormalised.
#include <cmath>

#include "ud_common.h"
#include "ud_prof.h"

namespace {

constexpr int kMaxTasks = 8;
constexpr int kMaxViews = 16;
constexpr int kHeads = 7;            // hm, reg, height, dim, rot, vel, iou
constexpr int kMaxEntries = 256;     // channels of all heads of all tasks
constexpr int kThreads = 256;
constexpr int kViewDoubles = 11;     // T (row-major 2x3), Ti (row-major 2x2), s

enum Head { kHm = 0, kReg, kHeight, kDim, kRot, kVel, kIou };

struct Desc {                        // one head: source [V*B, c, H*W] and destination [B, c, H*W] through their strides
  const float* src;
  float* dst;
  int sb, sc, sp;
  int db, dc, dp;
};
struct View {
  double t[6];                       // q = (t0 u + t1 v + t2, t3 u + t4 v + t5)
  double ti[4];                      // inverse of the linear part, cell units
};
struct Params {
  Desc d[kMaxTasks * kHeads];
  unsigned char head_of[kMaxEntries];           // entry -> index into d
  unsigned char entry0[kMaxTasks * kHeads];     // first entry of a head: channel = entry - entry0
  View view[kMaxViews];
  double s[kMaxViews];
  double cell_ratio;                            // cell_x / cell_y
  int B, V, H, W, J, no_log, entry_fastest;
  unsigned total;
};
static_assert(sizeof(Params) <= 4096, "kernel arguments are passed by value");

// one axis: the first neighbour, the fraction, and whether every neighbour of non-zero weight is inside [0, n)
__device__ __forceinline__ bool axis(double q, int n, int& i0, double& f) {
  const double g = q - 0.5, fl = floor(g);
  f = g - fl;
  if (!(fl >= 0.0 && fl + (f != 0.0 ? 1.0 : 0.0) <= (double)(n - 1))) return false;     // NaN and inf fail here
  i0 = (int)fl;
  return true;
}

__global__ __launch_bounds__(kThreads) void k_tta_merge_affine(const Params P) {
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
  const int k = P.head_of[e], c = (int)e - (int)P.entry0[k], head = k % kHeads;
  const Desc& d = P.d[k];
  const int y = (int)(pix / (unsigned)P.W), x = (int)(pix - (unsigned)y * (unsigned)P.W);
  const bool is_hm = head == kHm, is_log = head == kDim && !P.no_log, wide = is_hm || is_log;
  const bool vec2 = head == kReg || head == kRot || head == kVel, is_reg = head == kReg;
  // a scalar head reads its own channel; a two-vector head reads channels 0 and 1 for either output channel
  const float* src0 = d.src + (long long)(vec2 ? 0 : c) * d.sc;
  const float* src1 = d.src + (long long)d.sc;
  const double px = (double)x, py = (double)y;
  float acc = 0.f;
  double accw = 0.0;
  int n = 0;
  for (int v = 0; v < P.V; ++v) {
    const View& vw = P.view[v];
    const double qx = vw.t[0] * (px + 0.5) + vw.t[1] * (py + 0.5) + vw.t[2];
    const double qy = vw.t[3] * (px + 0.5) + vw.t[4] * (py + 0.5) + vw.t[5];
    int x0 = 0, y0 = 0;
    double fx, fy;
    if (!axis(qx, P.W, x0, fx) || !axis(qy, P.H, y0, fy)) continue;
    const double s = P.s[v], inv_s = 1.0 / s;
    // the view's coefficients on (a0, a1), and for reg the rows of Ti in double for the neighbour's constant
    float m0 = 1.0f, m1 = 0.0f;
    double r0 = 0.0, r1 = 0.0;
    if (head == kHeight || (head == kDim && P.no_log)) {
      m0 = (float)inv_s;
    } else if (vec2) {
      const double* ti = vw.ti;
      if (is_reg) {
        r0 = ti[2 * c];
        r1 = ti[2 * c + 1];
        m0 = (float)r0;
        m1 = (float)r1;
      } else {
        const double li[4] = {ti[0], ti[1] * P.cell_ratio, ti[2] / P.cell_ratio, ti[3]};
        if (head == kVel) {
          m0 = (float)li[2 * c];
          m1 = (float)li[2 * c + 1];
        } else if (c == 0) {        // sin' = Qi10 cos + Qi11 sin: a0 is sin, a1 is cos
          m0 = (float)(s * li[3]);
          m1 = (float)(s * li[2]);
        } else {                    // cos' = Qi00 cos + Qi01 sin
          m0 = (float)(s * li[1]);
          m1 = (float)(s * li[0]);
        }
      }
    }
    const long long row = (long long)(v * P.B + (int)b) * d.sb;
    float val = 0.f;
    double valw = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int jx = j & 1, jy = j >> 1;
      if ((jx && fx == 0.0) || (jy && fy == 0.0)) continue;            // weight 0: not read, may lie outside
      const double w = (jy ? fy : 1.0 - fy) * (jx ? fx : 1.0 - fx);
      const int xs = x0 + jx, ys = y0 + jy;
      const long long off = row + (long long)(ys * P.W + xs) * d.sp;
      const float a0 = src0[off];
      if (wide) {
        const double t = is_hm ? 1.0 / (1.0 + exp(-(double)a0)) : exp((double)a0) * inv_s;
        valw = j == 0 ? w * t : valw + w * t;
      } else {
        float t = m0 * a0;
        if (vec2) {
          t = t + m1 * src1[off];
          if (is_reg)
            t = (float)(r0 * ((double)xs - vw.t[2]) + r1 * ((double)ys - vw.t[5]) - (c == 0 ? px : py)) + t;
        }
        const float wf = (float)w;
        val = j == 0 ? wf * t : val + wf * t;
      }
    }
    if (wide) accw = n == 0 ? valw : accw + valw;
    else acc = n == 0 ? val : acc + val;
    ++n;
  }
  if (wide) {
    // back into the head's parametrisation.  logit(m) = log m - log1p(-m): -inf at m == 0, +inf at m == 1, never NaN (the
    // weights of a view add up to 1 only within rounding: the mean probability is clamped to 1)
    accw = accw / (double)n;
    acc = (float)(is_hm ? log(fmin(accw, 1.0)) - log1p(-fmin(accw, 1.0)) : log(accw));
  } else {
    acc *= 1.0f / (float)n;
  }
  d.dst[(long long)b * d.db + (long long)c * d.dc + (long long)pix * d.dp] = acc;
}

const int kChannels[kHeads] = {0, 2, 1, 3, 2, 2, 1};   // hm: the task's class count

// view 0 must map the grid onto itself: a flip or the identity with the offset that goes with it
bool covers_grid(const double* p, int H, int W) {
  const double n[2] = {(double)W, (double)H};
  if (p[1] != 0.0 || p[3] != 0.0 || p[10] != 1.0) return false;
  for (int a = 0; a < 2; ++a) {
    const double lin = p[a * 4], off = p[a * 3 + 2];
    if (!((lin == 1.0 && off == 0.0) || (lin == -1.0 && off == n[a]))) return false;
  }
  return true;
}

}  // namespace

extern "C" int ud_tta_merge_affine(const float* const* heads, const long long* strides, float* const* outs,
                                   const long long* out_strides, const int* num_classes, const double* view_params,
                                   double cell_ratio, int V, int B, int T, int H, int W, int no_log, ud_stream_t stream_) {
  if (V < 1 || V > kMaxViews || B <= 0 || T <= 0 || T > kMaxTasks || H <= 0 || W <= 0) return UD_ERR_INVALID_ARG;
  if (!heads || !strides || !outs || !out_strides || !num_classes || !view_params) return UD_ERR_INVALID_ARG;
  if ((long long)H * W > 0x7FFFFFFFll) return UD_ERR_INVALID_ARG;
  if (!std::isfinite(cell_ratio) || cell_ratio <= 0.0) return UD_ERR_INVALID_ARG;
  Params P;
  for (int v = 0; v < V; ++v) {
    const double* p = view_params + v * kViewDoubles;
    for (int i = 0; i < kViewDoubles; ++i)
      if (!std::isfinite(p[i])) return UD_ERR_INVALID_ARG;
    if (p[10] <= 0.0) return UD_ERR_INVALID_ARG;
    for (int i = 0; i < 6; ++i) P.view[v].t[i] = p[i];
    for (int i = 0; i < 4; ++i) P.view[v].ti[i] = p[6 + i];
    P.s[v] = p[10];
  }
  if (!covers_grid(view_params, H, W)) return UD_ERR_INVALID_ARG;
  int J = 0;
  for (int t = 0; t < T; ++t) {
    if (num_classes[t] <= 0 || !heads[t * kHeads + kHm]) return UD_ERR_INVALID_ARG;
    for (int j = 0; j < kHeads; ++j) {
      const int k = t * kHeads + j;
      Desc& d = P.d[k];
      d.src = heads[k];
      d.dst = outs[k];
      P.entry0[k] = 0;
      if (!d.src) { d.dst = nullptr; d.sb = d.sc = d.sp = d.db = d.dc = d.dp = 0; continue; }      // an absent head
      if (!d.dst) return UD_ERR_INVALID_ARG;
      const int nc = j == kHm ? num_classes[t] : kChannels[j];
      // every stride fits an int; offsets are formed in 64 bits from them
      long long st[6];
      for (int i = 0; i < 3; ++i) {
        st[i] = strides[k * 3 + i];
        st[3 + i] = out_strides[k * 3 + i];
      }
      for (int i = 0; i < 6; ++i) {
        if (st[i] < 0) return UD_ERR_INVALID_ARG;
        if (st[i] > 0x7FFFFFFFll) return UD_ERR_UNSUPPORTED;
      }
      d.sb = (int)st[0]; d.sc = (int)st[1]; d.sp = (int)st[2];
      d.db = (int)st[3]; d.dc = (int)st[4]; d.dp = (int)st[5];
      if (J + nc > kMaxEntries) return UD_ERR_UNSUPPORTED;
      P.entry0[k] = (unsigned char)J;
      for (int c = 0; c < nc; ++c, ++J) P.head_of[J] = (unsigned char)k;
    }
  }
  const long long total = (long long)B * H * W * J;
  if (total > 0x7FFFFFFFll || (long long)V * B > 0x7FFFFFFFll) return UD_ERR_UNSUPPORTED;
  // planes have a pixel stride of 1: the pixel runs fastest; anything else is taken as channels-last, the entry runs fastest
  P.entry_fastest = P.d[kHm].sp != 1;
  P.cell_ratio = cell_ratio;
  P.B = B; P.V = V; P.H = H; P.W = W; P.J = J; P.no_log = no_log != 0; P.total = (unsigned)total;
  hipStream_t stream = (hipStream_t)stream_;
  UdProfScope prof("tta.merge_affine", stream);
  k_tta_merge_affine<<<ud_div_up(total, kThreads), kThreads, 0, stream>>>(P);
  UD_LAUNCH_CHECK();
  return UD_OK;
}
