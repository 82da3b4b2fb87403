// JPEG decode after collate: the reference's skimage_io.imread of every camera frame
// (nuscenes_multimodal.py:171-177, :197 -> Pillow -> libjpeg-turbo), rebuilt on the device and bit-exact to Pillow.
//
//   ud_jpeg_parse    host: markers -> one UdJpegFrame record (tables, geometry, entropy-coded byte range)
//   k_jd_destuff     one workgroup per frame: FF 00 -> FF, split at RSTn, end at the first other marker; a compaction
//                    (wave scans, no global atomics)
//   k_jd_huffman     one workgroup per frame: every restart segment is cut into UD_JPEG_SUB_BITS-bit subsequences,
//                    one thread each.  The decoder state (bit position, zig-zag index, block in the MCU) fully
//                    determines what follows, so each subsequence decodes from a guessed entry state until it crosses
//                    its end, its exit becomes the next one's entry, and the subsequences whose entry changed decode
//                    again until every boundary agrees (Huffman codes self-synchronise within a few symbols; the
//                    first subsequence of a segment starts from the known state, so round r fixes at least the first
//                    r and the loop is bounded).  A scan of the block counts and DC sums, then the final pass writes
//                    the coefficients in natural order with the DC prediction resolved.
//   k_jd_idct        one thread per block: dequantise + jidctint.c's ISLOW IDCT -> uint8 component planes
//   k_jd_color       per pixel: libjpeg's fancy upsampling (h2v1 / h2v2 triangle filter, box when the downsampled
//                    width is <= 2), jdcolor.c's YCbCr -> RGB, cropped to W x H; zeros for a failed frame.
// The exactness notes (the SIMD clamp after the IDCT, the fancy-upsampling edges) are in DESIGN §2.11.
#include <string.h>

#include "ud_common.h"
#include "ud_prof.h"

namespace {

constexpr int kSub = UD_JPEG_SUB_BITS;
constexpr int kLook = UD_JPEG_LOOKAHEAD;
constexpr int kWg = 1024;                  // threads of the per-frame workgroups (destuff, Huffman)
constexpr int kDestuffBytes = 16;          // bytes per thread per destuff chunk

__constant__ unsigned char c_natural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const unsigned char h_natural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- host: markers -> record ---------------------------------------------------------------------------------
int jd_huff_table(const unsigned char* counts, const unsigned char* vals, UdJpegHuff* t) {
  memset(t, 0, sizeof(*t));
  int total = 0;
  for (int l = 0; l < 16; ++l) total += counts[l];
  memcpy(t->vals, vals, (size_t)total);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    t->maxcode[l] = -1;
    const int n = counts[l - 1];
    // libjpeg's rule (jdhuff.c jpeg_make_d_derived_tbl): the codes of a length must stay below the all-ones code.
    // Checked before any entry is written, so an oversubscribed table never indexes past look[].
    if (code + n >= (1 << l)) return UD_JPEG_CORRUPT;
    if (n) {
      t->valoff[l] = k - code;
      for (int i = 0; i < n; ++i, ++code, ++k)
        if (l <= kLook) {
          const int sh = kLook - l;
          for (int e = code << sh; e < (code + 1) << sh; ++e) t->look[e] = (uint16_t)(l << 8 | vals[k]);
        }
      t->maxcode[l] = code - 1;
    }
    code <<= 1;
  }
  t->maxcode[0] = t->maxcode[17] = -1;
  return UD_JPEG_OK;
}

inline int64_t jd_div_up(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Geometry every kernel relies on, derived from the sizes and sampling factors alone.
void jd_geometry(UdJpegFrame* f) {
  f->mcus_x = (int)jd_div_up(f->width, 8 * f->hmax);
  f->mcus_y = (int)jd_div_up(f->height, 8 * f->vmax);
  f->bpm = f->hmax * f->vmax + 2;
  const int64_t nmcu = (int64_t)f->mcus_x * f->mcus_y;
  f->nseg = f->restart ? (int)jd_div_up(nmcu, f->restart) : 1;
  for (int c = 0; c < 3; ++c) {
    f->cw[c] = (int)jd_div_up((int64_t)f->width * f->h[c], f->hmax);
    f->ch[c] = (int)jd_div_up((int64_t)f->height * f->v[c], f->vmax);
  }
}

size_t jd_plane_bytes(const UdJpegFrame& f, int c) {
  return (size_t)f.mcus_x * f.h[c] * 8 * (size_t)f.mcus_y * f.v[c] * 8;
}

struct JdSubRes {              // exit state of one subsequence + what it decoded (two int4)
  int pos, zzblk, n, ch;       // zzblk = zz | blk << 8; ch: changed in this round
  int dc0, dc1, dc2, pad;
};

// Workspace of one frame, in the order ud_jpeg_plan lays it out (coefficients of all frames first: one zero pass).
struct JdSizes {
  size_t ecs, seg, sub, state, scan, coef, plane[3];
};
JdSizes jd_sizes(const UdJpegFrame& f) {
  JdSizes s;
  const int64_t nsub = jd_div_up(f.ecs_bytes * 8, kSub) + f.nseg;
  s.ecs = ud_align_up((size_t)f.ecs_bytes + 16, 16);
  s.seg = ud_align_up(2 * ((size_t)f.nseg + 1) * sizeof(int), 16);
  s.sub = ud_align_up((size_t)nsub * sizeof(int4), 16);
  s.state = ud_align_up(2 * (size_t)nsub * sizeof(JdSubRes), 16);
  s.scan = ud_align_up(((size_t)nsub + 1) * sizeof(int4), 16);
  s.coef = (size_t)f.mcus_x * f.mcus_y * f.bpm * 64 * sizeof(int16_t);
  for (int c = 0; c < 3; ++c) s.plane[c] = ud_align_up(jd_plane_bytes(f, c), 16);
  return s;
}

bool jd_record_ok(const UdJpegFrame& f) {
  if (f.width <= 0 || f.height <= 0 || f.width > 65535 || f.height > 65535 || f.restart < 0 || f.restart > 65535 ||
      f.ecs_off < 0 || f.ecs_bytes < 0 || f.ecs_bytes > (1LL << 28) || f.src_off < 0 || f.out_off < 0)
    return false;
  const bool s444 = f.hmax == 1 && f.vmax == 1, s422 = f.hmax == 2 && f.vmax == 1, s420 = f.hmax == 2 && f.vmax == 2;
  if (!(s444 || s422 || s420) || f.h[0] != f.hmax || f.v[0] != f.vmax) return false;
  for (int c = 1; c < 3; ++c)
    if (f.h[c] != 1 || f.v[c] != 1) return false;
  UdJpegFrame g = f;
  jd_geometry(&g);
  if (g.mcus_x != f.mcus_x || g.mcus_y != f.mcus_y || g.bpm != f.bpm || g.nseg != f.nseg) return false;
  for (int c = 0; c < 3; ++c)
    if (g.cw[c] != f.cw[c] || g.ch[c] != f.ch[c]) return false;
  return f.total_blocks == (int64_t)f.mcus_x * f.mcus_y * f.bpm &&
         f.nsub_max == jd_div_up(f.ecs_bytes * 8, kSub) + f.nseg;
}

// ---- device: bit reader over one destuffed segment ------------------------------------------------------------
// 64-bit window; bytes past the segment read as zero (libjpeg fills zeros after a marker), so no read leaves it.
struct JdBits {
  const unsigned char* p;
  int nbytes;
  int base;                    // bit position of the window's most significant bit
  unsigned long long w;
  __device__ void fill(int pos) {
    base = pos & ~7;
    const int b0 = base >> 3;
    unsigned long long v = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) v = v << 8 | (b0 + i < nbytes ? p[b0 + i] : 0u);
    w = v;
  }
  __device__ unsigned peek32(int pos) {      // the 32 bits from pos
    if (pos - base > 32 || pos < base) fill(pos);
    return (unsigned)((w << (pos - base)) >> 32);
  }
};

struct JdTables {                            // the frame's six Huffman tables, in LDS
  uint16_t look[6][1 << kLook];
  int maxcode[6][18];
  int valoff[6][18];
  unsigned char vals[6][256];
};

struct JdSt {
  int pos, zz, blk;
};

__device__ __forceinline__ int jd_extend(int v, int s) { return s && v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// Huffman symbol at pos in table t -> symbol, *len (0: invalid code).
__device__ __forceinline__ int jd_huff(const JdTables& T, int t, unsigned w, int* len) {
  const int e = T.look[t][w >> (32 - kLook)];
  if (e) {
    *len = e >> 8;
    return e & 255;
  }
  for (int l = kLook + 1; l <= 16; ++l) {
    const int code = (int)(w >> (32 - l));
    if (code <= T.maxcode[t][l]) {
      *len = l;
      return T.vals[t][(T.valoff[t][l] + code) & 255];
    }
  }
  *len = 0;
  return 0;
}

enum { kEvNone = 0, kEvBlock = 1, kEvInvalid = 2 };

// One symbol (code + extra bits) from state s, as tests/jpeg_reference.py step().  *zpos / *val: the coefficient's
// zig-zag index (-1: none) and value (the DC difference at 0).  Returns kEv*.
__device__ __forceinline__ int jd_step(const JdTables& T, const int* blk_comp, int bpm, JdBits& br, JdSt& s, int* zpos,
                                       int* val) {
  *zpos = -1;
  const int c = blk_comp[s.blk];
  const unsigned w = br.peek32(s.pos);
  int len;
  bool block_end = false, invalid = false;
  if (s.zz == 0) {
    const int sym = jd_huff(T, 2 * c, w, &len);
    if (!len || sym > 15) {
      invalid = true;
    } else {
      *zpos = 0;
      *val = sym ? jd_extend((int)((w << len) >> (32 - sym)), sym) : 0;
      s.pos += len + sym;
      s.zz = 1;
    }
  } else {
    const int rs = jd_huff(T, 2 * c + 1, w, &len);
    if (!len) {
      invalid = true;
    } else {
      const int r = rs >> 4, sz = rs & 15;
      s.pos += len;
      if (sz) {
        s.zz += r;
        if (s.zz > 63) {
          invalid = true;
          len = 0;
          s.pos += sz - 16;                  // matches the reference: the block is abandoned after the extra bits
        } else {
          *zpos = s.zz;
          *val = jd_extend((int)((w << len) >> (32 - sz)), sz);
          s.zz += 1;
          s.pos += sz;
        }
      } else if (r == 15) {
        s.zz += 16;
      } else {
        s.zz = 64;
      }
      block_end = s.zz >= 64;
    }
  }
  if (invalid) s.pos += 16;
  if (invalid || block_end) {
    s.zz = 0;
    s.blk = s.blk + 1 < bpm ? s.blk + 1 : 0;
  }
  return invalid ? kEvInvalid : (block_end ? kEvBlock : kEvNone);
}

// ---- device: workgroup scans (kWg threads, 16 waves) -----------------------------------------------------------
__device__ __forceinline__ unsigned jd_wave_incl(unsigned v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// Exclusive scan of v over the workgroup; *total <- the sum.  lds: 16 words.  Contains barriers.
__device__ unsigned jd_wg_excl(unsigned v, unsigned* lds, unsigned* total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned inc = jd_wave_incl(v);
  __syncthreads();
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  unsigned before = 0, all = 0;
  for (int i = 0; i < kWg / 64; ++i) {
    const unsigned x = lds[i];
    before += i < wave ? x : 0u;
    all += x;
  }
  *total = all;
  return before + inc - v;
}

// ---- K1: destuff + split at RSTn ------------------------------------------------------------------------------
__global__ __launch_bounds__(kWg) void k_jd_destuff(const unsigned char* __restrict__ src,
                                                    const UdJpegFrame* __restrict__ frames,
                                                    unsigned char* __restrict__ ws, int* __restrict__ status,
                                                    int* __restrict__ iters) {
  constexpr int kChunk = kWg * kDestuffBytes;
  __shared__ unsigned s_scan[16];
  __shared__ int s_err, s_term;
  const UdJpegFrame& f = frames[blockIdx.x];
  const unsigned char* e = src + f.src_off + f.ecs_off;
  const long long L = f.ecs_bytes;
  unsigned char* out = ws + f.ws_ecs;
  int* seg_start = (int*)(ws + f.ws_seg);
  const int nseg = f.nseg;
  if (threadIdx.x == 0) s_err = 0, seg_start[0] = 0;
  int err = 0;
  unsigned kept_base = 0, rst_base = 0;
  bool ended = false;                         // uniform: the scan's end marker was found
  for (long long c0 = 0; c0 < L && !ended; c0 += kChunk) {
    const long long i0 = c0 + (long long)threadIdx.x * kDestuffBytes;
    // The scan ends at the first FF not followed by 00 or RSTn (EOI, any other marker, or FF as the last byte), as
    // libjpeg stops reading entropy-coded data at a marker; whatever follows it (e.g. bytes after EOI) is ignored.
    // Before that position every FF starts a stuffed pair or an RSTn, so the classification below is unambiguous.
    if (threadIdx.x == 0) s_term = kChunk;
    __syncthreads();
    for (int j = 0; j < kDestuffBytes; ++j) {
      const long long i = i0 + j;
      if (i >= L) break;
      if (e[i] != 0xFF) continue;
      const int nxt = i + 1 < L ? (int)e[i + 1] : -1;
      if (nxt != 0 && (nxt < 0xD0 || nxt > 0xD7)) {
        atomicMin(&s_term, (int)(i - c0));    // LDS
        break;
      }
    }
    __syncthreads();
    const long long lim = c0 + s_term < L ? c0 + s_term : L;
    unsigned keep = 0, rst = 0;
    // classify: 1 keep, 2 restart marker byte, 0 drop (stuffed 00, the FF of an RSTn)
    unsigned char cls[kDestuffBytes];
#pragma unroll
    for (int j = 0; j < kDestuffBytes; ++j) {
      const long long i = i0 + j;
      cls[j] = 0;
      if (i >= lim) continue;
      const unsigned b = e[i];
      if (i > 0 && e[i - 1] == 0xFF) cls[j] = b == 0 ? 0 : 2;
      else cls[j] = b == 0xFF ? (e[i + 1] == 0 ? 1 : 0) : 1;   // i + 1 < L: an FF at L - 1 is the scan's end
      keep += cls[j] == 1;
      rst += cls[j] == 2;
    }
    unsigned tk, tr;
    unsigned pk = jd_wg_excl(keep, s_scan, &tk) + kept_base;
    __syncthreads();
    unsigned pr = jd_wg_excl(rst, s_scan, &tr) + rst_base;
#pragma unroll
    for (int j = 0; j < kDestuffBytes; ++j) {
      const long long i = i0 + j;
      if (cls[j] == 1) {
        out[pk++] = e[i];
      } else if (cls[j] == 2) {
        if ((e[i] & 7u) != (pr & 7u) || (long long)pr + 1 >= nseg) err = 1;
        else seg_start[pr + 1] = (int)pk;
        ++pr;
      }
    }
    kept_base += tk;
    rst_base += tr;
    ended = s_term < kChunk;
    __syncthreads();
  }
  if (err) atomicOr(&s_err, 1);               // LDS flag of the workgroup
  __syncthreads();
  if (threadIdx.x == 0) {
    if ((long long)rst_base + 1 != nseg) s_err = 1;
    seg_start[nseg] = (int)kept_base;
    status[blockIdx.x] = s_err ? UD_JPEG_ST_MARKER : 0;
    if (iters) iters[blockIdx.x] = 0;
  }
}

// ---- K2: self-synchronising Huffman decode -----------------------------------------------------------------------
struct JdDesc {
  int seg, start, end, first;      // bits relative to the segment's first destuffed byte
};

__device__ __forceinline__ JdBits jd_bits(const unsigned char* ecs, const int* seg_start, int s) {
  JdBits b;
  b.p = ecs + seg_start[s];
  b.nbytes = seg_start[s + 1] - seg_start[s];
  b.base = 0;
  b.fill(0);
  return b;
}

// Decode from st until the position reaches end: -> exit state, blocks ended, DC difference sums per component.
__device__ JdSubRes jd_run(const JdTables& T, const int* blk_comp, int bpm, JdBits& br, JdSt st, int end) {
  JdSubRes r = {};
  unsigned dc[3] = {0, 0, 0};
  while (st.pos < end) {
    const int c = blk_comp[st.blk];
    int zpos, val;
    const int ev = jd_step(T, blk_comp, bpm, br, st, &zpos, &val);
    if (zpos == 0) dc[c] += (unsigned)val;
    r.n += ev != kEvNone;
  }
  r.pos = st.pos;
  r.zzblk = st.zz | st.blk << 8;
  r.dc0 = (int)dc[0], r.dc1 = (int)dc[1], r.dc2 = (int)dc[2];
  return r;
}

__device__ __forceinline__ JdSt jd_state(const JdSubRes& r) { return {r.pos, r.zzblk & 255, r.zzblk >> 8}; }

__global__ __launch_bounds__(kWg) void k_jd_huffman(const UdJpegFrame* __restrict__ frames,
                                                    unsigned char* __restrict__ ws, int* __restrict__ status,
                                                    int* __restrict__ iters) {
  __shared__ JdTables T;
  __shared__ unsigned s_scan[16];
  __shared__ int s_err, s_blk_comp[8];
  const UdJpegFrame& f = frames[blockIdx.x];
  if (status[blockIdx.x] != 0) return;        // uniform over the workgroup
  for (int i = threadIdx.x; i < 6 * (1 << kLook); i += kWg) T.look[i >> kLook][i & ((1 << kLook) - 1)] =
      f.huff[i >> kLook].look[i & ((1 << kLook) - 1)];
  for (int i = threadIdx.x; i < 6 * 18; i += kWg) {
    T.maxcode[i / 18][i % 18] = f.huff[i / 18].maxcode[i % 18];
    T.valoff[i / 18][i % 18] = f.huff[i / 18].valoff[i % 18];
  }
  for (int i = threadIdx.x; i < 6 * 256; i += kWg) T.vals[i >> 8][i & 255] = f.huff[i >> 8].vals[i & 255];
  const int ny = f.hmax * f.vmax, bpm = f.bpm;
  if (threadIdx.x < 8) s_blk_comp[threadIdx.x] = threadIdx.x < ny ? 0 : (threadIdx.x == ny ? 1 : 2);
  if (threadIdx.x == 0) s_err = 0;
  const unsigned char* ecs = ws + f.ws_ecs;
  const int* seg_start = (const int*)(ws + f.ws_seg);
  int* sub_off = (int*)(ws + f.ws_seg) + f.nseg + 1;
  JdDesc* desc = (JdDesc*)(ws + f.ws_sub);
  JdSubRes* X = (JdSubRes*)(ws + f.ws_state);
  const long long nsub_max = f.nsub_max;
  JdSubRes* Xb[2] = {X, X + nsub_max};
  int4* P = (int4*)(ws + f.ws_scan);
  const int nseg = f.nseg;
  __syncthreads();

  // subsequences per segment -> sub_off (exclusive scan over the segments)
  unsigned carry = 0;
  for (int s0 = 0; s0 < nseg; s0 += kWg) {
    const int s = s0 + threadIdx.x;
    unsigned n = 0;
    if (s < nseg) {
      const long long bits = 8LL * (seg_start[s + 1] - seg_start[s]);
      n = bits > kSub ? (unsigned)((bits + kSub - 1) / kSub) : 1u;
    }
    unsigned tot;
    const unsigned ex = jd_wg_excl(n, s_scan, &tot);
    if (s < nseg) sub_off[s] = (int)(carry + ex);
    carry += tot;
    __syncthreads();
  }
  const int nsub = (int)carry;
  if (threadIdx.x == 0) sub_off[nseg] = nsub;
  if ((long long)nsub > nsub_max) {           // cannot happen for a destuffed stream of ecs_bytes; checked anyway
    if (threadIdx.x == 0) status[blockIdx.x] = UD_JPEG_ST_LENGTH;
    return;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nsub; k += kWg) {
    int lo = 0, hi = nseg - 1;                // largest s with sub_off[s] <= k
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (sub_off[mid] <= k) lo = mid;
      else hi = mid - 1;
    }
    const int j = k - sub_off[lo];
    const int bits = 8 * (seg_start[lo + 1] - seg_start[lo]);
    const int start = j * kSub;
    desc[k] = {lo, start, start + kSub < bits ? start + kSub : bits, j == 0};
  }
  __syncthreads();

  // round 0 from the guessed entries, then re-decode the subsequences whose entry changed until none does
  for (int k = threadIdx.x; k < nsub; k += kWg) {
    const JdDesc d = desc[k];
    JdBits br = jd_bits(ecs, seg_start, d.seg);
    JdSubRes r = jd_run(T, s_blk_comp, bpm, br, {d.first ? 0 : d.start, 0, 0}, d.end);
    r.ch = 1;
    Xb[0][k] = r;
  }
  int cur = 0, rounds = 1;
  for (int it = 1; it <= nsub; ++it) {
    __syncthreads();
    const JdSubRes* Xp = Xb[cur];
    JdSubRes* Xq = Xb[cur ^ 1];
    int any = 0;
    for (int k = threadIdx.x; k < nsub; k += kWg) {
      const JdDesc d = desc[k];
      JdSubRes old = Xp[k];
      if (!d.first && Xp[k - 1].ch) {
        JdBits br = jd_bits(ecs, seg_start, d.seg);
        JdSubRes r = jd_run(T, s_blk_comp, bpm, br, jd_state(Xp[k - 1]), d.end);
        r.ch = r.pos != old.pos || r.zzblk != old.zzblk;
        any |= r.ch;
        Xq[k] = r;
      } else {
        old.ch = 0;
        Xq[k] = old;
      }
    }
    cur ^= 1;
    if (!__syncthreads_or(any)) break;
    ++rounds;
  }
  const JdSubRes* Xf = Xb[cur];

  // exclusive scan of (blocks, DC sums) over the subsequences
  carry = 0;
  unsigned cdc[3] = {0, 0, 0};
  for (int k0 = 0; k0 <= nsub; k0 += kWg) {
    const int k = k0 + threadIdx.x;
    JdSubRes r = {};
    if (k < nsub) r = Xf[k];
    unsigned t0, t1, t2, t3;
    const unsigned e0 = jd_wg_excl((unsigned)r.n, s_scan, &t0);
    __syncthreads();
    const unsigned e1 = jd_wg_excl((unsigned)r.dc0, s_scan, &t1);
    __syncthreads();
    const unsigned e2 = jd_wg_excl((unsigned)r.dc1, s_scan, &t2);
    __syncthreads();
    const unsigned e3 = jd_wg_excl((unsigned)r.dc2, s_scan, &t3);
    if (k <= nsub) P[k] = make_int4((int)(carry + e0), (int)(cdc[0] + e1), (int)(cdc[1] + e2), (int)(cdc[2] + e3));
    carry += t0, cdc[0] += t1, cdc[1] += t2, cdc[2] += t3;
    __syncthreads();
  }
  __syncthreads();

  const long long nmcu = (long long)f.mcus_x * f.mcus_y;
  const long long R = f.restart ? f.restart : nmcu;
  int err = 0;
  for (int s = threadIdx.x; s < nseg; s += kWg) {          // every segment holds at least its blocks
    const long long b0 = s * R * bpm, b1 = ((s + 1) * R < nmcu ? (s + 1) * R : nmcu) * bpm;
    if ((long long)(P[sub_off[s + 1]].x - P[sub_off[s]].x) < b1 - b0) err |= UD_JPEG_ST_LENGTH;
  }
  // final pass: coefficients in natural order, DC prediction resolved, stop at the segment's last block
  int16_t* coef = (int16_t*)(ws + f.ws_coef);
  for (int k = threadIdx.x; k < nsub; k += kWg) {
    const JdDesc d = desc[k];
    const int4 p0 = P[sub_off[d.seg]], pk = P[k];
    const long long b0 = d.seg * R * bpm;
    const long long b1 = ((d.seg + 1) * R < nmcu ? (d.seg + 1) * R : nmcu) * bpm;
    long long b = b0 + (unsigned)(pk.x - p0.x);
    int pred[3] = {pk.y - p0.y, pk.z - p0.z, pk.w - p0.w};
    JdSt st = d.first ? JdSt{0, 0, 0} : jd_state(Xf[k - 1]);
    JdBits br = jd_bits(ecs, seg_start, d.seg);
    while (st.pos < d.end && b < b1) {
      const int c = s_blk_comp[st.blk];
      int zpos, val;
      const int ev = jd_step(T, s_blk_comp, bpm, br, st, &zpos, &val);
      if (zpos >= 0) {
        if (zpos == 0) val = pred[c] = (int)((unsigned)pred[c] + (unsigned)val);
        coef[b * 64 + c_natural[zpos]] = (int16_t)val;
      }
      if (ev == kEvInvalid) {
        err |= UD_JPEG_ST_CODE;
        break;
      }
      if (ev == kEvBlock && ++b == b1 && (st.pos + 7) / 8 != br.nbytes) err |= UD_JPEG_ST_LENGTH;
    }
  }
  if (err) atomicOr(&s_err, err);            // LDS flag of the workgroup
  __syncthreads();
  if (threadIdx.x == 0) {
    status[blockIdx.x] = s_err;
    if (iters) iters[blockIdx.x] = rounds;
  }
}

// ---- K3: dequantise + ISLOW IDCT (jidctint.c: CONST_BITS 13, PASS1_BITS 2) -> component planes ------------------
__device__ __forceinline__ void jd_idct_1d(const int* in, int stride_in, int* out, int stride_out, int shift) {
  const int s0 = in[0], s1 = in[stride_in], s2 = in[2 * stride_in], s3 = in[3 * stride_in];
  const int s4 = in[4 * stride_in], s5 = in[5 * stride_in], s6 = in[6 * stride_in], s7 = in[7 * stride_in];
  int z1 = (s2 + s6) * 4433;
  const int tmp2 = z1 + s6 * -15137, tmp3 = z1 + s2 * 6270;
  const int tmp0 = (s0 + s4) * 8192, tmp1 = (s0 - s4) * 8192;
  const int t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
  int t0 = s7, t1 = s5, t2 = s3, t3 = s1;
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * 9633;
  t0 *= 2446, t1 *= 16819, t2 *= 25172, t3 *= 12299;
  z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
  t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
  const int half = 1 << (shift - 1);
  out[0] = (t10 + t3 + half) >> shift;
  out[7 * stride_out] = (t10 - t3 + half) >> shift;
  out[1 * stride_out] = (t11 + t2 + half) >> shift;
  out[6 * stride_out] = (t11 - t2 + half) >> shift;
  out[2 * stride_out] = (t12 + t1 + half) >> shift;
  out[5 * stride_out] = (t12 - t1 + half) >> shift;
  out[3 * stride_out] = (t13 + t0 + half) >> shift;
  out[4 * stride_out] = (t13 - t0 + half) >> shift;
}

__global__ __launch_bounds__(128) void k_jd_idct(const UdJpegFrame* __restrict__ frames,
                                                 unsigned char* __restrict__ ws, const int* __restrict__ status) {
  const UdJpegFrame& f = frames[blockIdx.y];
  const long long b = (long long)blockIdx.x * 128 + threadIdx.x;
  if (b >= f.total_blocks || status[blockIdx.y] != 0) return;
  const int bpm = f.bpm, ny = f.hmax * f.vmax;
  const long long mcu = b / bpm;
  const int j = (int)(b - mcu * bpm);
  const int my = (int)(mcu / f.mcus_x), mx = (int)(mcu - (long long)my * f.mcus_x);
  int c = 0, jx = 0, jy = 0;
  if (j < ny) jy = j / f.hmax, jx = j - jy * f.hmax;
  else c = j - ny + 1;
  const int hc = c ? 1 : f.hmax, vc = c ? 1 : f.vmax;
  const long long pw = (long long)f.mcus_x * hc * 8;
  unsigned char* plane = ws + f.ws_plane[c] + ((long long)(my * vc + jy) * 8) * pw + (long long)(mx * hc + jx) * 8;
  const int4* cp = (const int4*)(ws + f.ws_coef + b * 128);
  int blk[64], tmp[64];
  const uint16_t* q = f.qt[c];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int4 v = cp[i];
    const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      blk[8 * i + 2 * h] = (int)(int16_t)(w[h] & 0xFFFF) * (int)q[8 * i + 2 * h];
      blk[8 * i + 2 * h + 1] = (int)(int16_t)((unsigned)w[h] >> 16) * (int)q[8 * i + 2 * h + 1];
    }
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) jd_idct_1d(blk + u, 8, tmp + u, 8, 11);         // columns: pass 1
#pragma unroll
  for (int v = 0; v < 8; ++v) jd_idct_1d(tmp + 8 * v, 1, blk + 8 * v, 1, 18); // rows: pass 2
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int x = blk[8 * v + u] + 128;                     // libjpeg-turbo's SIMD IDCT saturates (packsswb)
      x = x < 0 ? 0 : (x > 255 ? 255 : x);
      if (u < 4) lo |= (unsigned)x << (8 * u);
      else hi |= (unsigned)x << (8 * (u - 4));
    }
    unsigned* row = (unsigned*)(plane + v * pw);
    row[0] = lo;
    row[1] = hi;
  }
}

// ---- K4: upsample + YCbCr -> RGB ----------------------------------------------------------------------------------
__device__ __forceinline__ int jd_chroma(const unsigned char* p, long long pw, int cw, int ch, int hs, int vs, int x,
                                         int y) {
  if (hs == 1 && vs == 1) return p[(long long)y * pw + x];
  if (cw <= 2) return p[(long long)(y / vs) * pw + x / hs];        // libjpeg: plain replication when width <= 2
  const int i = x >> 1, in = (x & 1) ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
  if (vs == 2) {
    const int r = y >> 1, rn = (y & 1) ? (r + 1 < ch ? r + 1 : ch - 1) : (r > 0 ? r - 1 : 0);
    const unsigned char* a = p + (long long)r * pw;
    const unsigned char* n = p + (long long)rn * pw;
    const int cs = 3 * a[i] + n[i], cn = 3 * a[in] + n[in];
    return (3 * cs + cn + ((x & 1) ? 7 : 8)) >> 4;
  }
  const unsigned char* a = p + (long long)y * pw;
  return (3 * a[i] + a[in] + ((x & 1) ? 2 : 1)) >> 2;
}

__device__ __forceinline__ unsigned jd_clamp8(int v) { return v < 0 ? 0u : (v > 255 ? 255u : (unsigned)v); }

constexpr int kPx = 4;

__global__ __launch_bounds__(256) void k_jd_color(const UdJpegFrame* __restrict__ frames,
                                                  const unsigned char* __restrict__ ws, const int* __restrict__ status,
                                                  unsigned char* __restrict__ out) {
  const UdJpegFrame& f = frames[blockIdx.y];
  const int W = f.width, H = f.height;
  const int groups = (W + kPx - 1) / kPx;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)groups * H) return;
  const int y = (int)(t / groups), x0 = (int)(t - (long long)y * groups) * kPx;
  const int n = W - x0 < kPx ? W - x0 : kPx;
  const bool ok = status[blockIdx.y] == 0;
  unsigned v[3 * kPx] = {};
  const long long pw0 = (long long)f.mcus_x * f.hmax * 8, pwc = f.mcus_x * 8LL;
  const int hs = f.hmax, vs = f.vmax;
  for (int j = 0; j < n && ok; ++j) {
    const int x = x0 + j;
    const int Y = ws[f.ws_plane[0] + (long long)y * pw0 + x];
    const int cb = jd_chroma(ws + f.ws_plane[1], pwc, f.cw[1], f.ch[1], hs, vs, x, y) - 128;
    const int cr = jd_chroma(ws + f.ws_plane[2], pwc, f.cw[2], f.ch[2], hs, vs, x, y) - 128;
    v[3 * j] = jd_clamp8(Y + ((91881 * cr + 32768) >> 16));
    v[3 * j + 1] = jd_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    v[3 * j + 2] = jd_clamp8(Y + ((116130 * cb + 32768) >> 16));
  }
  unsigned char* o = out + f.out_off + ((long long)y * W + x0) * 3;
  if (n == kPx && ((uintptr_t)o & 3) == 0) {
    unsigned* q = (unsigned*)o;
    q[0] = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
    q[1] = v[4] | v[5] << 8 | v[6] << 16 | v[7] << 24;
    q[2] = v[8] | v[9] << 8 | v[10] << 16 | v[11] << 24;
  } else {
    for (int i = 0; i < 3 * n; ++i) o[i] = (unsigned char)v[i];
  }
}

__global__ void k_jd_zero(uint4* __restrict__ p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    p[i] = make_uint4(0, 0, 0, 0);
}

}  // namespace

// ---- host entry points ---------------------------------------------------------------------------------------------
extern "C" int ud_jpeg_parse(const unsigned char* d, int64_t n, UdJpegFrame* out) {
  if (!d || !out || n < 0) return UD_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return UD_JPEG_CORRUPT;
  int64_t pos = 2;
  bool have_qt[4] = {}, have_ht[2][4] = {}, have_sof = false, jfif = false;
  int adobe = -1, restart = 0, H = 0, W = 0, td[3] = {}, ta[3] = {};
  int cid[3] = {}, ch_[3] = {}, cv[3] = {}, ctq[3] = {};
  uint16_t qt[4][64] = {};
  UdJpegHuff* ht = new UdJpegHuff[8];            // [class * 4 + id], 11 KB: off the stack
  auto done = [&](int rc) {
    delete[] ht;
    return rc;
  };
  for (;;) {
    if (pos + 2 > n) return done(UD_JPEG_TRUNCATED);
    if (d[pos] != 0xFF) return done(UD_JPEG_CORRUPT);
    while (pos < n && d[pos] == 0xFF) ++pos;
    if (pos >= n) return done(UD_JPEG_TRUNCATED);
    const int m = d[pos++];
    if (m == 0xD9) return done(UD_JPEG_TRUNCATED);
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) return done(UD_JPEG_CORRUPT);
    if (pos + 2 > n) return done(UD_JPEG_TRUNCATED);
    const int len = d[pos] << 8 | d[pos + 1];
    if (len < 2) return done(UD_JPEG_CORRUPT);
    if (pos + len > n) return done(UD_JPEG_TRUNCATED);
    const unsigned char* seg = d + pos + 2;
    const int sl = len - 2;
    pos += len;
    if (m == 0xE0 && sl >= 5 && !memcmp(seg, "JFIF\0", 5)) {
      jfif = true;
    } else if (m == 0xEE && sl >= 12 && !memcmp(seg, "Adobe", 5)) {
      adobe = seg[11];
    } else if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
    } else if (m == 0xDB) {
      for (int i = 0; i < sl;) {
        const int pq = seg[i] >> 4, tq = seg[i] & 15;
        if (pq > 1 || tq > 3) return done(UD_JPEG_CORRUPT);
        const int w = 64 * (pq + 1);
        if (i + 1 + w > sl) return done(UD_JPEG_CORRUPT);
        for (int k = 0; k < 64; ++k)
          qt[tq][h_natural[k]] = pq ? (uint16_t)(seg[i + 1 + 2 * k] << 8 | seg[i + 2 + 2 * k]) : seg[i + 1 + k];
        have_qt[tq] = true;
        i += 1 + w;
      }
    } else if (m == 0xC4) {
      for (int i = 0; i < sl;) {
        if (i + 17 > sl) return done(UD_JPEG_CORRUPT);
        const int tc = seg[i] >> 4, th = seg[i] & 15;
        int tot = 0;
        for (int l = 0; l < 16; ++l) tot += seg[i + 1 + l];
        if (tc > 1 || th > 3 || tot > 256 || i + 17 + tot > sl) return done(UD_JPEG_CORRUPT);
        if (tc == 0)
          for (int k = 0; k < tot; ++k)
            if (seg[i + 17 + k] > 15) return done(UD_JPEG_CORRUPT);
        if (jd_huff_table(seg + i + 1, seg + i + 17, &ht[tc * 4 + th]) != UD_JPEG_OK) return done(UD_JPEG_CORRUPT);
        have_ht[tc][th] = true;
        i += 17 + tot;
      }
    } else if (m == 0xDD) {
      if (sl != 2) return done(UD_JPEG_CORRUPT);
      restart = seg[0] << 8 | seg[1];
    } else if (m == 0xC0 || m == 0xC1) {
      if (have_sof || sl < 6) return done(UD_JPEG_CORRUPT);
      const int prec = seg[0], nf = seg[5];
      H = seg[1] << 8 | seg[2];
      W = seg[3] << 8 | seg[4];
      if (sl != 6 + 3 * nf) return done(UD_JPEG_CORRUPT);
      if (prec != 8 || nf != 3 || H == 0) return done(UD_JPEG_UNSUPPORTED);
      if (W == 0) return done(UD_JPEG_CORRUPT);
      for (int c = 0; c < 3; ++c)
        cid[c] = seg[6 + 3 * c], ch_[c] = seg[7 + 3 * c] >> 4, cv[c] = seg[7 + 3 * c] & 15, ctq[c] = seg[8 + 3 * c];
      have_sof = true;
    } else if (m == 0xDA) {
      if (!have_sof) return done(UD_JPEG_CORRUPT);
      const int ns = sl > 0 ? seg[0] : 0;
      if (sl != 4 + 2 * ns) return done(UD_JPEG_CORRUPT);
      if (ns != 3) return done(UD_JPEG_UNSUPPORTED);
      for (int c = 0; c < 3; ++c)
        if (seg[1 + 2 * c] != cid[c]) return done(UD_JPEG_UNSUPPORTED);
      if (seg[7] != 0 || seg[8] != 63 || seg[9] != 0) return done(UD_JPEG_UNSUPPORTED);
      for (int c = 0; c < 3; ++c) td[c] = seg[2 + 2 * c] >> 4, ta[c] = seg[2 + 2 * c] & 15;
      break;
    } else if (m == 0xC2 || m == 0xC3 || m == 0xCC || (m >= 0xC5 && m <= 0xCF)) {
      return done(UD_JPEG_UNSUPPORTED);
    } else {
      return done(UD_JPEG_CORRUPT);
    }
  }
  const bool s_ok = ((ch_[0] == 1 && cv[0] == 1) || (ch_[0] == 2 && cv[0] == 1) || (ch_[0] == 2 && cv[0] == 2)) &&
                    ch_[1] == 1 && cv[1] == 1 && ch_[2] == 1 && cv[2] == 1;
  if (!s_ok) return done(UD_JPEG_UNSUPPORTED);
  const bool rgb_ids = (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B') || (cid[0] == 'r' && cid[1] == 'g' && cid[2] == 'b');
  if (adobe == 0 || (adobe < 0 && !jfif && rgb_ids)) return done(UD_JPEG_UNSUPPORTED);
  for (int c = 0; c < 3; ++c)
    if (ctq[c] > 3 || !have_qt[ctq[c]] || td[c] > 3 || ta[c] > 3 || !have_ht[0][td[c]] || !have_ht[1][ta[c]])
      return done(UD_JPEG_CORRUPT);
  // The scan's bytes are taken to the end of the data: k_jd_destuff ends the scan at its first marker other than RSTn
  // (normally EOI; bytes after it are ignored).  Without one the scan was cut short and the decode reports the frame.
  UdJpegFrame* f = out;
  f->width = W, f->height = H, f->hmax = ch_[0], f->vmax = cv[0], f->restart = restart;
  for (int c = 0; c < 3; ++c) {
    f->comp_id[c] = cid[c], f->h[c] = ch_[c], f->v[c] = cv[c];
    memcpy(f->qt[c], qt[ctq[c]], sizeof(f->qt[c]));
    f->huff[2 * c] = ht[td[c]];
    f->huff[2 * c + 1] = ht[4 + ta[c]];
  }
  jd_geometry(f);
  f->ecs_off = pos;
  f->ecs_bytes = n - pos;
  f->total_blocks = (int64_t)f->mcus_x * f->mcus_y * f->bpm;
  f->nsub_max = jd_div_up(f->ecs_bytes * 8, kSub) + f->nseg;
  return done(UD_JPEG_OK);
}

extern "C" size_t ud_jpeg_plan(UdJpegFrame* frames, int N) {
  if (!frames || N <= 0) return 0;
  size_t coef = 0, rest = 0, outb = 0;
  for (int i = 0; i < N; ++i) {
    UdJpegFrame& f = frames[i];
    f.total_blocks = (int64_t)f.mcus_x * f.mcus_y * f.bpm;
    f.nsub_max = jd_div_up(f.ecs_bytes * 8, kSub) + f.nseg;
    if (!jd_record_ok(f)) return 0;
    coef += jd_sizes(f).coef;
  }
  coef = ud_align_up(coef, 256);
  size_t cpos = 0;
  for (int i = 0; i < N; ++i) {
    UdJpegFrame& f = frames[i];
    const JdSizes s = jd_sizes(f);
    f.ws_coef = (int64_t)cpos;
    cpos += s.coef;
    size_t p = coef + rest;
    f.ws_ecs = (int64_t)p, p += s.ecs;
    f.ws_seg = (int64_t)p, p += s.seg;
    f.ws_sub = (int64_t)p, p += s.sub;
    f.ws_state = (int64_t)p, p += s.state;
    f.ws_scan = (int64_t)p, p += s.scan;
    for (int c = 0; c < 3; ++c) f.ws_plane[c] = (int64_t)p, p += s.plane[c];
    rest = p - coef;
    f.out_off = (int64_t)outb;
    outb += (size_t)f.width * f.height * 3;
  }
  return coef + rest;
}

extern "C" int ud_jpeg_decode(const unsigned char* src, int64_t src_bytes, const UdJpegFrame* frames_host,
                              const UdJpegFrame* frames_dev, int N, unsigned char* out, int64_t out_bytes,
                              int32_t* status, int32_t* iters, void* workspace, size_t workspace_bytes,
                              ud_stream_t stream_) {
  if (N == 0) return UD_OK;
  if (N < 0 || N > 65535 || !src || !frames_host || !frames_dev || !out || !status || (uintptr_t)workspace % 16)
    return UD_ERR_INVALID_ARG;
  long long max_blocks = 0, max_groups = 0;
  size_t coef_end = 0;
  for (int i = 0; i < N; ++i) {
    const UdJpegFrame& f = frames_host[i];
    if (!jd_record_ok(f) || f.src_off + f.ecs_off + f.ecs_bytes > src_bytes ||
        f.out_off + (int64_t)f.width * f.height * 3 > out_bytes)
      return UD_ERR_INVALID_ARG;
    const JdSizes s = jd_sizes(f);
    const int64_t regions[][2] = {{f.ws_ecs, (int64_t)s.ecs},   {f.ws_seg, (int64_t)s.seg},
                                  {f.ws_sub, (int64_t)s.sub},   {f.ws_state, (int64_t)s.state},
                                  {f.ws_scan, (int64_t)s.scan}, {f.ws_coef, (int64_t)s.coef},
                                  {f.ws_plane[0], (int64_t)s.plane[0]}, {f.ws_plane[1], (int64_t)s.plane[1]},
                                  {f.ws_plane[2], (int64_t)s.plane[2]}};
    for (const auto& r : regions)
      if (r[0] < 0 || r[0] % 16 || (size_t)(r[0] + r[1]) > workspace_bytes) return UD_ERR_WORKSPACE;
    if (!workspace) return UD_ERR_WORKSPACE;
    coef_end = (size_t)(f.ws_coef + s.coef) > coef_end ? (size_t)(f.ws_coef + s.coef) : coef_end;
    max_blocks = f.total_blocks > max_blocks ? f.total_blocks : max_blocks;
    const long long g = (long long)f.height * ((f.width + kPx - 1) / kPx);
    max_groups = g > max_groups ? g : max_groups;
  }
  hipStream_t stream = (hipStream_t)stream_;
  unsigned char* ws = (unsigned char*)workspace;
  UdProfScope prof("input.k_jpeg_decode", stream);
  // every frame's coefficients lie in [0, coef_end) (ud_jpeg_plan puts them first); zeroed by a kernel, not a memset
  const size_t n16 = (coef_end + 15) / 16;
  if (n16) {
    k_jd_zero<<<(unsigned)(n16 / 256 + 1 < 2048 ? n16 / 256 + 1 : 2048), 256, 0, stream>>>((uint4*)ws, n16);
    UD_LAUNCH_CHECK();
  }
  k_jd_destuff<<<N, kWg, 0, stream>>>(src, frames_dev, ws, status, iters);
  UD_LAUNCH_CHECK();
  k_jd_huffman<<<N, kWg, 0, stream>>>(frames_dev, ws, status, iters);
  UD_LAUNCH_CHECK();
  k_jd_idct<<<dim3((unsigned)ud_div_up(max_blocks, 128), N), 128, 0, stream>>>(frames_dev, ws, status);
  UD_LAUNCH_CHECK();
  k_jd_color<<<dim3((unsigned)ud_div_up(max_groups, 256), N), 256, 0, stream>>>(frames_dev, ws, status, out);
  UD_LAUNCH_CHECK();
  return UD_OK;
}
