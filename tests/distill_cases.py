"""Inputs the distillation-loss tests share; a helper, not a test.

Seeded cases for tests/test_distill_reference_cpu.py (conditions on the inputs) and tests/test_distill_reference_gpu.py (the kernels of
csrc/distill.hip against the restatement of tests/distill_reference.py), each built once on the CPU together with its float64 and
float32 restatement.  Box positions are written in BEV pixels (a, b): a runs over [0, W] and picks the ROW a H / W - 1/2, b runs over
[0, H] and picks the COLUMN b W / H - 1/2 (the reference's column swap, see distill_reference)."""
import functools

import numpy as np

import distill_reference as D

HEADS = ("reg", "height", "dim", "rot", "vel", "iou")
WIDTH = (2, 1, 3, 2, 2, 1)


def _normal(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _rows_from_pixels(rows, pc_min, pixel, S=10):
    """(a, b, length, width, yaw) in pixels -> gt rows f32 [n, S] in metres (z, dz, velocity and label filled with plain values)."""
    out = np.zeros((len(rows), 10), np.float32)
    for i, (a, b, la, lb, yaw) in enumerate(rows):
        out[i] = [pc_min[0] + a * pixel[0], pc_min[1] + b * pixel[1], -1.0, la * pixel[0], lb * pixel[1], 1.5, yaw, 0.5, -0.25, 1 + i % 9]
    return out[:, :S]


# ---- box losses on a non-square map ----------------------------------------------------------------------------------------------
BOX_H, BOX_W, BOX_M = 24, 40, 9
BOX_PC_MIN, BOX_PIXEL = (-10.0, -6.0), (0.5, 0.5)            # the world origin is pixel (20, 12)
BOX_CHANNELS = (1, 63, 64, 65, 130)
# sample 0: rows 0..6 valid, 7..8 padding
BOX_ROWS_0 = dict(inside=0, low_a=1, high_a=2, low_b=3, high_b=4, outside=5, agree=6)
# sample 1: rows 0..6 valid (row 3 is all zero: valid, a zero-size box at the world origin), 7..8 padding
BOX_ROWS_1 = dict(centre=0, minus_half=1, w_minus_half=2, zero_row=3, zero_size=4, twin_a=5, twin_b=6)


@functools.lru_cache(maxsize=None)
def box_geometry():
    """-> dict: gt f32 [2,9,10], corners f32 [2,9,4,2] (box_corners of gt, the exact key points written in afterwards), valid [2,9]."""
    gt = np.zeros((2, BOX_M, 10), np.float32)
    gt[0, :7] = _rows_from_pixels([(20.3, 11.7, 6.0, 3.0, 0.4),          # fully inside
                                   (0.4, 8.2, 5.0, 2.5, 0.2),            # straddles a = 0 (rows above the map)
                                   (39.8, 15.1, 4.0, 3.0, -0.3),         # straddles a = W
                                   (12.6, 0.3, 3.0, 4.0, 1.1),           # straddles b = 0 (columns left of the map)
                                   (27.2, 23.9, 5.0, 2.0, 2.0),          # straddles b = H
                                   (-15.0, -12.0, 4.0, 2.0, 0.7),        # entirely outside
                                   (8.0, 18.0, 3.0, 2.0, 0.5)],          # student == teacher on every pixel it touches
                                  BOX_PC_MIN, BOX_PIXEL)
    gt[1, :7] = _rows_from_pixels([(25.3, 15.35, 5.6, 3.7, 0.0),         # corner 0 written to a pixel centre below
                                   (12.6, 2.05, 4.6, 4.1, 0.0),          # corners 0 and 3 written to column -1/2 below
                                   (32.4, 21.85, 4.4, 4.3, 0.0),         # corners 1 and 2 written to column W - 1/2 below
                                   (0.0, 0.0, 0.0, 0.0, 0.0),            # replaced by an all-zero row
                                   (17.3, 9.6, 0.0, 0.0, 0.9),           # zero size: nine key points on one spot
                                   (30.5, 6.4, 3.5, 2.5, -0.8),          # two identical boxes
                                   (30.5, 6.4, 3.5, 2.5, -0.8)],
                                  BOX_PC_MIN, BOX_PIXEL)
    gt[1, 3] = 0.0
    gt[1, 6] = gt[1, 5]
    corners, valid = D.box_corners(gt, BOX_PC_MIN, BOX_PIXEL)
    corners = corners.copy()
    f = np.float32
    # (a, b) = (22.5, 13.5): row 22.5 * 24 / 40 - 1/2 = 13, column 13.5 * 40 / 24 - 1/2 = 22, both exact in float32
    corners[1, 0] = [[f(22.5), f(13.5)], [f(22.5), f(17.2)], [f(28.1), f(17.2)], [f(28.1), f(13.5)]]
    # b = 0 -> column -1/2: the west taps are padding, the east taps (column 0) weigh 1/2
    corners[1, 1] = [[f(10.3), f(0.0)], [f(10.3), f(4.1)], [f(14.9), f(4.1)], [f(14.9), f(0.0)]]
    # b = H -> column W - 1/2: the east taps are padding
    corners[1, 2] = [[f(30.2), f(19.7)], [f(30.2), f(24.0)], [f(34.6), f(24.0)], [f(34.6), f(19.7)]]
    return dict(gt=gt, corners=corners, valid=valid, corners_of_gt=D.box_corners(gt, BOX_PC_MIN, BOX_PIXEL))


def _agree(s, t, corners, valid, rows):
    """Make the student equal the teacher on every pixel the boxes `rows` = [(b, m)] touch -> the pixel sets."""
    B, C, H, W = s.shape
    tp = D.taps(D.key_points(corners), H, W)
    pix = []
    for b, m in rows:
        p = np.unique(tp["pix"][b, m][tp["inside"][b, m]])
        s.reshape(B, C, H * W)[b][:, p] = t.reshape(B, C, H * W)[b][:, p]
        pix.append((b, p))
    return pix


def _both(fn, *args, **kw):
    return {"f64": fn(*args, dtype=np.float64, **kw), "f32": fn(*args, dtype=np.float32, **kw)}


BOX_UPSTREAM = 1.75          # the gradient that arrives at the loss


@functools.lru_cache(maxsize=None)
def box_case(kind, C):
    """kind 0 feature / 1 relation, C channels -> dict: s, t f32 [2,C,24,40], corners, valid, agree_pixels, f64 / f32 results."""
    geo = box_geometry()
    s = _normal(100 + C, 2, C, BOX_H, BOX_W)
    t = 3 * _normal(200 + C, 2, C, BOX_H, BOX_W)                         # 3x: the Gram difference's diagonal has a decided sign
    agree = _agree(s, t, geo["corners"], geo["valid"], [(0, BOX_ROWS_0["agree"])])
    fn = D.relation_loss if kind else D.feature_loss
    out = dict(s=s, t=t, corners=geo["corners"], valid=geo["valid"], agree_pixels=agree, upstream=BOX_UPSTREAM)
    out.update(_both(fn, s, t, geo["corners"], geo["valid"], upstream=BOX_UPSTREAM))
    return out


# ---- the deterministic scatter ---------------------------------------------------------------------------------------------------
SCATTER_CASES = {
    "m56": dict(M=56, H=32, W=32, C=8, B=2),           # 2016 terms: the 2048-entry LDS sort, nearly full
    "m57": dict(M=57, H=32, W=32, C=8, B=2),           # 2052 terms: the first size of the 4096-entry sort
    "m227": dict(M=227, H=32, W=32, C=8, B=2),         # 8172 terms: the largest LDS sort (8192 entries, 80 KB)
    "m228": dict(M=228, H=32, W=32, C=8, B=2),         # 8208 terms: the rank sort
    "m455": dict(M=455, H=32, W=32, C=8, B=2),         # 16380 / 16416 terms: where the boundary was meant to be; a 16384-entry LDS
    "m456": dict(M=456, H=32, W=32, C=8, B=2),         # sort does not fit a CU (M = 228..455 used to fail at launch), both rank-sort
    "map512": dict(M=300, H=512, W=512, C=4, B=1),     # 10800 terms on 2^18 pixels: the rank sort
    "map_wide": dict(M=200, H=512, W=1024, C=2, B=1),  # 7200 terms would fit the LDS sort, H W = 2^19 = 2^(32 - 13) does not
}


def _scatter_rows(rng, n, H, W, crowd):
    a0, b0 = 0.5 * W + 0.1, 0.5 * H - 0.2
    if crowd:       # sub-pixel boxes around one spot: their terms fall on a handful of pixels, runs of hundreds of terms
        return np.stack([a0 + rng.uniform(-0.2, 0.2, n), b0 + rng.uniform(-0.2, 0.2, n), rng.uniform(0.3, 0.9, n),
                         rng.uniform(0.3, 0.9, n), rng.uniform(-3, 3, n)], 1)
    lim = min(H, W, 32)
    return np.stack([a0 + rng.uniform(-0.25, 0.25, n) * lim, b0 + rng.uniform(-0.25, 0.25, n) * lim, rng.uniform(1, 5, n),
                     rng.uniform(1, 5, n), rng.uniform(-3, 3, n)], 1)


@functools.lru_cache(maxsize=None)
def scatter_geometry(name):
    """-> corners f32 [B,M,4,2], valid [B,M] (three rows in the middle are padding; the first and the LAST row are valid boxes that sit
    alone), with every box's relation-loss decisions at least MARGIN from zero (undecided rows are drawn again)."""
    cfg = SCATTER_CASES[name]
    M, H, W, C, B = (cfg[k] for k in "MHWCB")
    rng = np.random.default_rng(4000 + M)
    crowd = np.arange(M) % 5 < 3
    rows = np.zeros((B, M, 5))
    for b in range(B):
        rows[b, crowd] = _scatter_rows(rng, int(crowd.sum()), H, W, True)
        rows[b, ~crowd] = _scatter_rows(rng, int((~crowd).sum()), H, W, False)
        rows[b, 0] = (3.3 + b, 4.6, 2.0, 1.5, 0.3)                       # alone in a corner of the map
        rows[b, M - 1] = (W - 1.2, H - 0.7, 1.0, 1.0, 0.2 + b)           # the last term indices, on the last pixels (partly padding)
    valid = np.ones((B, M), bool)
    valid[:, M // 2:M // 2 + 3] = False
    s, t = scatter_maps(name)
    for _ in range(50):
        gt = np.stack([_rows_from_pixels(rows[b], (0.0, 0.0), (1.0, 1.0)) for b in range(B)])
        corners, _ = D.box_corners(gt, (0.0, 0.0), (1.0, 1.0))
        und = np.zeros((B, M), bool)
        for dt in (np.float64, np.float32):
            dec = D.relation_loss(s, t, corners, valid, dtype=dt)["decision"]
            und |= ((dec != 0) & (np.abs(dec) < 2 * D.MARGIN)).any(-1) & valid
        if not und.any():
            return corners, valid
        for b, m in zip(*np.nonzero(und)):
            rows[b, m] = _scatter_rows(rng, 1, H, W, bool(crowd[m]))[0]
    raise AssertionError("could not draw boxes away from the relation loss's decisions")


@functools.lru_cache(maxsize=None)
def scatter_maps(name):
    cfg = SCATTER_CASES[name]
    M, H, W, C, B = (cfg[k] for k in "MHWCB")
    return _normal(300 + M, B, C, H, W), 3 * _normal(400 + M, B, C, H, W)


@functools.lru_cache(maxsize=None)
def scatter_case(name, kind):
    corners, valid = scatter_geometry(name)
    s, t = scatter_maps(name)
    fn = D.relation_loss if kind else D.feature_loss
    out = dict(s=s, t=t, corners=corners, valid=valid, upstream=BOX_UPSTREAM)
    out.update(_both(fn, s, t, corners, valid, upstream=BOX_UPSTREAM))
    return out


def longest_run(res, valid):
    """-> the largest number of terms (box, key point, tap) of one sample that fall on one pixel."""
    tp = res["taps"]
    best = 0
    for b in range(valid.shape[0]):
        sel = tp["inside"][b] & valid[b][:, None, None]
        best = max(best, int(np.bincount(tp["pix"][b][sel]).max()))
    return best


ACC_SCALE = 0.375            # the device scalar handed to the accumulate entry point


@functools.lru_cache(maxsize=None)
def acc_case(kind):
    """The accumulate entry point on the m57 boxes: prefill f32 [B,C,H,W] (what the map holds before) and per dtype the map after,
    prefill + ACC_SCALE * d(sum of the valid boxes' losses)/ds, as float64."""
    c = scatter_case("m57", kind)
    prefill = _normal(77 + kind, *c["s"].shape)
    nvalid = float(c["valid"].sum()) + 1e-4                              # the restatement's gradient is of sum / (count + 1e-4)
    out = dict(c, prefill=prefill, scale=ACC_SCALE)
    for key, dt in (("f64", np.float64), ("f32", np.float32)):
        g = c[key]["grad"] * (nvalid * ACC_SCALE / BOX_UPSTREAM)
        out["after_" + key] = (prefill.astype(dt) + g.astype(dt)).astype(np.float64)
    return out


# ---- response loss ---------------------------------------------------------------------------------------------------------------
RESP_B, RESP_H, RESP_W = 2, 17, 19                                       # 323 pixels: two workgroups, the second ragged
RESP_NCLS = {6: (1, 2, 2, 1, 2, 2), 8: (1, 2, 2, 1, 2, 2, 1, 2), 9: (1, 2, 2, 1, 2, 2, 1, 2, 1)}
RESP_W_CLS, RESP_W_REG = 1.0, 2.0
# (sample, pixel) of the constructed pixels
PIX_TIE, PIX_EQ, PIX_LOW, PIX_REG, PIX_MASK0 = (0, 5), (1, 300), (0, 100), (1, 17), ((0, 322), (1, 0), (1, 256))
TIE_AT = ((1, 1), (4, 0))                                                # (task, channel) of the two equal student maxima


@functools.lru_cache(maxsize=None)
def response_case(ntasks, clamp):
    """-> dict: s_hm / t_hm (ntasks arrays [B,ncls,H,W]), s_reg / t_reg (6 ntasks arrays, task-major in HEADS order), mask [B,H,W],
    lo, hi (float32), f64 / f32 results of d(1 cls + 2 reg)."""
    ncls = RESP_NCLS[ntasks]
    B, H, W = RESP_B, RESP_H, RESP_W
    rng = np.random.default_rng(900 + ntasks)
    lo, hi = np.float32(clamp), np.float32(1.0 - clamp)
    nrm = lambda *s: rng.standard_normal(s)
    s_hm = [np.clip(1 / (1 + np.exp(-2 * nrm(B, n, H * W))), clamp, 1 - clamp).astype(np.float32) for n in ncls]
    t_hm = [(3 * nrm(B, n, H * W)).astype(np.float32) for n in ncls]
    s_reg = [nrm(B, wd, H * W).astype(np.float32) for _ in ncls for wd in WIDTH]
    t_reg = [(x + 0.5 * nrm(*x.shape)).astype(np.float32) for x in s_reg]
    mask = rng.uniform(0, 1, (B, H * W)).astype(np.float32)
    mask[rng.uniform(0, 1, (B, H * W)) < 0.3] = 0.0
    for b, p in (PIX_TIE, PIX_EQ, PIX_LOW, PIX_REG):
        mask[b, p] = 0.5 + 0.25 * b
    for b, p in PIX_MASK0:
        mask[b, p] = 0.0
    # teacher logits at +-40: both sides of the clamp
    for x in t_hm:
        x[rng.uniform(0, 1, x.shape) < 0.02] = 40.0
        x[rng.uniform(0, 1, x.shape) < 0.02] = -40.0
    b, p = PIX_LOW
    for x in t_hm:
        x[b, :, p] = -40.0                                               # every channel: the teacher maximum is the lower bound
    b, p = PIX_TIE
    for x in s_hm:
        x[b, :, p] = np.minimum(x[b, :, p], np.float32(0.9))
    if ntasks > TIE_AT[1][0]:
        for ti, ch in TIE_AT:
            s_hm[ti][b, ch, p] = np.float32(0.93)                        # two equal maxima in different tasks
    for x in t_hm:
        x[b, :, p] = np.minimum(x[b, :, p], np.float32(1.0))             # teacher maximum below sigmoid(1/2) = 0.62: d > 0 decided
    b, p = PIX_EQ
    t_hm[0][b, 0, p] = 40.0
    s_hm[min(2, ntasks - 1)][b, 0, p] = hi                               # student maximum == teacher maximum == hi: d = 0 exactly
    b, p = PIX_REG
    for xs, xt in zip(s_reg, t_reg):
        xt[b, :, p] = xs[b, :, p]
    shape = lambda xs: [x.reshape(B, -1, H, W) for x in xs]
    out = dict(s_hm=shape(s_hm), t_hm=shape(t_hm), s_reg=shape(s_reg), t_reg=shape(t_reg), mask=mask.reshape(B, H, W), lo=lo, hi=hi,
               ncls=ncls, clamp=clamp)
    if ntasks <= 8:
        out.update(_both(D.response_loss, out["s_hm"], out["t_hm"], out["s_reg"], out["t_reg"], out["mask"], lo, hi, RESP_W_CLS,
                         RESP_W_REG))
    return out


# ---- Gaussian mask ---------------------------------------------------------------------------------------------------------------
MASK_B, MASK_M, MASK_H, MASK_W = 3, 12, 20, 28
MASK_PIXEL = (0.075 * 8, 0.1 * 8)
MASK_PC_MIN = (-0.5 * MASK_W * MASK_PIXEL[0], -0.5 * MASK_H * MASK_PIXEL[1])
MASK_R = 3
FAR = 1000


def _mask_row(cx, cy, r, yaw=0.3):
    """A gt row whose mask box is (cx, cy, r): the centre half a pixel inside its cell (on the far side of zero for a negative index,
    since the centre is truncated), both sides (r + 1/2) / 0.2735 pixels (radius = 0.2735.. x side for a square box)."""
    half = lambda i: i + 0.5 if i >= 0 else i - 0.5
    side = (r + 0.5) / 0.2735 if r > 0 else 0.5
    return [MASK_PC_MIN[0] + half(cx) * MASK_PIXEL[0], MASK_PC_MIN[1] + half(cy) * MASK_PIXEL[1], -1.0, side * MASK_PIXEL[0],
            side * MASK_PIXEL[1], 1.5, yaw, 0.5, -0.25, 2.0]


@functools.lru_cache(maxsize=None)
def mask_gt():
    """-> (gt f32 [3,12,10], expected (cx, cy, r) of the drawn rows per sample for S = 10)."""
    r, H, W = MASK_R, MASK_H, MASK_W
    gt = np.zeros((MASK_B, MASK_M, 10), np.float32)
    out_by = (r - 1, r, r + 1, FAR)                                      # less than r, exactly r, r + 1, far
    s0 = [(-d, 2 + 5 * i if d != FAR else 7, r) for i, d in enumerate(out_by)] + \
         [(W - 1 + d, 4 + 5 * i if d != FAR else 9, r) for i, d in enumerate(out_by)]
    s1 = [(3 + 7 * i if d != FAR else 5, -d, r) for i, d in enumerate(out_by)] + \
         [(5 + 7 * i if d != FAR else 8, H - 1 + d, r) for i, d in enumerate(out_by)]
    for b, rows in enumerate((s0, s1)):
        for m, (cx, cy, rr) in enumerate(rows):
            gt[b, m] = _mask_row(cx, cy, rr)
    gt[0, 8] = _mask_row(14, 3, 0)                                       # radius 0: one pixel
    gt[0, 9] = _mask_row(20, 16, 0)
    gt[0, 9, 3:5] = 0.0                                                  # dimensions 0
    gt[0, 10] = _mask_row(9, 18, 0)
    gt[0, 10, 3] = np.nan                                                # a NaN dimension: radius 0, still drawn
    gt[0, 11] = _mask_row(1, 4, r)                                       # overlaps row 0 (centre (-2, 2)): the maximum
    s0 = s0 + [(14, 3, 0), (20, 16, 0), (9, 18, 0), (1, 4, r)]
    gt[1, 8] = 0.0
    gt[1, 8, 8] = 0.25                                                   # zero in the seven box columns, not in column 8: a box of
    s1 = s1 + [(MASK_W // 2, MASK_H // 2, 0)]                            # size 0 at the world origin (S >= 9); a zero row for S = 7
    # row 9 stays all zero; rows 10, 11 are real boxes the mask never reaches, `valid` covers them
    gt[1, 10] = _mask_row(20, 10, r)
    gt[1, 11] = _mask_row(6, 12, 1)
    # centre at -1/2 pixel would truncate to 0; sample 2 is all zero
    return gt, [s0, s1, []]


@functools.lru_cache(maxsize=None)
def mask_case(S):
    gt, expect = mask_gt()
    gt = np.ascontiguousarray(gt[:, :, :S])
    if S == 7:
        expect = [expect[0], expect[1][:8], []]
    _, valid = D.box_corners(gt, MASK_PC_MIN, MASK_PIXEL)
    return dict(gt=gt, expect=expect, mask=D.gaussian_mask(gt, MASK_PC_MIN, MASK_PIXEL, MASK_H, MASK_W), valid=valid)


@functools.lru_cache(maxsize=None)
def mask_case_m1():
    """M = 1: a box inside, an all-zero sample, and a box whose centre truncates from -1/2 pixel to cell 0."""
    gt = np.zeros((3, 1, 10), np.float32)
    gt[0, 0] = _mask_row(5, 6, 2)
    gt[2, 0] = _mask_row(0, 3, 1)
    gt[2, 0, 0] = MASK_PC_MIN[0] - 0.5 * MASK_PIXEL[0]
    _, valid = D.box_corners(gt, MASK_PC_MIN, MASK_PIXEL)
    return dict(gt=gt, expect=[[(5, 6, 2)], [], [(0, 3, 1)]], mask=D.gaussian_mask(gt, MASK_PC_MIN, MASK_PIXEL, MASK_H, MASK_W),
                valid=valid)
