"""The distillation losses and the Gaussian box mask written out in numpy / PyTorch on the CPU; a helper, not a test.

What csrc/distill.hip computes (k_box_corners, k_feat, k_rel, the deterministic scatter, k_mask_*, k_resp), restated from the
definition of the operations: the computation runs in the dtype it is asked for (float64 is the yardstick, float32 measures what single
precision costs), calls no project op and no grid_sample.  tests/test_distill_reference_cpu.py ties the float64 evaluation to the
reference goldens of tests/golden/distill.npz; tests/test_distill_reference_gpu.py holds the kernels against it.

Conventions the kernels document and this file follows:
  * corners: rotation in double on the float32 box (sine and cosine in the asked dtype), the world corner rounded to float32, then
    (corner - pc_min) / pixel in float32;
  * key points (a, b) of a box in BEV pixels: column 0 is normalised by W, column 1 by H, then the columns are SWAPPED, so the
    width-direction sample coordinate is b W / H - 1/2 and the height-direction one a H / W - 1/2 (the reference's quirk: on a square map
    it is a plain transposition, on H != W a key point inside the map's [0, W] x [0, H] still lands inside);
  * bilinear taps with zero padding: a tap outside the map contributes nothing and receives no gradient;
  * `valid` runs to the LAST row whose S entries do not sum to zero (float32, column order) and never below row 0; the mask stops at
    the FIRST zero-sum row;
  * mask: radius and centre in double on the float32 box, max(0, int(r)) with NaN -> 0, centre truncated toward zero, the Gaussian in
    double and rounded to float32, drawn with Python's slice semantics (a window that is empty on either side draws nothing);
  * response loss: the teacher's probability is clamp(sigmoid(logit / 2), lo, hi) with lo, hi given as float32; on an exact tie of the
    student maximum the gradient goes to the first channel in concatenation order (task, then channel).

Decisions.  |x| has a one-sided derivative at 0, so a gradient value that depends on the sign of a quantity which a float32 evaluation
cannot decide is left out of gradient comparisons.  A decision quantity d = p - q counts as undecided when 0 < |d| < MARGIN * scale, scale
being the magnitude of what was subtracted (sum of |tap weight * value| of both samples; 1 for a Gram entry, whose operands are cosines).
An exact zero is decided: both precisions produce it by the same cancellation (equal inputs, or taps that are all padding).
MARGIN is 32 float32 epsilons: a bilinear sample is a 4-term sum (<= 4 eps of its magnitude), a Gram entry of normalised rows of at most
130 channels goes through a norm, two divisions and a tree-ordered dot product (<= about 10 eps), and 3x headroom on top.
"""
import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
MARGIN = 32 * EPS32
PAIRS = ((0, 1), (1, 2), (2, 3), (0, 3))            # the corners whose mid-points are key points 5..8


def _np_dtype(dtype):
    return np.float64 if dtype in (np.float64, torch.float64) else np.float32


def _torch_dtype(dtype):
    return torch.float64 if _np_dtype(dtype) is np.float64 else torch.float32


def row_sums(gt):
    """gt f32 [B,M,S] -> float32 sums of every row, added in column order."""
    gt = np.asarray(gt, np.float32)
    s = np.zeros(gt.shape[:2], np.float32)
    for k in range(gt.shape[2]):
        s = (s + gt[..., k]).astype(np.float32)
    return s


# ---- corners and validity --------------------------------------------------------------------------------------------------------
def box_corners(gt, pc_range, pixel, dtype=np.float64):
    """gt f32 [B,M,S] (x y z dx dy dz yaw ...), pixel = (size_x, size_y) in metres -> (corners f32 [B,M,4,2] in BEV pixels, valid bool
    [B,M])."""
    gt = np.asarray(gt, np.float32)
    B, M, _ = gt.shape
    yaw = gt[..., 6].astype(_np_dtype(dtype))
    sn, cs = np.sin(yaw).astype(np.float64)[..., None], np.cos(yaw).astype(np.float64)[..., None]
    lx = gt[..., 3, None].astype(np.float64) * np.array([-0.5, -0.5, 0.5, 0.5])
    ly = gt[..., 4, None].astype(np.float64) * np.array([-0.5, 0.5, 0.5, -0.5])
    wx = lx * cs - ly * sn + gt[..., 0, None].astype(np.float64)
    wy = lx * sn + ly * cs + gt[..., 1, None].astype(np.float64)
    world = np.stack([wx, wy], -1).astype(np.float32)
    lo = np.array([pc_range[0], pc_range[1]], np.float64).astype(np.float32)
    px = np.array([pixel[0], pixel[1]], np.float64).astype(np.float32)
    corners = ((world - lo) / px).astype(np.float32)
    nz = row_sums(gt) != 0
    valid = np.zeros((B, M), bool)
    for b in range(B):
        last = max([m for m in range(M) if nz[b, m]] + [0])
        valid[b, :last + 1] = True
    return corners, valid


# ---- key points and taps ---------------------------------------------------------------------------------------------------------
def key_points(corners, dtype=np.float64):
    """corners [B,M,4,2] -> the nine key points [B,M,9,2]: corners, centre, the four edge mid-points."""
    c = np.asarray(corners).astype(_np_dtype(dtype))
    mids = [(c[:, :, i] + c[:, :, j]) / 2 for i, j in PAIRS]
    centre = (((c[:, :, 0] + c[:, :, 1]) + c[:, :, 2]) + c[:, :, 3]) / 4
    return np.concatenate([c, centre[:, :, None], np.stack(mids, 2)], 2)


def sample_coords(kp, H, W):
    """key points [...,2] in BEV pixels -> (ix, iy), the sample position in units of pixel centres (column, row)."""
    dt = kp.dtype.type
    a0 = (kp[..., 0] - dt(W) / 2) / (dt(W) / 2)
    a1 = (kp[..., 1] - dt(H) / 2) / (dt(H) / 2)
    gx, gy = a1, a0                                      # the swap
    return ((gx + 1) * dt(W) - 1) / 2, ((gy + 1) * dt(H) - 1) / 2


def taps(kp, H, W):
    """-> dict: pix int64 [...,4] (linear pixel y W + x of the nw, ne, sw, se tap; 0 where outside), w [...,4], inside bool [...,4]."""
    ix, iy = sample_coords(kp, H, W)
    x0, y0 = np.floor(ix), np.floor(iy)
    wx = np.stack([(x0 + 1) - ix, ix - x0], -1)          # west, east
    wy = np.stack([(y0 + 1) - iy, iy - y0], -1)          # north, south
    xs = np.stack([x0, x0 + 1], -1).astype(np.int64)
    ys = np.stack([y0, y0 + 1], -1).astype(np.int64)
    x = np.stack([xs[..., 0], xs[..., 1], xs[..., 0], xs[..., 1]], -1)
    y = np.stack([ys[..., 0], ys[..., 0], ys[..., 1], ys[..., 1]], -1)
    w = np.stack([wx[..., 0] * wy[..., 0], wx[..., 1] * wy[..., 0], wx[..., 0] * wy[..., 1], wx[..., 1] * wy[..., 1]], -1)
    inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    return dict(pix=np.where(inside, y * W + x, 0), w=w.astype(kp.dtype), inside=inside, ix=ix, iy=iy)


def _sample(fmap, tp):
    """fmap torch [B,C,H,W], taps of [B,M,9] key points -> (samples [B,M,9,C], magnitude sum |w v| [B,M,9,C])."""
    B, C, H, W = fmap.shape
    M = tp["pix"].shape[1]
    flat = fmap.reshape(B, C, H * W)
    w = torch.from_numpy(np.where(tp["inside"], tp["w"], 0)).to(fmap.dtype)
    pix = torch.from_numpy(tp["pix"])
    val, mag = [], []
    for b in range(B):
        v = flat[b][:, pix[b].reshape(-1)].reshape(C, M, 9, 4) * w[b]
        val.append(v.sum(-1).permute(1, 2, 0))
        mag.append(v.detach().abs().sum(-1).permute(1, 2, 0))
    return torch.stack(val), torch.stack(mag)


def touched_pixels(tp, valid, H, W):
    """-> bool [B, H W]: pixels that a tap of a valid box lies on."""
    B = valid.shape[0]
    out = np.zeros((B, H * W), bool)
    for b in range(B):
        sel = tp["inside"][b] & valid[b][:, None, None]
        out[b, tp["pix"][b][sel]] = True
    return out


def _flag_pixels(tp, und, H, W, C):
    """und bool [B,M,9,C] (an undecided term per key point and channel) -> bool [B,C,H,W]: the gradient values it enters."""
    B = und.shape[0]
    out = np.zeros((B, H * W, C), bool)
    for b in range(B):
        sel = tp["inside"][b]                                       # [M,9,4]
        flags = np.broadcast_to(und[b][:, :, None, :], sel.shape + (C,))[sel]
        np.logical_or.at(out[b], tp["pix"][b][sel], flags)
    return out.transpose(0, 2, 1).reshape(B, C, H, W)


def _box_loss(kind, s, t, corners, valid, dtype, upstream):
    td = _torch_dtype(dtype)
    valid = np.asarray(valid, bool)
    B, C, H, W = s.shape
    tp = taps(key_points(corners, dtype), H, W)
    sm = torch.from_numpy(np.asarray(s)).to(td).clone().requires_grad_(True)
    tm = torch.from_numpy(np.asarray(t)).to(td)
    fs, ms = _sample(sm, tp)
    ft, mt = _sample(tm, tp)
    v = torch.from_numpy(valid)
    if kind == 0:
        d = fs - ft                                                  # [B,M,9,C]
        per_box = d.abs().mean(3).mean(2)
        dec = d.detach().double().numpy()
        scale = (ms + mt).double().numpy()
        und = (dec != 0) & (np.abs(dec) < MARGIN * scale) & valid[:, :, None, None]
    else:
        hs = fs / (torch.linalg.vector_norm(fs, dim=-1, keepdim=True) + 1e-4)
        ht = ft / (torch.linalg.vector_norm(ft, dim=-1, keepdim=True) + 1e-4)
        d = (hs @ hs.transpose(-1, -2) - ht @ ht.transpose(-1, -2)).reshape(B, -1, 81)
        per_box = d.abs().mean(2)
        dec = d.detach().double().numpy()
        box_und = ((dec != 0) & (np.abs(dec) < MARGIN)).any(-1) & valid
        und = np.broadcast_to(box_und[:, :, None, None], valid.shape + (9, C))
    loss = torch.where(v, per_box, torch.zeros((), dtype=td)).sum() / (v.to(td).sum() + 1e-4)
    grad, = torch.autograd.grad(loss * upstream, sm)
    return dict(loss=float(loss.detach()), grad=grad.double().numpy(), decision=dec, left_out=_flag_pixels(tp, und, H, W, C),
                touched=touched_pixels(tp, valid, H, W), taps=tp)


def feature_loss(s, t, corners, valid, dtype=np.float64, upstream=1.0):
    """Student and teacher maps [B,C,H,W], corners [B,M,4,2] in BEV pixels, valid [B,M] -> dict: loss = sum over valid boxes of the mean
    over 9 key points and C channels of |s - t| sampled there, over (number of valid boxes + 1e-4); grad = d(upstream loss)/ds
    [B,C,H,W]; decision = the sampled s - t [B,M,9,C]; left_out [B,C,H,W] = gradient values an undecided sign enters; touched [B, H W]."""
    return _box_loss(0, s, t, corners, valid, dtype, upstream)


def relation_loss(s, t, corners, valid, dtype=np.float64, upstream=1.0):
    """As feature_loss for the relation loss: the nine sampled rows f are normalised f / (|f| + 1e-4), G = F F^T, the loss of a box is the
    mean over the 81 entries of |Gs - Gt|; decision = Gs - Gt [B,M,81].  One undecided entry leaves out every value the box touches."""
    return _box_loss(1, s, t, corners, valid, dtype, upstream)


# ---- Gaussian box mask -----------------------------------------------------------------------------------------------------------
def gaussian_radius(a, b, min_overlap=0.7):
    """The smallest of the three radii at which a box a x b shifted by r still overlaps itself by min_overlap; double, NaN propagates."""
    with np.errstate(invalid="ignore"):
        a, b = np.float64(a), np.float64(b)
        b1, c1 = a + b, a * b * (1 - min_overlap) / (1 + min_overlap)
        r1 = (b1 + np.sqrt(b1 * b1 - 4 * c1)) / 2
        b2, c2 = 2 * (a + b), (1 - min_overlap) * a * b
        r2 = (b2 + np.sqrt(b2 * b2 - 16 * c2)) / 2
        a3, b3, c3 = 4 * min_overlap, -2 * min_overlap * (a + b), (min_overlap - 1) * a * b
        r3 = (b3 + np.sqrt(b3 * b3 - 4 * a3 * c3)) / 2
    rs = [r1, r2, r3]
    return np.float64("nan") if any(np.isnan(r) for r in rs) else min(rs)


def mask_boxes(gt, pc_range, pixel):
    """-> per sample the list of (cx, cy, r) of the rows the mask draws: every row before the first zero-sum row."""
    gt = np.asarray(gt, np.float32)
    sums = row_sums(gt)
    out = []
    for b in range(gt.shape[0]):
        rows = []
        for m in range(gt.shape[1]):
            if sums[b, m] == 0:
                break
            g = gt[b, m].astype(np.float64)
            r = gaussian_radius(g[3] / pixel[0], g[4] / pixel[1])
            r = int(r) if r > 0 else 0                               # NaN compares false
            rows.append((int((g[0] - pc_range[0]) / pixel[0]), int((g[1] - pc_range[1]) / pixel[1]), r))
        out.append(rows)
    return out


def gaussian_mask(gt, pc_range, pixel, H, W):
    """gt f32 [B,M,S] -> mask f32 [B,H,W]: the running maximum of one Gaussian window per box, sigma = (2 r + 1) / 6."""
    boxes = mask_boxes(gt, pc_range, pixel)
    out = np.zeros((len(boxes), H, W), np.float32)
    for b, rows in enumerate(boxes):
        for cx, cy, r in rows:
            ax = np.arange(-r, r + 1, dtype=np.float64)
            sigma = (2 * r + 1) / 6
            g = np.exp(-(ax[None, :] ** 2 + ax[:, None] ** 2) / (2 * sigma * sigma))
            west, east = min(cx, r), min(W - cx, r + 1)              # how far the window reaches to either side of the centre
            north, south = min(cy, r), min(H - cy, r + 1)
            dst = out[b, cy - north:cy + south, cx - west:cx + east]
            src = g[r - north:r + south, r - west:r + east]
            if dst.size and src.size:                                 # either one empty: nothing is drawn
                np.maximum(dst, src, out=dst, casting="same_kind")
    return out


# ---- response loss ---------------------------------------------------------------------------------------------------------------
def response_loss(s_hm, t_hm, s_reg, t_reg, mask, lo, hi, w_cls=1.0, w_reg=1.0, dtype=np.float64):
    """Lists of arrays [B,ch,H,W] (student heat maps as they are, teacher heat maps as logits, regression tensors), mask [B,H,W], the
    clamp bounds lo, hi (float32 values) -> dict: cls, reg (the two losses), g_hm, g_reg (lists: d(w_cls cls + w_reg reg)/d student),
    left_out bool [B,H,W] (pixels whose sign(smax - tmax) is undecided), decision = smax - tmax."""
    dt = _np_dtype(dtype)
    S = np.concatenate([np.asarray(x) for x in s_hm], 1).astype(dt)
    L = np.concatenate([np.asarray(x) for x in t_hm], 1).astype(dt)
    P = np.clip(dt(1) / (dt(1) + np.exp(-(L / dt(2)))), dt(np.float32(lo)), dt(np.float32(hi)))
    mk = np.asarray(mask).astype(dt)
    arg = S.argmax(1)                                                # the first of equal maxima
    smax, tmax = S.max(1), P.max(1)
    d = smax - tmax
    den = mk.sum(dtype=dt) + dt(1e-4)
    R = np.concatenate([np.asarray(x) for x in s_reg], 1).astype(dt) - np.concatenate([np.asarray(x) for x in t_reg], 1).astype(dt)
    nreg = R.shape[1]
    cls = (np.abs(d) * mk).sum(dtype=dt) / den
    reg = (np.abs(R).sum(1, dtype=dt) / dt(nreg) * mk).sum(dtype=dt) / den
    g_cat = np.zeros_like(S)
    np.put_along_axis(g_cat, arg[:, None], (np.sign(d) * mk * (dt(w_cls) / den))[:, None], 1)
    g_r = np.sign(R) * (mk * (dt(w_reg) / den) / dt(nreg))[:, None]
    split = lambda a, like: np.split(a.astype(np.float64), np.cumsum([x.shape[1] for x in like])[:-1], 1)
    dec = d.astype(np.float64)
    und = (dec != 0) & (np.abs(dec) < MARGIN * (np.abs(smax) + np.abs(tmax)).astype(np.float64))
    return dict(cls=float(cls), reg=float(reg), g_hm=split(g_cat, s_hm), g_reg=split(g_r, s_reg), left_out=und, decision=dec,
                arg=arg)
