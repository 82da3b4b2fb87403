"""The detection loss's default terms written out in PyTorch; a helper, not a test.

focal_ref and reg_ref restate what csrc/det_loss.hip computes by default (k_focal_*, k_reg_*<false>): the computation runs on the CPU
in the dtype of its inputs (float64 is the yardstick, float32 measures what single precision costs), is differentiable by autograd and
calls no project op.  tests/test_det_loss_reference_cpu.py ties it to CenterHeadIouAware._loss_terms_torch, which the reference golden
pins; tests/test_det_loss_reference_gpu.py holds the kernels against it.

reg_ref also returns the *decision margin* of every positive slot (the convention of rot_iou_reference): the smallest distance of any
quantity a branch decides on to that branch's threshold.  A slot with a small margin sits where a derivative is one-sided (or, at the
r = pi/4 switch of the nearest-BEV box, where the value itself jumps) and a float32 evaluation may take the other branch.  The distances:

    dim logit e (prediction and target)   |e - 80|, |min(e, 80) - log 1e-3|, |min(e, 80) - log 30|
    overlap of each axis                  |raw - 1e-3|, |A - B|, |C - D|          (metres)
    volume floor                          |log vraw - log 1e-3|
    clamp(iou, 0, 1)                      |1 - iou|, and |U| / (vp + vt) for the lower side
    nearest-BEV switch (both boxes)       |r - pi/4|                               (radians)
    L1 terms                              |g_j - tgt_j| (j < nb, target not NaN), |g_iou - tar|

exp(e) and vraw are products of positive factors held against a floor of 1e-3 (and a cap of 30): their float32 error is relative, and
below the floor no absolute distance can reach MARGIN, so they are measured as a log ratio (for exp(e): in the logit itself).  iou is
the ratio of inter > 0 (its factors are floored) and U = vp + vt - inter, so it is below 0 exactly when U is: the distance is U's, relative
to the terms it is the difference of.
"""
import math

import torch

from rot_iou_reference import MARGIN          # noqa: F401  (the threshold the tests use)

LOGIT_CLAMP = math.log(9999.0)                # where the clamped sigmoid's bounds 1e-4 and 1 - 1e-4 are reached


def focal_ref(logits_list, gt, alpha, gamma):
    """logits_list: T tensors [B, ncls_t, H, W]; gt [T, B, ncm, H, W] -> (prob [T,B,ncm,H,W], pos [T], neg [T]).
    Channels c >= ncls_t are padding: prob = 0 there and gt is not looked at."""
    T, ncm = len(logits_list), gt.shape[2]
    dt = logits_list[0].dtype
    gt = gt.to(dt)
    logits = torch.stack([torch.nn.functional.pad(x, (0, 0, 0, 0, 0, ncm - x.shape[1])) for x in logits_list])
    valid = (torch.arange(ncm)[None, :] < torch.tensor([x.shape[1] for x in logits_list])[:, None])[:, None, :, None, None]
    p = torch.clamp(torch.sigmoid(logits), min=1e-4, max=1 - 1e-4)           # 0.5 in the padding: every term below stays finite
    zero = torch.zeros((), dtype=dt)
    pos_t = torch.log(p) * torch.pow(1 - p, gamma) * alpha
    neg_t = torch.log(1 - p + 1e-4) * torch.pow(p, gamma) * (1 - alpha)
    pos = torch.where((gt == 1) & valid, pos_t, zero).sum(dim=(1, 2, 3, 4))
    neg = torch.where((gt == 0) & valid, neg_t, zero).sum(dim=(1, 2, 3, 4))
    return torch.where(valid, p, zero), pos, neg


def _decode_whl(e):
    """-> (clamp(exp(min(e, 80)), 1e-3, 30), margin of the three clamps, in the logit)."""
    ec = torch.clamp(e, max=80.0)
    whl = torch.clamp(torch.exp(ec), min=1e-3, max=30.0)
    ed = ec.detach().double()
    margin = torch.minimum(torch.minimum((e.detach().double() - 80.0).abs(), (ed - math.log(1e-3)).abs()), (ed - math.log(30.0)).abs())
    return whl, margin.amin(-1)


def _overlap(pc, pe, tc, te):
    A, B, C, D = pc + pe / 2, tc + te / 2, pc - pe / 2, tc - te / 2
    raw = torch.minimum(A, B) - torch.maximum(C, D)
    m = torch.minimum(torch.minimum((raw - 1e-3).abs(), (A - B).abs()), (C - D).abs())
    return torch.clamp(raw, min=1e-3), m.detach().double()


def _aligned_bev(x, y, w, l, rot):
    r = (rot - torch.floor(rot / math.pi + 0.5) * math.pi).abs()
    near = r < math.pi / 4
    dx, dy = torch.where(near, w, l), torch.where(near, l, w)
    return x - dx / 2, y - dy / 2, x + dx / 2, y + dy / 2, (r - math.pi / 4).abs().detach().double()


def reg_ref(g, tgt, mask, num_obj, sx, sy, nb):
    """g [T,B,K,11] gathered head values (reg2 height1 dim3 rot2 vel2 iou1; may require grad), tgt [T,B,K,>=nb], mask bool [T,B,K],
    num_obj [T] -> (box [T,nb], iou_loss [T], iou_aware [T], margin f64 [T,B,K], inf at masked-off slots; see the module docstring).
    CenterHeadIouAware._loss_terms_torch / _iou_losses term by term.  A NaN target entry makes its box-L1 column NaN and has derivative
    0 (the tensor-op formulation multiplies target and prediction by a 0 mask, which keeps the NaN in the value and passes no
    gradient).  That formulation reads the targets of masked-off slots too; the kernel does not, and the assigner zeroes them."""
    dt = g.dtype
    tgt, num_obj = tgt[..., :nb].to(dt), num_obj.to(dt)
    zero = torch.zeros((), dtype=dt)
    nan = torch.full((), math.nan, dtype=dt)
    den_box, den_iou = num_obj + 1e-4, torch.clamp(num_obj, min=1.0)
    # masked L1 per code dimension
    bad = torch.isnan(tgt)
    diff = g[..., :nb] - torch.nan_to_num(tgt)
    use = mask[..., None] & ~bad
    box = torch.where(use, diff, zero).abs().sum(dim=(1, 2)) / den_box[:, None]
    box = box + torch.where(bad.any(dim=(1, 2)), nan, zero)                   # target * 0 stays NaN and reaches the column's sum
    margin = torch.where(use, diff.detach().double().abs(), torch.full((), math.inf, dtype=torch.float64)).amin(-1)
    # decoded boxes: centres scaled to metres, extents through the clamped exp, yaw from (sin, cos)
    pw, m_pw = _decode_whl(g[..., 3:6])
    tw, m_tw = _decode_whl(tgt[..., 3:6])
    px, py, pz = g[..., 0] * sx, g[..., 1] * sy, g[..., 2]
    tx, ty, tz = tgt[..., 0] * sx, tgt[..., 1] * sy, tgt[..., 2]
    # axis-aligned "3-D IoU" with the reference's (x <-> whl0, y <-> whl2, z <-> whl1) pairing
    ox, m_x = _overlap(px, pw[..., 0], tx, tw[..., 0])
    oy, m_y = _overlap(py, pw[..., 2], ty, tw[..., 2])
    oz, m_z = _overlap(pz, pw[..., 1], tz, tw[..., 1])
    inter = ox * oy * oz
    vraw = pw[..., 0] * pw[..., 2] * pw[..., 1]
    vp = torch.clamp(vraw, min=1e-3)
    vt = torch.clamp(tw[..., 0] * tw[..., 2] * tw[..., 1], min=1e-3)
    U = vp + vt - inter
    iou = inter / U
    iou_loss = torch.where(mask, 1 - torch.clamp(iou, 0, 1), zero).sum(dim=(1, 2)) / den_iou
    m_v = (torch.log(vraw.detach().double()) - math.log(1e-3)).abs()
    m_iou = torch.minimum((1 - iou).abs(), U.abs() / (vp + vt)).detach().double()
    tar, m_r = bev_target(g, tgt, sx, sy)
    da = g[..., 10] - tar
    aware = torch.where(mask & ~torch.isnan(tar), da, zero).abs().sum(dim=(1, 2)) / den_box
    aware = aware + torch.where((mask & torch.isnan(tar)).any(dim=(1, 2)), nan, zero)
    for m in (m_pw, m_tw, m_x, m_y, m_z, m_v, m_iou, m_r, da.detach().double().abs()):
        margin = torch.minimum(margin, m)
    margin = torch.where(mask, margin, torch.full((), math.inf, dtype=torch.float64))
    return box, iou_loss, aware, margin


def bev_target(g, tgt, sx, sy):
    """The IoU-aware target 2 (IoU - 0.5): nearest-BEV IoU of the decoded target and the detached prediction (extents 0 and 1, whatever
    the loss paired) -> (tar [T,B,K] in g's dtype, min over both boxes of |r - pi/4| f64 [T,B,K]: the forward value jumps there)."""
    g, tgt = g.detach(), tgt.detach().to(g.dtype)
    pw, _ = _decode_whl(g[..., 3:6])
    tw, _ = _decode_whl(tgt[..., 3:6])
    a0x, a0y, a1x, a1y, m_ra = _aligned_bev(tgt[..., 0] * sx, tgt[..., 1] * sy, tw[..., 0], tw[..., 1], torch.atan2(tgt[..., 6], tgt[..., 7]))
    b0x, b0y, b1x, b1y, m_rb = _aligned_bev(g[..., 0] * sx, g[..., 1] * sy, pw[..., 0], pw[..., 1], torch.atan2(g[..., 6], g[..., 7]))
    iw = torch.clamp(torch.minimum(a1x, b1x) - torch.maximum(a0x, b0x), min=0)
    ih = torch.clamp(torch.minimum(a1y, b1y) - torch.maximum(a0y, b0y), min=0)
    ib = iw * ih
    area = (a1x - a0x) * (a1y - a0y) + (b1x - b0x) * (b1y - b0y) - ib
    return 2 * (ib / torch.clamp(area, min=1e-6) - 0.5), torch.minimum(m_ra, m_rb)
