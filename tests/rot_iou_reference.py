"""Rotated 3-D IoU written out from its definition in PyTorch; a helper, not a test.

Boxes are (x, y, z, dx, dy, dz, yaw).  The computation runs in the dtype of its inputs (float64 is the yardstick, float32 measures what
single precision costs), is differentiable by autograd in the first box, and walks a Python loop over the pairs:

    inter_bev = area of the intersection of the two rotated rectangles: rectangle a clipped by the four edges of rectangle b
                (Sutherland-Hodgman), shoelace formula
    oz        = max(min(z_a + dz_a/2, z_b + dz_b/2) - max(z_a - dz_a/2, z_b - dz_b/2), 0)
    IoU       = inter_bev oz / max(dx_a dy_a dz_a + dx_b dy_b dz_b - inter_bev oz, 1e-8)

Coordinates are taken relative to the centre of b (the IoU does not depend on the origin).  Beside the IoU every function returns the
*decision margin* of each pair: the smallest |signed distance| (metres, or the unit of the compared quantity) over every inside/outside
test of the clip, the three z-overlap comparisons and the clamps it passed.  A pair with a small margin sits next to a point where the
derivative is one-sided and a float32 evaluation may take the other branch.

Also here: the composition with the head decode of the detection loss (reg_terms_ref) and the random draws the tests share.
"""
import math

import torch

MARGIN = 1e-3        # pairs closer than this to a decision are left out of derivative comparisons


def _f(t):
    return float(t.detach())


def _corners(x, y, dx, dy, yaw):
    c, s = torch.cos(yaw), torch.sin(yaw)
    out = []
    for lx, ly in ((-dx / 2, -dy / 2), (dx / 2, -dy / 2), (dx / 2, dy / 2), (-dx / 2, dy / 2)):     # counter-clockwise
        out.append((x + lx * c - ly * s, y + lx * s + ly * c))
    return out


def _inter_bev(a, b):
    """a, b: 7 zero-dim tensors each -> (area, margin)."""
    poly = _corners(a[0] - b[0], a[1] - b[1], a[3], a[4], a[6])
    clip = _corners(torch.zeros_like(b[0]), torch.zeros_like(b[1]), b[3], b[4], b[6])
    margin = math.inf
    for e in range(4):
        p, q = clip[e], clip[(e + 1) % 4]
        ex, ey = q[0] - p[0], q[1] - p[1]
        ln = torch.sqrt(ex * ex + ey * ey)
        dist = [(ex * (v[1] - p[1]) - ey * (v[0] - p[0])) / ln for v in poly]      # >= 0: inside (left of the edge)
        new = []
        for k in range(len(poly)):
            s, t = poly[k], poly[(k + 1) % len(poly)]
            ds, dt = dist[k], dist[(k + 1) % len(poly)]
            margin = min(margin, abs(_f(ds)))
            ins, int_ = bool(ds >= 0), bool(dt >= 0)
            if ins:
                new.append(s)
            if ins != int_:
                u = ds / (ds - dt)
                new.append((s[0] + u * (t[0] - s[0]), s[1] + u * (t[1] - s[1])))
        poly = new
        if not poly:
            break
    if len(poly) < 3:
        return a[0] * 0, margin
    a2 = 0
    for k in range(len(poly)):
        s, t = poly[k], poly[(k + 1) % len(poly)]
        a2 = a2 + (s[0] * t[1] - t[0] * s[1])
    return 0.5 * torch.abs(a2), margin


def iou3d_one(a, b):
    """a, b: sequences of 7 zero-dim tensors -> (IoU3D_rot, decision margin)."""
    ib, margin = _inter_bev(a, b)
    hi_a, hi_b, lo_a, lo_b = a[2] + a[5] / 2, b[2] + b[5] / 2, a[2] - a[5] / 2, b[2] - b[5] / 2
    raw = torch.minimum(hi_a, hi_b) - torch.maximum(lo_a, lo_b)
    oz = torch.clamp(raw, min=0)
    inter = ib * oz
    union = a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - inter
    iou = inter / torch.clamp(union, min=1e-8)
    margin = min(margin, abs(_f(hi_a - hi_b)), abs(_f(lo_a - lo_b)), abs(_f(raw)), abs(_f(union) - 1e-8))
    return iou, margin


def iou3d_pairs(a, b):
    """a [N,7] (may require grad), b [N,7] -> (iou [N], margin f64 [N])."""
    ious, margins = [], []
    for i in range(a.shape[0]):
        iou, m = iou3d_one(a[i].unbind(0), b[i].unbind(0))
        ious.append(iou)
        margins.append(m)
    return torch.stack(ious), torch.tensor(margins, dtype=torch.float64)


def iou3d_and_grad(a, b, dtype):
    """-> (iou [N], d iou / d a [N,7], margin [N]) evaluated in ``dtype``, returned as float64."""
    x = a.detach().to(dtype).clone().requires_grad_(True)
    iou, margin = iou3d_pairs(x, b.detach().to(dtype))
    grad, = torch.autograd.grad(iou.sum(), x)
    return iou.detach().double(), grad.double(), margin


# ---- the detection loss's terms in rotated mode ------------------------------------------------------------------------------
def decode(e, sx, sy):
    """e [..., >= 8] head or target code (x/sx, y/sy, z, log dx, log dy, log dz, sin, cos) -> (boxes [..., 7], margin [...])."""
    ex = torch.exp(torch.clamp(e[..., 3:6], max=80.0))
    whl = torch.clamp(ex, min=1e-3, max=30.0)
    box = torch.cat([e[..., 0:1] * sx, e[..., 1:2] * sy, e[..., 2:3], whl, torch.atan2(e[..., 6:7], e[..., 7:8])], -1)
    margin = torch.minimum((ex - 1e-3).abs(), (ex - 30.0).abs()).amin(-1).detach().double()
    return box, margin


def reg_terms_ref(g, tgt, mask, num_obj, sx, sy, nb):
    """g [T,B,K,11] gathered head values (may require grad), tgt [T,B,K,>=nb], mask bool [T,B,K], num_obj [T]
    -> (box_loss [T,nb], iou_loss [T], iou_aware [T], margin f64 [T,B,K] (inf at masked slots)).
    The L1 terms treat a NaN target entry as masked with zero derivative (the kernels' derivative there)."""
    T, B, K = mask.shape
    dt = g.dtype
    tgt, num_obj = tgt.to(dt), num_obj.to(dt)
    pbox, pm = decode(g, sx, sy)
    tbox, tm = decode(tgt, sx, sy)
    margin = torch.full((T, B, K), math.inf, dtype=torch.float64)
    zero = torch.zeros((), dtype=dt)
    iou_loss, aware, box = [], [], []
    for t in range(T):
        li, la = zero, zero
        for b in range(B):
            for k in range(K):
                if not bool(mask[t, b, k]):
                    continue
                iou, m = iou3d_one(pbox[t, b, k].unbind(0), tbox[t, b, k].unbind(0))
                margin[t, b, k] = min(m, float(pm[t, b, k]), float(tm[t, b, k]))
                li = li + (1 - torch.clamp(iou, 0, 1))
                tar = 2 * (iou.detach() - 0.5)
                margin[t, b, k] = min(float(margin[t, b, k]), abs(_f(g[t, b, k, 10] - tar)))
                la = la + torch.abs(g[t, b, k, 10] - tar)
        iou_loss.append(li / torch.clamp(num_obj[t], min=1.0))
        aware.append(la / (num_obj[t] + 1e-4))
        mj = mask[t, :, :, None] & ~torch.isnan(tgt[t, :, :, :nb])
        d = torch.where(mj, g[t, :, :, :nb] - torch.nan_to_num(tgt[t, :, :, :nb]), torch.zeros_like(g[t, :, :, :nb]))
        box.append(d.abs().sum(dim=(0, 1)) / (num_obj[t] + 1e-4))
    return torch.stack(box), torch.stack(iou_loss), torch.stack(aware), margin


# ---- the random draws the tests share ------------------------------------------------------------------------------------------
def random_pairs(n, seed=0):
    """-> (pred f64 [n,7], target f64 [n,7]): target extents U(0.3, 12) m, prediction = target moved by N(0, 0.3 extent), extents
    scaled by exp N(0, 0.2), turned by N(0, 0.4); every tenth pair is two independent boxes a few metres apart."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)
    nrm = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    dims = 0.3 + 11.7 * u(n, 3)
    ctr = torch.cat([u(n, 2) * 100 - 50, u(n, 1) * 6 - 3], 1)
    yaw = (u(n, 1) * 2 - 1) * math.pi
    tgt = torch.cat([ctr, dims, yaw], 1)
    pred = torch.cat([ctr + nrm(n, 3) * 0.3 * dims, dims * torch.exp(nrm(n, 3) * 0.2), yaw + nrm(n, 1) * 0.4], 1)
    free = torch.cat([ctr + (u(n, 3) * 2 - 1) * torch.tensor([6.0, 6.0, 2.0], dtype=torch.float64), 0.3 + 11.7 * u(n, 3),
                      (u(n, 1) * 2 - 1) * math.pi], 1)
    every_tenth = (torch.arange(n) % 10 == 9)[:, None]
    return torch.where(every_tenth, free, pred), tgt


def encode(box, sx, sy, rscale=None):
    """boxes [..., 7] -> codes [..., 8] (x/sx, y/sy, z, log extents, r sin, r cos)."""
    r = 1.0 if rscale is None else rscale
    return torch.cat([box[..., 0:1] / sx, box[..., 1:2] / sy, box[..., 2:3], torch.log(box[..., 3:6]),
                      r * torch.sin(box[..., 6:7]), r * torch.cos(box[..., 6:7])], -1)


def random_codes(n, sx, sy, seed=0):
    """The same draw in head space, centres within a few cells of the anchor: -> (pred code f64 [n,8], target code f64 [n,8]);
    the prediction's (sin, cos) pair is scaled by U(0.5, 2), so it is not unit-norm."""
    pred, tgt = random_pairs(n, seed)
    ctr = tgt[:, :3].clone()
    ctr[:, :2] *= 0.02                                 # +-1 m: offsets from the anchor point, not map coordinates
    pred = torch.cat([pred[:, :3] - tgt[:, :3] + ctr, pred[:, 3:]], 1)
    tgt = torch.cat([ctr, tgt[:, 3:]], 1)
    g = torch.Generator().manual_seed(seed + 1000)
    r = 0.5 + 1.5 * torch.rand(n, 1, generator=g, dtype=torch.float64)
    return encode(pred, sx, sy, r), encode(tgt, sx, sy)
