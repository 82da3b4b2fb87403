"""Float64 restatement of the box-level fusion of DESIGN §2.22 (csrc/box_fusion.hip, ops/box_fusion.py), in numpy and plain
Python floats: un-view, validity, order, greedy same-label clusters, confidence-weighted fusion, output order.

``iou_bev64`` restates csrc/bev_iou.h's Sutherland-Hodgman clipping (rectangle A clipped by the four half-planes of
rectangle B, shoelace area, IoU = inter / max(area_a + area_b - inter, 1e-8)) in float64 on the fp32 box entries.
"""
import math

import numpy as np

PI = math.pi


def sincos(rot_deg):
    """ops.tta._sincos, restated: exact at multiples of 90 degrees."""
    q = rot_deg / 90.0
    if q == math.floor(q):
        return ((0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0))[int(q % 4)]
    a = rot_deg / 180 * np.pi
    return float(np.sin(a)), float(np.cos(a))


def general(views, S):
    if views is None:
        return [(0.0, 1.0, 0, 0)] * S
    return [(0.0, 1.0) + tuple(v) if len(v) == 2 else tuple(v) for v in views]


def _corners(b):
    cs, sn = math.cos(b[6]), math.sin(b[6])
    hx, hy = 0.5 * b[3], 0.5 * b[4]
    return [(b[0] + lx * cs - ly * sn, b[1] + lx * sn + ly * cs) for lx, ly in ((-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy))]


def _clipped_area(A, B):
    poly = list(A)
    for e in range(4):
        if not poly:
            break
        p, q = B[e], B[(e + 1) & 3]
        ex, ey = q[0] - p[0], q[1] - p[1]
        out = []
        n = len(poly)
        for k in range(n):
            s, t = poly[k], poly[(k + 1) % n]
            ds = ex * (s[1] - p[1]) - ey * (s[0] - p[0])
            dt = ex * (t[1] - p[1]) - ey * (t[0] - p[0])
            if ds >= 0.0:
                out.append(s)
            if (ds >= 0.0) != (dt >= 0.0):
                u = ds / (ds - dt)
                out.append((s[0] + u * (t[0] - s[0]), s[1] + u * (t[1] - s[1])))
        poly = out
    if len(poly) < 3:
        return 0.0
    a2 = 0.0
    for k in range(len(poly)):
        s, t = poly[k], poly[(k + 1) % len(poly)]
        a2 += s[0] * t[1] - t[0] * s[1]
    return 0.5 * abs(a2)


def iou_bev64(a, b):
    """Rotated-BEV IoU of two boxes (x, y, z, dx, dy, dz, yaw): bev_iou.h's clipping in float64."""
    a, b = [float(v) for v in a[:7]], [float(v) for v in b[:7]]
    # footprints whose centres are further apart than their half-diagonals together cannot meet: the clip gives exactly 0
    if math.hypot(a[0] - b[0], a[1] - b[1]) > 0.5 * (math.hypot(a[3], a[4]) + math.hypot(b[3], b[4])) * (1 + 1e-9) + 1e-9:
        return 0.0
    inter = _clipped_area(_corners(a), _corners(b))
    return inter / max(a[3] * a[4] + b[3] * b[4] - inter, 1e-8)


def unview(box, view):
    """One fp32 box of a view back in the original frame, float64 [9] (velocity 0 for a 7-entry box)."""
    rot_deg, scale, fdx, fdy = view
    sn, cs = sincos(float(rot_deg))
    rot = float(rot_deg) / 180 * PI
    fx, fy = (-1.0 if fdx else 1.0), (-1.0 if fdy else 1.0)
    v = [float(e) for e in box]
    x, y = fx * v[0], fy * v[1]
    u = [0.0] * 9
    u[0] = (cs * x + sn * y) / scale
    u[1] = (cs * y - sn * x) / scale
    for k in (2, 3, 4, 5):
        u[k] = v[k] / scale
    yaw = v[6]
    u[6] = (PI + yaw - rot if fdy else PI - yaw - rot) if fdx else (-yaw - rot if fdy else yaw - rot)
    if len(v) == 9:
        vx, vy = fx * v[7], fy * v[8]
        u[7] = (cs * vx + sn * vy) / scale
        u[8] = (cs * vy - sn * vx) / scale
    return u


def wrap_half_open(y):
    """into [-pi, pi)"""
    return y - 2.0 * PI * math.floor((y + PI) / (2.0 * PI))


def fuse_reference(rois, scores, labels, num, S, *, views=None, weights=None, iou_threshold, score_threshold=0.0,
                   max_out=500, dtype=np.float32):
    """``dtype``: the precision the inputs are read in: float32 as the kernel reads them; float64 for invariants of the
    algorithm itself.  -> list over the B samples of dicts: ``rows`` f64[n, box_dim], ``scores`` f64[n], ``scores32`` f32[n] (the order's
    key), ``labels``, ``anchor`` (s * R + r of each cluster's anchor), ``members``; and of the whole sample ``order`` (s * R + r
    of the valid boxes in sorted order), ``anchor_of`` (for each of them the sorted position of its anchor), ``clusters`` (the
    number before the cut at max_out) and ``margin`` (the smallest |IoU - iou_threshold| over its same-label valid pairs;
    inf without a pair)."""
    rois, scores = np.asarray(rois, dtype), np.asarray(scores, dtype)
    SB, R, D = rois.shape
    B = SB // S
    views = general(views, S)
    weights = [1.0] * S if weights is None else [float(w) for w in weights]
    w_all = 0.0
    for w in weights:
        w_all += w
    thr32 = float(np.float32(iou_threshold))
    out = []
    for b in range(B):
        items = []
        for s in range(S):
            row = s * B + b
            n = min(max(int(num[row]), 0), R)
            for r in range(n):
                sc, lab = scores[row, r], int(labels[row, r])
                if not (np.isfinite(rois[row, r]).all() and np.isfinite(sc) and sc > dtype(score_threshold)
                        and 0 <= lab <= 65535):
                    continue
                items.append((lab, -float(sc), s, r))
        items.sort()
        n = len(items)
        boxes64 = [unview(rois[s * B + b, r], views[s]) for _, _, s, r in items]
        boxes32 = [[float(x) for x in np.asarray(u[:7], np.float64).astype(np.float32)] for u in boxes64]
        conf = [weights[s] * float(scores[s * B + b, r]) for _, _, s, r in items]
        # all same-label pairs: the IoU matrix (earlier box first) and the margin
        iou = {}
        margin = math.inf
        start = 0
        while start < n:
            end = start
            while end < n and items[end][0] == items[start][0]:
                end += 1
            for i in range(start, end):
                for j in range(i + 1, end):
                    v = iou_bev64(boxes32[i], boxes32[j])
                    margin = min(margin, abs(v - thr32))
                    if v > thr32:
                        iou[(i, j)] = v
            start = end
        anchor_of = [-1] * n
        for i in range(n):
            if anchor_of[i] >= 0:
                continue
            anchor_of[i] = i
            for j in range(i + 1, n):
                if items[j][0] != items[i][0]:
                    break
                if anchor_of[j] < 0 and (i, j) in iou:
                    anchor_of[j] = i
        clusters = []
        for a in range(n):
            if anchor_of[a] != a:
                continue
            members = [j for j in range(a, n) if anchor_of[j] == a]
            csum, wsum, dsum = 0.0, 0.0, 0.0
            acc = [0.0] * 9
            for m, j in enumerate(members):
                c = conf[j]
                if m == 0:
                    csum, wsum = c, weights[items[j][2]]
                    acc = [c * v for v in boxes64[j]]
                    continue
                csum += c
                wsum += weights[items[j][2]]
                acc = [x + c * v for x, v in zip(acc, boxes64[j])]
                d = boxes64[j][6] - boxes64[a][6]
                d -= 2.0 * PI * math.ceil((d - PI) / (2.0 * PI))
                if d > 0.5 * PI:
                    d -= PI
                elif d < -0.5 * PI:
                    d += PI
                dsum += c * d
            row = [x / csum for x in acc]
            row[6] = wrap_half_open(boxes64[a][6] + dsum / csum)
            score = csum / max(wsum, w_all)
            clusters.append((-float(np.float32(score)), a, row[:D], score, len(members)))
        clusters.sort(key=lambda c: (c[0], c[1]))
        kept = clusters[:max_out]
        out.append({
            "rows": np.array([c[2] for c in kept], np.float64).reshape(len(kept), D),
            "scores": np.array([c[3] for c in kept], np.float64),
            "scores32": np.array([-c[0] for c in kept], np.float32),
            "labels": np.array([items[c[1]][0] for c in kept], np.int64),
            "anchor": np.array([items[c[1]][2] * R + items[c[1]][3] for c in kept], np.int64),
            "members": np.array([c[4] for c in kept], np.int64),
            "order": [s * R + r for _, _, s, r in items],
            "anchor_of": anchor_of,
            "clusters": len(clusters),
            "margin": margin,
        })
    return out


def make_views(rois, view):
    """The fp32 boxes [n, box_dim] of the original frame as a view sees them: A_v = F S R applied in float64 and rounded."""
    rot_deg, scale, fdx, fdy = view
    sn, cs = sincos(float(rot_deg))
    rot = float(rot_deg) / 180 * PI
    fx, fy = (-1.0 if fdx else 1.0), (-1.0 if fdy else 1.0)
    b = np.asarray(rois, np.float64)
    o = b.copy()
    o[:, 0] = fx * scale * (cs * b[:, 0] - sn * b[:, 1])
    o[:, 1] = fy * scale * (sn * b[:, 0] + cs * b[:, 1])
    o[:, 2:6] = b[:, 2:6] * scale
    yaw = b[:, 6] + rot
    o[:, 6] = (PI + yaw if fdy else PI - yaw) if fdx else (-yaw if fdy else yaw)
    if b.shape[1] == 9:
        o[:, 7] = fx * scale * (cs * b[:, 7] - sn * b[:, 8])
        o[:, 8] = fy * scale * (sn * b[:, 7] + cs * b[:, 8])
    return o
