"""Box-level fusion at the workload's size: B = 4 samples, S = 8 views (rotations 0 and 7.5 degrees x the four flips), 600 rows
per source (6 tasks x post-NMS 100), 10 labels, box_dim 9.  ops.box_fusion.fuse_padded (csrc/box_fusion.hip: three launches, no
host synchronisation) against the same algorithm composed of PyTorch ops: the un-view with tensor ops in float64, a sort per
sample, ops.nms.boxes_iou_bev_gpu for the full IoU matrix of a sample, a greedy loop that reads the matrix on the host, and the
weighted sums by index_add.  HIP events around whole calls (the composition's host loop and copies included: that is what it
costs), the two paths alternated in one process; the kernels alone by the library's profiler scope "box_fusion".
Prints one JSON line.  Run it under a time limit:  timeout -k 10 300 python tools/time_box_fusion.py"""
import os as _os; _os.environ.setdefault("UD_RANDOM_INIT", "1")
import json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
import numpy as np
import torch
from unidistill_amd import _lib
from unidistill_amd.ops import box_fusion, nms, tta

assert torch.cuda.is_available(), "time_box_fusion.py measures on the GPU only"
dev = torch.device("cuda:0")
B, S, R, LABELS, D, THR, MAX_OUT = 4, 8, 600, 10, 9, 0.2, 500
VIEWS = tta.views(rotations=(0.0, 7.5), flips="double")
assert len(VIEWS) == S


def make():
    """Per sample 450 objects on a 4 m lattice; every source sees nine in ten of them, jittered, and fills up with distractors."""
    rng = np.random.default_rng(0)
    rois = np.zeros((S * B, R, D), np.float32)
    scores = np.zeros((S * B, R), np.float32)
    labels = np.zeros((S * B, R), np.int64)
    num = np.zeros(S * B, np.int32)
    for b in range(B):
        n = 450
        cell = rng.permutation(26 * 26)[:n]
        obj = np.zeros((n, D))
        obj[:, 0] = (cell % 26) * 4.0 - 50 + rng.uniform(-0.3, 0.3, n)
        obj[:, 1] = (cell // 26) * 4.0 - 50 + rng.uniform(-0.3, 0.3, n)
        obj[:, 2] = rng.uniform(-2, 1, n)
        obj[:, 3:6] = rng.uniform(0.6, 3.0, (n, 3))
        obj[:, 6] = rng.uniform(-3.1, 3.1, n)
        obj[:, 7:9] = rng.uniform(-5, 5, (n, 2))
        lab, sc = rng.integers(1, LABELS + 1, n), rng.uniform(0.12, 0.9, n)
        for s, (rot, scale, fx, fy) in enumerate(VIEWS):
            keep = rng.random(n) < 0.9
            o = obj[keep].copy()
            o[:, 0:2] += rng.uniform(-0.1, 0.1, (len(o), 2))
            o[:, 3:6] *= rng.uniform(0.97, 1.03, (len(o), 3))
            o[:, 6] += rng.uniform(-0.03, 0.03, len(o))
            extra = R - len(o) - int(rng.integers(0, 40))
            d = np.zeros((max(extra, 0), D))
            d[:, 0:2] = rng.uniform(-52, 52, (len(d), 2))
            d[:, 3:6] = rng.uniform(0.5, 2.0, (len(d), 3))
            d[:, 6] = rng.uniform(-3.1, 3.1, len(d))
            o = np.concatenate([o, d])
            a, c, sn = rot / 180 * math.pi, *tta._sincos(rot)[::-1]
            x, y = o[:, 0].copy(), o[:, 1].copy()
            o[:, 0], o[:, 1] = (-1 if fx else 1) * scale * (c * x - sn * y), (-1 if fy else 1) * scale * (sn * x + c * y)
            o[:, 2:6] *= scale
            yaw = o[:, 6] + a
            o[:, 6] = (math.pi + yaw if fy else math.pi - yaw) if fx else (-yaw if fy else yaw)
            vx, vy = o[:, 7].copy(), o[:, 8].copy()
            o[:, 7], o[:, 8] = (-1 if fx else 1) * scale * (c * vx - sn * vy), (-1 if fy else 1) * scale * (sn * vx + c * vy)
            k = len(o)
            row = s * B + b
            rois[row, :k] = o
            scores[row, :k] = np.concatenate([sc[keep] * rng.uniform(0.9, 1.1, int(keep.sum())), rng.uniform(0.1, 0.3, len(d))])
            labels[row, :k] = np.concatenate([lab[keep], rng.integers(1, LABELS + 1, len(d))])
            num[row] = k
    return [torch.from_numpy(a).to(dev) for a in (rois, scores, labels, num)]


def torch_ops(rois, scores, labels, num):
    """The same algorithm from PyTorch ops (unit weights): -> fused counts per sample."""
    counts = num.tolist()
    outs = []
    for b in range(B):
        parts, sc, lb = [], [], []
        for s, (rot, scale, fx, fy) in enumerate(VIEWS):
            n = counts[s * B + b]
            p = rois[s * B + b, :n].double()
            sn, c = tta._sincos(rot)
            x, y = (-p[:, 0] if fx else p[:, 0]), (-p[:, 1] if fy else p[:, 1])
            vx, vy = (-p[:, 7] if fx else p[:, 7]), (-p[:, 8] if fy else p[:, 8])
            a = rot / 180 * math.pi
            yaw = p[:, 6]
            yaw = ((math.pi + yaw - a) if fy else (math.pi - yaw - a)) if fx else ((-yaw - a) if fy else (yaw - a))
            parts.append(torch.stack([(c * x + sn * y) / scale, (c * y - sn * x) / scale, p[:, 2] / scale, p[:, 3] / scale,
                                      p[:, 4] / scale, p[:, 5] / scale, yaw, (c * vx + sn * vy) / scale,
                                      (c * vy - sn * vx) / scale], 1))
            sc.append(scores[s * B + b, :n])
            lb.append(labels[s * B + b, :n])
        box, sc, lb = torch.cat(parts), torch.cat(sc), torch.cat(lb)
        order = torch.argsort(-sc, stable=True)
        order = order[torch.argsort(lb[order], stable=True)]
        box, sc, lb = box[order], sc[order].double(), lb[order]
        iou = nms.boxes_iou_bev_gpu(box.float(), box.float()).cpu().numpy()            # the host reads the matrix
        lab = lb.cpu().numpy()
        n = len(lab)
        anchor = np.full(n, -1, np.int64)
        idx = np.arange(n)
        for i in range(n):
            if anchor[i] >= 0:
                continue
            anchor[i] = i
            take = (iou[i] > THR) & (lab == lab[i]) & (anchor < 0) & (idx > i)
            anchor[take] = i
        anc = torch.from_numpy(anchor).to(dev)
        d = box[:, 6] - box[anc, 6]
        d = d - 2 * math.pi * torch.ceil((d - math.pi) / (2 * math.pi))
        d = torch.where(d > math.pi / 2, d - math.pi, torch.where(d < -math.pi / 2, d + math.pi, d))
        vals = torch.cat([box, d[:, None], torch.ones_like(d)[:, None]], 1) * sc[:, None]
        acc = torch.zeros((n, D + 2), dtype=torch.float64, device=dev).index_add_(0, anc, vals)
        members = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, anc, torch.ones_like(d))
        is_anchor = anc == torch.arange(n, device=dev)
        csum = acc[is_anchor, D + 1]
        fused = acc[is_anchor, :D] / csum[:, None]
        yaw = box[is_anchor, 6] + acc[is_anchor, D] / csum
        fused[:, 6] = yaw - 2 * math.pi * torch.floor((yaw + math.pi) / (2 * math.pi))
        score = (csum / torch.clamp_min(members[is_anchor], float(S))).float()
        top = torch.argsort(-score, stable=True)[:MAX_OUT]
        outs.append((fused[top].float(), score[top], lb[is_anchor][top]))
    return outs


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


args = make()
hip = lambda: box_fusion.fuse_padded(*args, S, views=VIEWS, iou_threshold=THR, max_out=MAX_OUT)
ref = lambda: torch_ops(*args)
for fn, n in ((hip, 3), (ref, 1)):
    for _ in range(n):
        fn()
a, b = hip(), ref()
counts = box_fusion.read_num(a[3])
same_counts = counts == [len(o[1]) for o in b]
score_diff = max(float((a[1][i, :counts[i]] - b[i][1]).abs().max()) for i in range(B)) if same_counts else None
paths = [("hip", hip, 20), ("torch_ops", ref, 1)]
results = {name: [] for name, _, _ in paths}
for rep in range(5):                        # alternate the paths so that clock / neighbour drift hits both alike
    for name, fn, n in paths:
        results[name].append(timed(fn, n))
_lib.prof_enable(True)
_lib.prof_read("box_fusion")
for _ in range(20):
    hip()
ms, calls = _lib.prof_read("box_fusion")
_lib.prof_enable(False)
out = {"tool": "time_box_fusion",
       "shape": {"B": B, "S": S, "R": R, "labels": LABELS, "box_dim": D, "valid_boxes_per_sample": int(sum(args[3].tolist()) / B),
                 "max_out": MAX_OUT},
       "fused_counts": counts, "same_counts_as_torch_ops": same_counts, "max_abs_score_diff_vs_torch_ops": score_diff,
       "launches": 3, "hip_kernels": {"mean_us": round(ms * 1e3 / max(calls, 1), 2), "calls": calls}}
for name, _, _ in paths:
    r = sorted(results[name])
    out[name] = {"median_us": round(r[len(r) // 2], 2), "min_us": round(r[0], 2), "max_us": round(r[-1], 2)}
print(json.dumps(out))
