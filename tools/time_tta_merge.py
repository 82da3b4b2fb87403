"""The flip test-time-augmentation merge at the workload's size: 6 tasks (1 2 2 1 2 2 classes), 180 x 180, V = 4 views,
B = 1 and 4, the heads being channel slices of the packed channels-last head output [V * B, 128, 180, 180] (42 heads padded
to 3 channels + 2).  ops.tta.flip_merge (csrc/tta_merge.hip: one launch) against the same arithmetic written with plain
PyTorch ops on the same device (flip, 1 - r, negation, sigmoid / exp, mean, logit / log per head), HIP events, the two paths
alternated in one process; the kernel alone is timed by the library's profiler scope "tta.merge".  GB/s is by algorithmic bytes: every merged channel read once per view and written once.
Prints one JSON line.  Run it under a time limit:  timeout -k 10 300 python tools/time_tta_merge.py"""
import os as _os; _os.environ.setdefault("UD_RANDOM_INIT", "1")
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
import torch
from unidistill_amd import _lib
from unidistill_amd.ops import tta

assert torch.cuda.is_available(), "time_tta_merge.py measures on the GPU only"
dev = torch.device("cuda:0")
NCS, H, W, KMAX, VIEWS = (1, 2, 2, 1, 2, 2), 180, 180, 3, tta.DOUBLE_FLIP
HEADS = (("iou", 1), ("reg", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2), ("hm", None))   # the packed head's order
V = len(VIEWS)


def make(B):
    g = torch.Generator().manual_seed(B)
    z = torch.randn(V * B, len(NCS) * len(HEADS) * KMAX + 2, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    preds, c0 = [], 0
    for nc in NCS:
        d = {}
        for name, c in HEADS:
            d[name] = z[:, c0:c0 + (c or nc)]
            c0 += KMAX
        preds.append(d)
    return z, preds


def torch_ops(preds, B):
    out = []
    for d in preds:
        res = {}
        for name, x in d.items():
            acc = 0
            for v, (fx, fy) in enumerate(VIEWS):
                t = x[v * B:(v + 1) * B]
                dims = [k for k, f in ((3, fx), (2, fy)) if f]
                if dims:
                    t = t.flip(dims)
                if name == "reg" and (fx or fy):
                    t = torch.stack([1 - t[:, 0] if fx else t[:, 0], 1 - t[:, 1] if fy else t[:, 1]], 1)
                elif name in ("rot", "vel") and (fx or fy):
                    sx, sy = (-1.0 if fx else 1.0), (-1.0 if fy else 1.0)
                    t = t * t.new_tensor([sy, sx] if name == "rot" else [sx, sy]).view(1, 2, 1, 1)
                elif name == "hm":
                    t = torch.sigmoid(t)
                elif name == "dim":
                    t = torch.exp(t)
                acc = acc + t
            acc = acc / V
            if name == "hm":
                acc = torch.log(acc) - torch.log1p(-acc)
            elif name == "dim":
                acc = torch.log(acc)
            res[name] = acc
        out.append(res)
    return out


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


out = {"tool": "time_tta_merge", "shape": {"tasks": len(NCS), "H": H, "W": W, "V": V, "packed_channels": len(NCS) * len(HEADS) * KMAX + 2}}
for B in (1, 4):
    z, preds = make(B)
    channels = sum(x.shape[1] for d in preds for x in d.values())
    nbytes = (V + 1) * B * channels * H * W * 4
    hip = lambda: tta.flip_merge(preds, VIEWS, no_log=False, nbox=9)
    ref = lambda: torch_ops(preds, B)
    for fn in (hip, ref):
        for _ in range(3):
            fn()
    a, b = hip(), ref()
    torch.cuda.synchronize()
    agree = max(float((x[k] - y[k]).abs().max()) for x, y in zip(a, b) for k in x)
    paths = [("hip", hip, 100), ("torch_ops", ref, 10)]
    results = {name: [] for name, _, _ in paths}
    for rep in range(5):                    # alternate the paths so that clock / neighbour drift hits both alike
        for name, fn, n in paths:
            results[name].append(timed(fn, n))
    # the kernel alone, by the library's own events around the launch (the call above includes the host's descriptor set-up)
    _lib.prof_enable(True)
    _lib.prof_read("tta.merge")
    for _ in range(50):
        hip()
    ms, calls = _lib.prof_read("tta.merge")
    _lib.prof_enable(False)
    kernel_us = ms * 1e3 / max(calls, 1)
    row = {"merged_channels": channels, "algorithmic_bytes": nbytes, "max_abs_diff_vs_torch_ops": agree,
           "hip_kernel": {"mean_us": round(kernel_us, 2), "calls": calls, "GBps": round(nbytes / kernel_us / 1e3, 1)}}
    for name, _, _ in paths:
        r = sorted(results[name])
        med = r[len(r) // 2]
        row[name] = {"median_us": round(med, 2), "min_us": round(r[0], 2), "max_us": round(r[-1], 2),
                     "GBps": round(nbytes / med / 1e3, 1)}
    out[f"B{B}"] = row
    del z, preds
print(json.dumps(out))
