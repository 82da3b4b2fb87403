"""The rotation / scale / flip test-time-augmentation merge at the workload's size: 6 tasks (1 2 2 1 2 2 classes), 180 x 180,
B = 1, V = 12 views (rotations 0, +-7.5 degrees x the four flips), the heads being channel slices of the packed channels-last
head output [V * B, 128, 180, 180].  ops.tta.affine_merge (csrc/tta_merge_affine.hip: one launch) against the same arithmetic
composed of PyTorch ops on the same device: per view one grid_sample (bilinear, zeros outside) of the whole packed map after
the per-head elementwise part that has to come before the blend (sigmoid / exp), a grid_sample of ones for the coverage, the
value rules per head, the masked sum over the views, the division by the count and logit / log.  HIP events, the two paths
alternated in one process; the kernel alone is timed by the library's profiler scope "tta.merge_affine".  GB/s is by
algorithmic bytes, as for tools/time_tta_merge.py: every merged channel read once per view and written once (the kernel reads
up to four neighbours per view, most of them from the cache).
Prints one JSON line.  Run it under a time limit:  timeout -k 10 300 python tools/time_tta_affine.py"""
import os as _os; _os.environ.setdefault("UD_RANDOM_INIT", "1")
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
import torch
import torch.nn.functional as F
from unidistill_amd import _lib
from unidistill_amd.ops import tta

assert torch.cuda.is_available(), "time_tta_affine.py measures on the GPU only"
dev = torch.device("cuda:0")
NCS, H, W, KMAX, B = (1, 2, 2, 1, 2, 2), 180, 180, 3, 1
PC_RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
VIEWS = tta.views(rotations=(0.0, 7.5, -7.5), flips="double")
HEADS = (("iou", 1), ("reg", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2), ("hm", None))   # the packed head's order
V = len(VIEWS)
PARAMS, RATIO = tta.affine_params(VIEWS, PC_RANGE, H, W)
ROWS = PARAMS.tolist()                               # plain floats for the PyTorch composition


def make():
    g = torch.Generator().manual_seed(B)
    z = torch.randn(V * B, len(NCS) * len(HEADS) * KMAX + 2, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    slices, c0 = [], 0
    for nc in NCS:
        d = {}
        for name, c in HEADS:
            d[name] = (c0, c0 + (c or nc))
            c0 += KMAX
        slices.append(d)
    return z, slices, [{k: z[:, a:b] for k, (a, b) in d.items()} for d in slices]


def geometry():
    """Per view: the normalised sampling grid [1, H, W, 2] of grid_sample (align_corners=False), g = q - 1/2 and p as [H, W]."""
    py, px = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    out = []
    for row in ROWS:
        t = row[:6]
        qx = t[0] * (px + 0.5) + t[1] * (py + 0.5) + t[2]
        qy = t[3] * (px + 0.5) + t[4] * (py + 0.5) + t[5]
        grid = torch.stack([qx / W * 2 - 1, qy / H * 2 - 1], -1)[None].float().to(dev)
        out.append((grid, (qx - 0.5).float().to(dev), (qy - 0.5).float().to(dev), px.float().to(dev), py.float().to(dev)))
    return out


GEO = geometry()
ONES = torch.ones(1, 1, H, W, device=dev)


def torch_ops(z, slices):
    pre = z.clone()                                   # what is blended: probabilities and sizes, not logits and logs
    for d in slices:
        a, b = d["hm"]
        pre[:, a:b] = torch.sigmoid(z[:, a:b])
        a, b = d["dim"]
        pre[:, a:b] = torch.exp(z[:, a:b])
    acc = [{k: 0 for k in d} for d in slices]
    count = 0
    for v, (row, (grid, gx, gy, px, py)) in enumerate(zip(ROWS, GEO)):
        s = F.grid_sample(pre[v * B:(v + 1) * B], grid.expand(B, -1, -1, -1), mode="bilinear", padding_mode="zeros", align_corners=False)
        cover = (F.grid_sample(ONES, grid, mode="bilinear", padding_mode="zeros", align_corners=False) > 1 - 1e-6).float()
        count = count + cover
        ti, sc = row[6:10], row[10]
        li = [ti[0], ti[1] * RATIO, ti[2] / RATIO, ti[3]]
        for d, res in zip(slices, acc):
            for name, (a, b) in d.items():
                t = s[:, a:b]
                if name == "reg":
                    cx, cy = gx + t[:, 0] - row[2], gy + t[:, 1] - row[5]
                    t = torch.stack([ti[0] * cx + ti[1] * cy - px, ti[2] * cx + ti[3] * cy - py], 1)
                elif name in ("height", "dim"):
                    t = t / sc
                elif name == "vel":
                    t = torch.stack([li[0] * t[:, 0] + li[1] * t[:, 1], li[2] * t[:, 0] + li[3] * t[:, 1]], 1)
                elif name == "rot":
                    cs, sn = t[:, 1], t[:, 0]
                    t = torch.stack([sc * (li[2] * cs + li[3] * sn), sc * (li[0] * cs + li[1] * sn)], 1)
                res[name] = res[name] + t * cover
    out = []
    for res in acc:
        o = {}
        for name, t in res.items():
            t = t / count
            if name == "hm":
                t = torch.log(t) - torch.log1p(-t)
            elif name == "dim":
                t = torch.log(t)
            o[name] = t
        out.append(o)
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


z, slices, preds = make()
channels = sum(x.shape[1] for d in preds for x in d.values())
nbytes = (V + 1) * B * channels * H * W * 4
hip = lambda: tta.affine_merge_table(preds, PARAMS, RATIO, no_log=False, nbox=9)
ref = lambda: torch_ops(z, slices)
for fn in (hip, ref):
    for _ in range(3):
        fn()
a, b = hip(), ref()
torch.cuda.synchronize()
# away from the rim of a view's coverage, where the composition's threshold on a sampled mask of ones stands in for the rule
diff = torch.stack([(x[k] - y[k]).abs().amax(dim=(0, 1)) for x, y in zip(a, b) for k in x]).amax(0)
agree = float(diff.flatten().kthvalue(int(0.99 * H * W)).values)
paths = [("hip", hip, 50), ("torch_ops", ref, 5)]
results = {name: [] for name, _, _ in paths}
for rep in range(5):                        # alternate the paths so that clock / neighbour drift hits both alike
    for name, fn, n in paths:
        results[name].append(timed(fn, n))
# the kernel alone, by the library's own events around the launch (the call above includes the host's descriptor set-up)
_lib.prof_enable(True)
_lib.prof_read("tta.merge_affine")
for _ in range(50):
    hip()
ms, calls = _lib.prof_read("tta.merge_affine")
_lib.prof_enable(False)
kernel_us = ms * 1e3 / max(calls, 1)
out = {"tool": "time_tta_affine",
       "shape": {"tasks": len(NCS), "B": B, "H": H, "W": W, "V": V, "packed_channels": z.shape[1], "merged_channels": channels},
       "algorithmic_bytes": nbytes, "p99_pixel_max_abs_diff_vs_torch_ops": agree,
       "hip_kernel": {"mean_us": round(kernel_us, 2), "calls": calls, "GBps": round(nbytes / kernel_us / 1e3, 1)}}
for name, _, _ in paths:
    r = sorted(results[name])
    med = r[len(r) // 2]
    out[name] = {"median_us": round(med, 2), "min_us": round(r[0], 2), "max_us": round(r[-1], 2), "GBps": round(nbytes / med / 1e3, 1)}
print(json.dumps(out))
