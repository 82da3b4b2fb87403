"""The depth metric at the workload's size: B = 4, 6 cameras, D = 112 depth bins, 16 x 44 feature cells, the logits being the
first 112 channels of the depth net's channels-last [24, 192, 16, 44] output (and once more as NCHW).
ops.depth_metric (csrc/depth_metric.hip: 2 launches, nothing materialised) against the same sums written with plain PyTorch
ops on the same device (softmax, expectation, masks, sums into a float64 state), HIP events, the paths alternated in one
process.  Prints one JSON line.  Run it under a time limit:  timeout -k 10 300 python tools/time_depth_metric.py"""
import os as _os; _os.environ.setdefault("UD_RANDOM_INIT", "1")
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
import torch
from unidistill_amd.ops import depth_metric

assert torch.cuda.is_available(), "time_depth_metric.py measures on the GPU only"
dev = torch.device("cuda:0")
B, NCAM, D, C, FH, FW, D_BOUND = 4, 6, 112, 80, 16, 44, [2.0, 58.0, 0.5]
EDGES = [2.0, 20.0, 40.0, 58.0]
g = torch.Generator().manual_seed(0)
feat = (torch.randn(B * NCAM, D + C, FH, FW, generator=g) * 2).to(dev).contiguous(memory_format=torch.channels_last)
nchw = feat[:, :D].contiguous()
dmin = 2.0 + torch.rand(B * NCAM, FH, FW, generator=g) * 55.9
dmin[torch.rand(B * NCAM, FH, FW, generator=g) < 0.5] = float("inf")
dmin = dmin.to(dev)
state = torch.zeros(NCAM, len(EDGES) - 1, 12, dtype=torch.float64, device=dev)
tstate = torch.zeros_like(state)
centre = (2.0 + (torch.arange(D, device=dev, dtype=torch.float64) + 0.5) * 0.5).float().view(1, D, 1, 1)
edges_t = torch.tensor(EDGES, device=dev)


def hip_cl():
    return depth_metric.depth_metric_accumulate(feat[:, :D], dmin, state, D_BOUND, EDGES, NCAM)


def hip_nchw():
    return depth_metric.depth_metric_accumulate(nchw, dmin, state, D_BOUND, EDGES, NCAM)


def torch_ops(x=None):
    """The same twelve sums per (camera, range) with library ops: fp32 per pixel, the sums in float64."""
    x = feat[:, :D] if x is None else x
    k = torch.floor((dmin - 2.0) / 0.5)
    lab = torch.isfinite(dmin) & (k >= 0) & (k < D)
    b = torch.where(lab, k, torch.zeros_like(k)).long()
    d = torch.where(lab, dmin, torch.ones_like(dmin))
    p = torch.softmax(x, 1)
    dhat = (p * centre).sum(1)
    ahat = x.argmax(1)
    pb = p.gather(1, b[:, None])[:, 0]
    e = dhat - d
    q = torch.maximum(dhat / d, d / dhat)
    lg = torch.log(dhat) - torch.log(d)
    terms = torch.stack([torch.ones_like(e), e.abs(), e.abs() / d, e * e / d, e * e, lg * lg, (q < 1.25).float(),
                         (q < 1.25 ** 2).float(), (q < 1.25 ** 3).float(), (ahat == b).float(), ((ahat - b).abs() <= 1).float(),
                         -torch.log(pb.clamp(min=1e-44))], -1).double()                                  # [BN, fH, fW, 12]
    r = torch.bucketize(d, edges_t, right=True) - 1                                                      # edges[r] <= d < edges[r + 1]
    onehot = (lab & (r >= 0) & (r < len(EDGES) - 1))[..., None] & (r[..., None] == torch.arange(len(EDGES) - 1, device=dev))
    sums = torch.einsum("nhwr,nhwt->nrt", onehot.double(), terms)                                        # [BN, R, 12]
    tstate.add_(sums.view(B, NCAM, len(EDGES) - 1, 12).sum(0))
    return tstate


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def launches(fn):
    """GPU kernels + memcpys of one call, counted by the profiler in a pass of its own (never inside a timed window)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as exc:
        return f"not measured ({type(exc).__name__})"


paths = [("hip_channels_last", hip_cl, 200), ("hip_nchw", hip_nchw, 200), ("torch_ops", torch_ops, 50)]
for _, fn, _n in paths:
    for _ in range(3):
        fn()
state.zero_(); tstate.zero_()
hip_cl(); torch_ops()
torch.cuda.synchronize()
agree = float(((state - tstate).abs() / tstate.abs().clamp(min=1.0)).max())
labelled = int(state[..., 0].sum().item())          # of one call: the timed calls below go on accumulating
results = {name: [] for name, _, _ in paths}
for rep in range(5):                    # alternate the paths so that clock / neighbour drift hits all alike
    for name, fn, n in paths:
        results[name].append(timed(fn, n))
out = {"tool": "time_depth_metric", "shape": {"B": B, "ncam": NCAM, "D": D, "fH": FH, "fW": FW, "ranges": len(EDGES) - 1,
                                              "groups": NCAM}, "logit_bytes": B * NCAM * D * FH * FW * 4,
       "labelled": labelled, "max_rel_diff_vs_torch_ops": agree}
for name, fn, _ in paths:
    r = sorted(results[name])
    out[name] = {"median_us": round(r[len(r) // 2], 2), "min_us": round(r[0], 2), "max_us": round(r[-1], 2),
                 "launches": launches(fn)}
print(json.dumps(out))
