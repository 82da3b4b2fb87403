"""LiDAR depth supervision at the workload's size: B = 4, 6 cameras of 256 x 704, D = 112 depth bins, 4 x 300 k points.
ops.depth_sup (csrc/depth_sup.hip: labels in 3 launches, loss forward in 2, backward in 1) against the same computation
written with PyTorch ops on the same device (batched matmul projection + scatter_reduce(amin) for the labels; softmax +
F.binary_cross_entropy + autograd for the loss), HIP events, the two alternated in one process.  Prints both times and the
launches of each.  Run it under a time limit:  timeout -k 10 300 python tools/time_depth_sup.py"""
import os as _os; _os.environ.setdefault("UD_RANDOM_INIT", "1")
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
import numpy as np
import torch
import torch.nn.functional as F
from unidistill_amd import _lib, synthetic as syn
from unidistill_amd.ops import depth_sup

assert torch.cuda.is_available(), "time_depth_sup.py measures on the GPU only"
dev = torch.device("cuda:0")
B, NCAM, H, W, DS, D_BOUND, C, NPTS = 4, 6, 256, 704, 16, [2.0, 58.0, 0.5], 80, 300000
FH, FW, D = H // DS, W // DS, 112
g = syn.rng(0)
s2e, intrin, ida, bda = (torch.from_numpy(a).to(dev) for a in syn.camera_rig(g, B, NCAM, bda_aug=True))
s2e, intrin, ida = s2e[:, 0].contiguous(), intrin[:, 0].contiguous(), ida[:, 0].contiguous()
clouds = [syn.lidar_cloud(g, NPTS // 10 + 2500, 10)[:NPTS] for _ in range(B)]        # 10 sweeps, ~300 k rows after the range filter
points = torch.from_numpy(syn.pad_clouds(clouds)).to(dev)
feat = (torch.randn(B * NCAM, D + C, FH, FW, device=dev) * 2).contiguous(memory_format=torch.channels_last)


def hip_labels():
    return depth_sup.lidar_depth_labels(points, s2e, intrin, ida, bda, D_BOUND, (H, W), DS)[1]


def torch_labels():
    """The same rules with library ops, in float64 like the kernel: inverse, batched matmuls, masks, scatter_reduce(amin)."""
    minv = torch.linalg.inv(bda.double()[:, None] @ s2e.double())                      # [B, ncam, 4, 4]
    xyz1 = torch.cat([points[..., :3].double(), torch.ones_like(points[..., :1], dtype=torch.float64)], -1)
    q = torch.einsum("bcij,bnj->bcni", minv, xyz1)                                     # [B, ncam, N, 4]
    pix = torch.einsum("bcij,bcnj->bcni", intrin.double()[..., :3, :3], q[..., :3])
    uvd = torch.stack([pix[..., 0] / pix[..., 2], pix[..., 1] / pix[..., 2], q[..., 2], torch.ones_like(q[..., 2])], -1)
    uvd = torch.einsum("bcij,bcnj->bcni", ida.double(), uvd)
    u, v, d = uvd[..., 0], uvd[..., 1], uvd[..., 2]
    pad = (points[..., :3] == 0).all(-1)[:, None]
    ok = (torch.isfinite(uvd).all(-1) & (d >= D_BOUND[0]) & (d < D_BOUND[1]) & (u >= 0) & (u < W) & (v >= 0) & (v < H) & ~pad)
    cell = (torch.floor(v / DS).long().clamp(0, FH - 1) * FW + torch.floor(u / DS).long().clamp(0, FW - 1))
    cell = cell + torch.arange(B * NCAM, device=dev).view(B, NCAM, 1) * (FH * FW)
    dmin = torch.full((B * NCAM * FH * FW,), float("inf"), device=dev)
    dmin.scatter_reduce_(0, cell[ok], d[ok].float(), "amin")
    k = torch.floor((dmin.double() - D_BOUND[0]) / D_BOUND[2])
    return torch.where(torch.isfinite(dmin) & (k >= 0) & (k < D), k, -1.0).int().view(B, NCAM, FH, FW)


label = hip_labels().view(B * NCAM, FH, FW)
same = (torch_labels().view_as(label) == label).float().mean()
print(f"{B} x {points.shape[1]} points, {B * NCAM} images of {FH} x {FW} cells, D = {D}; labelled cells "
      f"{int((label >= 0).sum())} of {label.numel()}; library-op labels agree on {100 * float(same):.3f} % of the cells")


def hip_loss():
    x = feat.detach().requires_grad_(True)
    depth_sup.depth_loss(x[:, :D], label).backward()
    return x.grad


def torch_loss():
    x = feat.detach().requires_grad_(True)
    fg = label >= 0
    p = torch.softmax(x[:, :D], 1).permute(0, 2, 3, 1)[fg]
    t = F.one_hot(label[fg].long(), D).float()
    (F.binary_cross_entropy(p, t, reduction="sum") / fg.sum().clamp(min=1)).backward()
    return x.grad


def hip_loss_fwd():
    with torch.no_grad():
        return depth_sup.depth_loss(feat[:, :D], label)


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


paths = [("labels, ops.depth_sup", hip_labels, 20), ("labels, PyTorch ops (fp64 matmul + scatter_reduce amin)", torch_labels, 5),
         ("loss fwd + bwd, ops.depth_sup", hip_loss, 50), ("loss fwd + bwd, PyTorch ops (softmax + BCE + autograd)", torch_loss, 20),
         ("loss fwd only, ops.depth_sup", hip_loss_fwd, 50)]
for _, fn, _n in paths:
    for _ in range(3):
        fn()
results = {name: [] for name, _, _ in paths}
for rep in range(5):                    # alternate the paths so that clock / neighbour drift hits all alike
    for name, fn, n in paths:
        results[name].append(timed(fn, n))
for name, fn, _ in paths:
    r = sorted(results[name])
    print(f"{name:58s} device {r[len(r) // 2]:9.1f} us/call (min {r[0]:.1f}, max {r[-1]:.1f})  launches/call {launches(fn)}")
_lib.prof_enable(True)
for _ in range(10):
    hip_labels()
    hip_loss()
torch.cuda.synchronize()
_lib.prof_enable(False)
for k in ("depth_sup.k_depth_project", "depth_sup.k_depth_loss_fwd", "depth_sup.k_depth_loss_bwd"):
    ms, n = _lib.prof_read(k, reset=True)
    print(f"  {k:30s} {ms / max(n, 1) * 1e3:8.1f} us over {n} calls")
