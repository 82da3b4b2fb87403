"""Forward + backward through an eval-mode BatchNorm (+ ReLU) inside a training graph (frozen_bn / norm_eval fine-tuning):
layers.dense.batchnorm_act on the frozen-statistics kernels (csrc/bn_act.hip: ud_bn_act_fwd* + ud_bn_act_bwd_frozen_ld*)
against the PyTorch-ops path taken before they existed (bn(x), ReLU under autograd), with trainable and with frozen affine
parameters, on one fp32 trunk map, one bf16 image-branch map and one fp32 voxel-row tensor of the sparse backbone.  HIP events,
the paths alternated in one process; the backward kernels' own time comes from the library's event counters in a pass of its
own.  Bytes: the tensors a pass must move (forward x -> y, backward x, dy -> dx: 5 tensors; the one-launch backward 3).
Prints one JSON line.  Run it under a time limit:  timeout -k 10 300 python tools/time_bn_frozen.py"""
import os as _os; _os.environ.setdefault("UD_RANDOM_INIT", "1")
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
import torch
from unidistill_amd import _lib
from unidistill_amd.layers.dense import batchnorm_act

assert torch.cuda.is_available(), "time_bn_frozen.py measures on the GPU only"
dev = torch.device("cuda:0")
SHAPES = [("trunk_f32", (4, 128, 180, 180), torch.float32), ("image_bf16", (24, 256, 64, 176), torch.bfloat16),
          ("voxel_rows_f32", (120000, 16), torch.float32)]
BWD_KERNELS = ("bn_act.k_bwd_frozen_dx", "bn_act.k_bwd_frozen_sums")


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def case(shape, dtype, affine_grad):
    g = torch.Generator().manual_seed(sum(shape))
    C = shape[1]
    bn = (torch.nn.BatchNorm2d if len(shape) == 4 else torch.nn.BatchNorm1d)(C, eps=1e-3, momentum=0.01)
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.5, generator=g); bn.running_var.uniform_(0.5, 2, generator=g)
        bn.weight.uniform_(0.5, 1.5, generator=g); bn.bias.normal_(0, 0.2, generator=g)
    bn = bn.to(dev).eval().requires_grad_(affine_grad)
    x = torch.randn(*shape, generator=g).to(dev).to(dtype)
    gy = torch.randn(*shape, generator=g).to(dev).to(dtype)
    if len(shape) == 4:
        x, gy = x.contiguous(memory_format=torch.channels_last), gy.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)

    def hip():
        x.grad = bn.weight.grad = bn.bias.grad = None
        batchnorm_act(bn, x, None, True).backward(gy)
        return x.grad

    def torch_ops():
        x.grad = bn.weight.grad = bn.bias.grad = None
        with _lib.strict(False):
            torch.relu(bn(x)).backward(gy)
        return x.grad

    return hip, torch_ops


out = {"tool": "time_bn_frozen", "cases": {}}
for name, shape, dtype in SHAPES:
    for affine_grad in (True, False):
        hip, torch_ops = case(shape, dtype, affine_grad)
        for fn in (hip, torch_ops):
            for _ in range(3):
                fn()
        a, b = hip().float(), torch_ops().float()
        torch.cuda.synchronize()
        tensor_bytes = a.numel() * (4 if dtype == torch.float32 else 2)
        res = {"hip": [], "torch_ops": []}
        for rep in range(5):                    # alternate the paths so that clock / neighbour drift hits both alike
            res["hip"].append(timed(hip, 50))
            res["torch_ops"].append(timed(torch_ops, 50))
        for k in BWD_KERNELS:
            _lib.prof_read(k, reset=True)
        _lib.prof_enable(True)
        for _ in range(20):
            hip()
        torch.cuda.synchronize()
        _lib.prof_enable(False)
        ms, calls = max((_lib.prof_read(k) for k in BWD_KERNELS), key=lambda t: t[1])
        bwd_us = ms * 1e3 / max(calls, 1)
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        out["cases"][f"{name}/{'affine' if affine_grad else 'frozen_affine'}"] = {
            "shape": list(shape), "tensor_bytes": tensor_bytes, "fwd_bwd_bytes": 5 * tensor_bytes,
            "hip_median_us": round(med["hip"], 2), "hip_min_us": round(min(res["hip"]), 2),
            "torch_ops_median_us": round(med["torch_ops"], 2), "torch_ops_min_us": round(min(res["torch_ops"]), 2),
            "hip_fwd_bwd_GBps": round(5 * tensor_bytes / med["hip"] / 1e3, 1),
            "torch_ops_fwd_bwd_GBps": round(5 * tensor_bytes / med["torch_ops"] / 1e3, 1),
            "speedup": round(med["torch_ops"] / med["hip"], 2),
            "bwd_launch_us": round(bwd_us, 2), "bwd_launch_GBps": round(3 * tensor_bytes / bwd_us / 1e3, 1),
            "max_abs_dx_diff_vs_torch_ops": float((a - b).abs().max())}
print(json.dumps(out))
