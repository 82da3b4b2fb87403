"""Clip + AdamW on the camera student's real parameter set: PyTorch's path (clip_grad_norm_(foreach=True) + AdamW(fused=True))
against ops.optim.ClipAdamW (csrc/optim.hip), random gradients, HIP events, the two alternated in one process.
Reports launches per step, device us per step, host enqueue us per step and the bytes each path has to move.
The weight-EMA leg adds two rows in the same alternation: ClipAdamW(ema_decay=...) (the average rides in the update launch)
and ClipAdamW without it followed by torch._foreach_lerp_ on a cloned parameter list (what a host-side average costs).
UD_TIME_OPTIM_FRESH_GRADS=1 gives every step new gradient tensors (pointer upload through the pinned ring every step)."""
import os as _os; _os.environ.setdefault("UD_RANDOM_INIT", "1")   # synthetic weights (tools never train for real)
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
import torch
from unidistill_amd import _lib, train
from unidistill_amd.ops.optim import ClipAdamW

assert torch.cuda.is_available(), "time_optim.py measures on the GPU only"
dev = torch.device("cuda:0")
FRESH = os.environ.get("UD_TIME_OPTIM_FRESH_GRADS", "0") == "1"
LR, WD, CLIP, EMA_DECAY = 2e-4, 1e-7, 0.1, 0.999
torch.manual_seed(0)


def param_set():
    model = train.to_channels_last(train.build_model("camera").to(dev))
    return [p for p in model.parameters() if p.requires_grad]


def give_grads(params, scale):
    for p in params:
        p.grad = torch.randn_like(p) * scale


class TorchPath:
    name = "torch clip_grad_norm_ + AdamW(fused)"

    def __init__(self):
        self.params = param_set()
        self.opt = torch.optim.AdamW(self.params, lr=LR, weight_decay=WD, fused=True)

    def step(self):
        torch.nn.utils.clip_grad_norm_(self.params, CLIP, foreach=True)
        self.opt.step()


class HipPath:
    name = "ClipAdamW (2 launches)"

    def __init__(self):
        self.params = param_set()
        self.opt = ClipAdamW(self.params, lr=LR, weight_decay=WD, max_norm=CLIP)

    def step(self):
        self.opt.step()


class HipEmaPath(HipPath):
    name = "ClipAdamW + fused EMA (2 launches)"

    def __init__(self):
        self.params = param_set()
        self.opt = ClipAdamW(self.params, lr=LR, weight_decay=WD, max_norm=CLIP, ema_decay=EMA_DECAY)


class HipForeachEmaPath(HipPath):
    name = "ClipAdamW, then _foreach_lerp_ EMA"

    def __init__(self):
        super().__init__()
        self.ema = [p.detach().clone() for p in self.params]

    @torch.no_grad()
    def step(self):
        self.opt.step()
        torch._foreach_lerp_(self.ema, self.params, 1.0 - EMA_DECAY)


def timed(path, n):
    """-> (device us / step, host enqueue us / step) over n steps."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if FRESH:
        dev_us, host_us = 0.0, 0.0
        for _ in range(n):
            give_grads(path.params, 1e-3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record(); path.step(); e1.record()
            host_us += (time.perf_counter() - t0) * 1e6
            torch.cuda.synchronize()
            dev_us += e0.elapsed_time(e1) * 1e3
        return dev_us / n, host_us / n
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        path.step()
    e1.record()
    host = (time.perf_counter() - t0) * 1e6 / n
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n, host


def launches(path):
    """GPU kernels + memcpys of one step, counted by the profiler in a pass of its own (never inside a timed window)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            path.step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as exc:   # the count is a by-product; the timing above stands without it
        return f"not measured ({type(exc).__name__})"


paths = [TorchPath(), HipPath(), HipEmaPath(), HipForeachEmaPath()]
n_param = sum(p.numel() for p in paths[0].params)
print(f"camera student: {len(paths[0].params)} trainable tensors, {n_param / 1e6:.2f} M parameters, "
      f"{paths[1].opt._n_chunks} chunks of {paths[1].opt._chunk}; gradients {'new every step' if FRESH else 'static'}")
for path in paths:
    give_grads(path.params, 1e-3)       # total norm ~ 1e-3 * sqrt(N): above the 0.1 threshold, the clip is active
    for _ in range(5):
        path.step()
torch.cuda.synchronize()
results = {p.name: [] for p in paths}
for rep in range(5):                    # alternate the paths so that clock / neighbour drift hits all alike
    for path in paths:
        results[path.name].append(timed(path, 10 if FRESH else 50))
# bytes the algorithm has to move (fp32): torch = norm read g; clip read + write g; AdamW read p, m, v, g, write p, m, v
# hip = sqnorm read g; AdamW read p, m, v, g, write p, m, v; fused EMA: + read e, write e; foreach EMA: + read p, e, write e
need = {paths[0].name: 10 * 4 * n_param, paths[1].name: 8 * 4 * n_param, paths[2].name: 10 * 4 * n_param,
        paths[3].name: 11 * 4 * n_param}
med_of = {}
for path in paths:
    runs = results[path.name]
    dev_us = sorted(r[0] for r in runs)
    host_us = sorted(r[1] for r in runs)
    med = dev_us[len(dev_us) // 2]
    med_of[path.name] = med
    print(f"{path.name:40s} device {med:8.1f} us/step (min {dev_us[0]:.1f}, max {dev_us[-1]:.1f})  "
          f"host enqueue {host_us[len(host_us) // 2]:8.1f} us/step  launches/step {launches(path)}  "
          f"bytes {need[path.name] / 1e6:.0f} MB -> {need[path.name] / med / 1e6:.2f} TB/s")
base = med_of[paths[1].name]
print(f"weight EMA: fused {med_of[paths[2].name] / base:.3f} x, _foreach_lerp_ {med_of[paths[3].name] / base:.3f} x the ClipAdamW "
      f"step without one; fused / foreach {med_of[paths[2].name] / med_of[paths[3].name]:.3f}")
_lib.prof_enable(True)
for _ in range(10):
    paths[1].step()
    paths[2].step()
torch.cuda.synchronize()
_lib.prof_enable(False)
for k in ("optim.k_sqnorm", "optim.k_clip_adamw", "optim.k_clip_adamw_ema"):
    ms, n = _lib.prof_read(k, reset=True)
    print(f"  {k:22s} {ms / max(n, 1) * 1e3:8.1f} us over {n} calls")
print(f"  skipped {float(paths[1].opt.skipped):.0f}, last total_norm {float(paths[1].opt.last_norm):.4f}, "
      f"coef {float(paths[1].opt.last_coef):.4f}, pointer uploads {paths[1].opt.grad_uploads}")
