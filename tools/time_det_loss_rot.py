"""Gathered regression / IoU terms of the detection loss at the workload's size -- T = 6 tasks, B = 4, K = 2500 slots per sample on
180 x 180 maps, about 360 positive slots per sample and task -- forward + backward of ops.det_loss.reg_terms in both IoU modes:
"reference" (ud_det_reg_fwd / _bwd: axis-aligned IoU loss, nearest-BEV IoU-aware target) and "rotated3d" (ud_det_reg_fwd_rot / _bwd_rot:
the rotated 3-D IoU of csrc/rot_iou3d.h in both terms).  HIP events, warm-up, the two modes alternated in one process, median of the
windows; then the kernels' own times from the library's event timers.  Inputs are the shared random draw of tests/rot_iou_reference.py
(predictions near their targets), so the clip runs on overlapping boxes as it does in training.
Run it under a time limit:  timeout -k 10 300 python tools/time_det_loss_rot.py"""
import os as _os; _os.environ.setdefault("UD_RANDOM_INIT", "1")
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd"), os.path.join(ROOT, "tests")]
import torch
import rot_iou_reference as R
from unidistill_amd import _lib
from unidistill_amd.ops import det_loss

assert torch.cuda.is_available(), "time_det_loss_rot.py measures on the GPU only"
dev = torch.device("cuda:0")
T, B, K, H, W, POS = 6, 4, 2500, 180, 180, 360
SX = SY = 8 * 0.075
g = torch.Generator().manual_seed(0)
n = T * B * POS
pred, tgt8 = R.random_codes(n, SX, SY, seed=0)
ind = torch.zeros(T, B, K, dtype=torch.long)
mask = torch.zeros(T, B, K, dtype=torch.bool)
tgt = torch.zeros(T, B, K, 10)
packed = torch.randn(B, T * 11, H, W, generator=g) * 0.1                     # one packed head tensor, as PackedSepHeads returns
flat = packed.view(B, T * 11, H * W)
code = torch.cat([pred.float(), torch.randn(n, 3, generator=g) * 0.3], 1).view(T, B, POS, 11)
for t in range(T):
    for b in range(B):
        pix = torch.randperm(H * W, generator=g)[:POS].sort().values         # ascending anchors, like the assigner
        ind[t, b, :POS], mask[t, b, :POS] = pix, True
        tgt[t, b, :POS, :8] = tgt8.view(T, B, POS, 8)[t, b].float()
        flat[b, t * 11:(t + 1) * 11, pix] = code[t, b].t()
packed = packed.to(dev)
ind, mask, tgt = ind.to(dev), mask.to(dev), tgt.to(dev)
num_obj = mask.float().sum(dim=(1, 2))
w_box, w_iou = torch.rand(T, 10, device=dev) + 0.5, torch.full((T,), 5.0, device=dev)
print(f"T = {T}, B = {B}, K = {K}, maps {H} x {W}; {int(mask.sum())} positive slots of {mask.numel()} ({POS} per sample and task)")


def step(mode):
    x = packed.detach().requires_grad_(True)
    preds = []
    for t in range(T):
        c, pd = t * 11, {}
        for name, wd in zip(det_loss.HEADS, det_loss.WIDTH):
            pd[name] = x[:, c:c + wd]
            c += wd
        preds.append(pd)
    box, il, aw = det_loss.reg_terms(preds, ind, mask, tgt, num_obj, SX, SY, 10, iou_mode=mode)
    ((box * w_box).sum() + (il * w_iou).sum() + aw.sum()).backward()
    return il.detach(), aw.detach(), x.grad


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


modes = ("reference", "rotated3d")
for m in modes:
    for _ in range(5):
        out = step(m)
    print(f"  {m:10s} mean IoU loss per task {float(out[0].mean()):.4f}, IoU-aware L1 {float(out[1].mean()):.4f}, "
          f"|d heads| max {float(out[2].abs().max()):.3e}")
results = {m: [] for m in modes}
for rep in range(7):                    # alternate the modes so that clock / neighbour drift hits both alike
    for m in modes:
        results[m].append(timed(lambda: step(m), 200))
med = {}
for m in modes:
    r = sorted(results[m])
    med[m] = r[len(r) // 2]
    print(f"reg_terms fwd + bwd (autograd glue included), {m:10s} device {med[m]:8.1f} us/step (min {r[0]:.1f}, max {r[-1]:.1f})")
print(f"rotated3d - reference: {med['rotated3d'] - med['reference']:+.1f} us/step")
_lib.prof_enable(True)
for _ in range(50):
    for m in modes:
        step(m)
torch.cuda.synchronize()
_lib.prof_enable(False)
for k in ("det_loss.reg_fwd", "det_loss.reg_fwd_rot"):
    ms, cnt = _lib.prof_read(k, reset=True)
    print(f"  {k:24s} (gather kernel + ordered sum) {ms / max(cnt, 1) * 1e3:8.1f} us over {cnt} calls")
