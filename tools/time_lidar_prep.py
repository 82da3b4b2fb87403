"""GPU timing of the LiDAR input chain after collate at production sizes: B = 4 samples x 10 clouds x
34 720 points, D = 5, random poses, BDA and the nuScenes range.  Prints the per-kernel times (device events, after
warm-up), the one H2D copy of the staged clouds, the host time of lidar_prep_host_clouds per batch (what collate_fn
spends on the points), and the host time of the reference's numpy chain (CollectLidarSweeps -> BevAffineTransformation
-> ObjectRangeFilter, float64 matmuls as in transforms3d.py) per sample on this machine's CPU.
    python tools/time_lidar_prep.py            [B=4 SWEEPS=10 N=34720 ITERS=30]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
import numpy as np
import torch

from unidistill_amd import _lib
from unidistill_amd.ops import input_prep as ip

B, SWEEPS, N = int(os.environ.get("B", 4)), int(os.environ.get("SWEEPS", 10)), int(os.environ.get("N", 34720))
ITERS = int(os.environ.get("ITERS", 30))
PCR = np.array([-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], np.float32)
d = torch.device("cuda:0")
rng = np.random.default_rng(0)


def pose():
    a = rng.uniform(-np.pi, np.pi)
    m = np.eye(4)
    m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    m[:3, 3] = rng.normal(scale=[300.0, 300.0, 1.0])
    return m


clouds, plans = [], []
for b in range(B):
    cs = []
    for _ in range(SWEEPS):
        p = np.zeros((N, 5), np.float32)
        p[:, :2] = rng.normal(scale=35.0, size=(N, 2))
        p[:, 2] = rng.normal(scale=2.0, size=N)
        p[:, 3] = rng.integers(0, 256, N)
        cs.append(p)
    l2e, e2g = pose(), pose()
    mats = []
    for _ in range(SWEEPS - 1):
        sweep_pose = e2g.copy()
        sweep_pose[:3, 3] += rng.normal(scale=[3.0, 3.0, 0.1])
        mats.append(ip.sweep_to_key_matrix(l2e, e2g, sweep_pose))
    plans.append({"segments": [N] * SWEEPS, "sweep_mats": np.stack(mats),
                  "time_lags": rng.uniform(0, 0.5, SWEEPS - 1).astype(np.float32),
                  "bda_mat": ip.bev_transform_matrix(20.0, 1.05, [0.1, -0.2, 0.05], True, False), "range": PCR})
    clouds.append(cs)


def reference_chain(cs, plan):
    """The reference's per-sample numpy work (transforms3d.py:379-443, :242-255): float64 homogeneous matmuls."""
    allp = cs[0].copy()
    allp[:, -1] = 0.0
    for j, f in enumerate(cs[1:]):
        f = f.copy()
        h = np.ones((f.shape[0], 4))
        h[:, :3] = f[:, :3]
        f[:, :3] = (plan["sweep_mats"][j] @ h.T).T[:, :3]
        f[:, -1] = plan["time_lags"][j]
        allp = np.concatenate([allp, f])
    h = np.ones((allp.shape[0], 4))
    h[:, :3] = allp[:, :3]
    allp[:, :3] = (plan["bda_mat"] @ h.T).T[:, :3]
    r = plan["range"]
    m = (allp[:, 0] >= r[0]) & (allp[:, 0] <= r[3]) & (allp[:, 1] >= r[1]) & (allp[:, 1] <= r[4])
    return allp[m]


rows = B * SWEEPS * N
nbytes = rows * 5 * 4
for _ in range(3):
    out = ip.lidar_prep_host_clouds(clouds, plans, d)
torch.cuda.synchronize()
kept = out.shape[1]

# kernel times (library event timing on the input stream)
_lib.prof_enable(True)
for name in ("input.k_lidar_count", "input.k_lidar_scan", "input.k_lidar_scatter"):
    _lib.prof_read(name)
for _ in range(ITERS):
    ip.lidar_prep_host_clouds(clouds, plans, d)
torch.cuda.synchronize()
kt = {}
for name in ("input.k_lidar_count", "input.k_lidar_scan", "input.k_lidar_scatter"):
    ms, n = _lib.prof_read(name)
    kt[name] = ms / max(n, 1) * 1e3
_lib.prof_enable(False)

# H2D of the staged batch (pinned -> device, its own stream)
host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
dev = torch.empty(nbytes, dtype=torch.uint8, device=d)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _ in range(3):
    dev.copy_(host, non_blocking=True)
e0.record()
for _ in range(ITERS):
    dev.copy_(host, non_blocking=True)
e1.record()
torch.cuda.synchronize()
h2d_us = e0.elapsed_time(e1) / ITERS * 1e3

# host time of the whole call (packing + launches + count readback), nothing else queued
t0 = time.perf_counter()
for _ in range(ITERS):
    ip.lidar_prep_host_clouds(clouds, plans, d)
torch.cuda.synchronize()
call_ms = (time.perf_counter() - t0) / ITERS * 1e3
t0 = time.perf_counter()
for _ in range(ITERS):
    ip.lidar_prep_host_clouds(clouds, plans, d)
host_ms = (time.perf_counter() - t0) / ITERS * 1e3                  # returns before the scatter finishes
torch.cuda.synchronize()

# the reference chain on this host, one sample at a time (numpy, default threading)
t0 = time.perf_counter()
for b in range(B):
    reference_chain(clouds[b], plans[b])
ref_ms = (time.perf_counter() - t0) / B * 1e3

print(f"batch: B={B} x {SWEEPS} clouds x {N} points, D=5: {rows} rows, {nbytes / 1e6:.1f} MB in, "
      f"Nmax={kept} ({B * kept * 20 / 1e6:.1f} MB out)")
for k, v in kt.items():
    print(f"  {k:24s} {v:8.1f} us")
print(f"  H2D of the staged clouds     {h2d_us:8.1f} us ({nbytes / h2d_us / 1e3:.1f} GB/s)")
print(f"  lidar_prep_host_clouds host  {host_ms:8.2f} ms per batch (call through completion {call_ms:.2f} ms)")
print(f"  reference chain on the host  {ref_ms:8.2f} ms per sample ({B * ref_ms:.1f} ms per batch)")
