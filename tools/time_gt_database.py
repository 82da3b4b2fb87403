"""Building the GT-sampling object database at workload size: one nuScenes-sized scene of 10 sweeps x
29 750 rows merged into the key frame (297 500 rows, D = 5) and 40 boxes.  Times, alternating in one process after a
warm-up, host call to finished result (wall clock around a device synchronise), median of 30:
  builder   ObjectDatabaseBuilder.add_scene on the device cloud: ud_points_in_boxes, ud_gt_db_count, one readback,
            ud_gt_db_extract
  torch     a PyTorch-ops restatement on the same device: the [N, M] broadcast inside test, argmax of the first hit,
            boolean indexing per box, the centre subtracted
and the kernels' own times from the library's event scopes.  Needs a GPU; prints one JSON line."""
import os as _os; _os.environ.setdefault("UD_RANDOM_INIT", "1")
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
import numpy as np
import torch
from unidistill_amd import _lib
from unidistill_amd.ops import gt_paste as gp

SWEEPS, ROWS, D, M = 10, 29750, 5, 40
CLASSES = ["car", "truck", "bus", "pedestrian"]
assert torch.cuda.is_available(), "time_gt_database.py measures on the GPU only"
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)

N = SWEEPS * ROWS
pts = np.zeros((N, D), np.float32)
pts[:, :2] = rng.normal(scale=30.0, size=(N, 2))
pts[:, 2] = rng.normal(scale=1.5, size=N)
pts[:, 3:] = rng.uniform(0, 1, (N, D - 3))
boxes = np.zeros((M, 9), np.float32)
boxes[:, :2] = rng.uniform(-50, 50, (M, 2))
boxes[:, 2] = rng.uniform(-2, 0, M)
boxes[:, 3:6] = rng.uniform([1.5, 0.6, 1.0], [10.0, 2.8, 3.5], (M, 3))
boxes[:, 6] = rng.uniform(-np.pi, np.pi, M)
labels = rng.integers(0, len(CLASSES), M)
pts_d, boxes_d = torch.from_numpy(pts).to(dev), torch.from_numpy(boxes).to(dev)


def run_builder():
    b = gp.ObjectDatabaseBuilder(CLASSES, device=dev)
    b.add_scene(pts_d, boxes, gt_labels=labels)
    return b


def run_torch():
    s = pts_d[:, None, :3] - boxes_d[None, :, :3]
    c, sn = torch.cos(boxes_d[:, 6]), torch.sin(boxes_d[:, 6])
    lx, ly = s[..., 0] * c + s[..., 1] * sn, -s[..., 0] * sn + s[..., 1] * c
    inside = (s[..., 2].abs() <= boxes_d[:, 5] / 2) & (lx.abs() < boxes_d[:, 3] / 2 + 1e-5) & \
             (ly.abs() < boxes_d[:, 4] / 2 + 1e-5)
    owner = torch.where(inside.any(dim=1), inside.int().argmax(dim=1), -1)
    out = []
    for i in range(M):
        g = pts_d[owner == i].clone()
        g[:, :3] -= boxes_d[i, :3]
        out.append(g)
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


# object sizes of both paths (torch's sin / cos may differ in the last bit, so a row on a face may fall either way; the
# clouds themselves are the GPU tests' subject)
rows_builder = np.concatenate(run_builder()._rows)
rows_torch = np.array([len(g) for g in run_torch()])
assert np.abs(rows_builder - rows_torch).sum() <= 1e-4 * N, (rows_builder, rows_torch)

fns = {"builder": run_builder, "torch": run_torch}
for fn in fns.values():
    for _ in range(5):
        fn()
times = {k: [] for k in fns}
for _ in range(30):                                     # alternating: other work on the host shifts both alike
    for k, fn in fns.items():
        times[k].append(wall(fn))
med = {k: float(np.median(v)) for k, v in times.items()}

_lib.prof_enable(True)
for _ in range(10):
    run_builder()
torch.cuda.synchronize()
_lib.prof_enable(False)
kernels = {}
for k in ("input.k_points_in_boxes", "input.k_db_tile_count", "input.k_db_scan", "input.k_db_list", "input.db_sort",
          "input.k_db_gather"):
    ms, n = _lib.prof_read(k, reset=True)
    kernels[k] = round(ms / n * 1e3, 2) if n else None   # us per call (event scope, incl. event overhead)

hits = int(rows_builder.sum())
print(json.dumps({
    "rows": N, "D": D, "boxes": M, "rows_in_boxes": hits, "share_in_boxes": round(hits / N, 4),
    "builder_ms_median": round(med["builder"], 3), "builder_ms_min": round(min(times["builder"]), 3),
    "builder_ms_max": round(max(times["builder"]), 3),
    "torch_ms_median": round(med["torch"], 3), "torch_ms_min": round(min(times["torch"]), 3),
    "torch_ms_max": round(max(times["torch"]), 3),
    "torch_over_builder": round(med["torch"] / med["builder"], 3), "calls": 30,
    "kernel_us": kernels,
    "bytes": {"k_points_in_boxes": N * 12 + N * 4 + M * 28, "k_db_tile_count": N * 4, "k_db_list": N * 4 + hits * 16,
              "db_sort": hits * 20, "k_db_gather": hits * (12 + 2 * D * 4)},
}))
