"""GT-sampling paste in the LiDAR input chain at workload size: B = 4 samples x 10 clouds, about 1.19 M
rows, 40 candidates per sample from the reference's sampler_groups (base_nuscenes_cfg.py:70-81).  Times, alternating in
one process after a warm-up, host call to finished result (wall clock around a device synchronise):
  paste     lidar_paste_host_clouds: selection + chain with removal and paste
  no paste  lidar_prep_host_clouds on the same clouds and plans without the paste record
  torch     a PyTorch-ops formulation of remove + concat alone on device clouds (what the paste adds to the chain)
and the kernels' own times from the library's event scopes.  Needs a GPU; prints one line per figure."""
import os as _os; _os.environ.setdefault("UD_RANDOM_INIT", "1")
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
import numpy as np
import torch
from unidistill_amd import _lib
from unidistill_amd.ops import gt_paste as gp, input_prep as ip

CLASSES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
           "traffic_cone"]
GROUPS = ["car:2", "truck:3", "construction_vehicle:7", "bus:4", "trailer:6", "barrier:2", "motorcycle:6", "bicycle:6",
          "pedestrian:2", "traffic_cone:2"]
PCR = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
B, CLOUDS, ROWS, D = 4, 10, 29750, 5
dev = torch.device("cuda:0")
assert torch.cuda.is_available(), "time_gt_paste.py measures on the GPU only"
rng = np.random.default_rng(0)


def boxes(n):
    b = np.zeros((n, 9), np.float32)
    b[:, :2] = rng.uniform(-50, 50, (n, 2))
    b[:, 2] = rng.uniform(-2, 0, n)
    b[:, 3:6] = rng.uniform([1.5, 0.6, 1.0], [10.0, 2.8, 3.5], (n, 3))
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


n_obj = 40 * len(CLASSES)
sizes = rng.integers(5, 400, n_obj)
db = gp.ObjectDatabase.from_arrays(rng.normal(scale=1.0, size=(int(sizes.sum()), D)).astype(np.float32),
                                   np.concatenate([[0], np.cumsum(sizes)]), boxes(n_obj), np.arange(n_obj) % len(CLASSES),
                                   CLASSES, device=dev)
sampler = gp.GTSampling(db, CLASSES, GROUPS, seed=0)
clouds, plain, paste = [], [], []
for b in range(B):
    cs = []
    for _ in range(CLOUDS):
        p = np.zeros((ROWS, D), np.float32)
        p[:, :2] = rng.normal(scale=30.0, size=(ROWS, 2))
        p[:, 2] = rng.normal(scale=1.5, size=ROWS)
        cs.append(p)
    mats = []
    for _ in range(CLOUDS - 1):
        m = np.eye(4)
        m[:3, 3] = rng.normal(scale=[2.0, 2.0, 0.05])
        mats.append(m)
    aug = {"segments": [ROWS] * CLOUDS, "sweep_mats": np.stack(mats), "bda_mat": None, "range": None,
           "time_lags": rng.uniform(0, 0.5, CLOUDS - 1).astype(np.float32)}
    d = sampler({"points": cs[0], "gt_boxes": boxes(30), "gt_labels": rng.integers(0, 10, 30), "lidar_aug": dict(aug)})
    bda = ip.bev_transform_matrix(rng.uniform(-45, 45), rng.uniform(0.9, 1.1), rng.normal(scale=0.5, size=3), True, False)
    for a in (aug, d["lidar_aug"]):
        a["bda_mat"], a["range"] = bda, np.array(PCR, np.float32)
    clouds.append(cs)
    plain.append(aug)
    paste.append(d["lidar_aug"])

run_paste = lambda: gp.lidar_paste_host_clouds(clouds, paste, dev)
run_plain = lambda: ip.lidar_prep_host_clouds(clouds, plain, dev)

# the PyTorch-ops formulation of what the paste adds: per sample, points-in-boxes over the accepted boxes, index, cat
out, counts, accept = run_paste()
torch.cuda.synchronize()
recs = [a["paste"] for a in paste]
scene_d = [torch.from_numpy(np.concatenate(cs)).to(dev) for cs in clouds]
acc_boxes = [torch.from_numpy(db.boxes[p["cand_idx"][p["accept"]], :7]).to(dev) for p in recs]
obj_d = [torch.cat([db.points[db.offsets[i]:db.offsets[i + 1]] for i in p["cand_idx"][p["accept"]]] + [db.points[:0]])
         for p in recs]


def run_torch():
    outs = []
    for pts, bx, obj in zip(scene_d, acc_boxes, obj_d):
        s = pts[:, None, :3] - bx[None, :, :3]
        c, sn = torch.cos(bx[:, 6]), torch.sin(bx[:, 6])
        lx, ly = s[..., 0] * c + s[..., 1] * sn, -s[..., 0] * sn + s[..., 1] * c
        inside = (s[..., 2].abs() <= bx[:, 5] / 2) & (lx.abs() < bx[:, 3] / 2 + 1e-5) & (ly.abs() < bx[:, 4] / 2 + 1e-5)
        outs.append(torch.cat([obj, pts[~inside.any(dim=1)]]))
    return outs


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


fns = {"paste": run_paste, "no paste": run_plain, "torch": run_torch}
for fn in fns.values():
    for _ in range(5):
        fn()
times = {k: [] for k in fns}
for _ in range(30):                                     # alternating: other work on the host shifts all three alike
    for k, fn in fns.items():
        times[k].append(wall(fn))
rows_in = B * CLOUDS * ROWS
print(f"rows {rows_in}  candidates/sample {[len(p['cand_idx']) for p in recs]}  accepted {[int(p['accept'].sum()) for p in recs]}  "
      f"kept rows {[int(c) for c in counts]}")
med = {k: float(np.median(v)) for k, v in times.items()}
for k, v in times.items():
    print(f"{k:9s} median {med[k]:7.3f} ms   min {min(v):7.3f}   max {max(v):7.3f}   (30 calls, host call -> synchronise)")
print(f"paste / no paste = {med['paste'] / med['no paste']:.3f}")

_lib.prof_enable(True)
for _ in range(10):
    run_paste()
    run_plain()
torch.cuda.synchronize()
_lib.prof_enable(False)
for k in ("input.k_gt_paste_select", "input.k_lidar_count_paste", "input.k_lidar_scatter_paste", "input.k_lidar_count",
          "input.k_lidar_scatter", "input.k_lidar_scan"):
    ms, n = _lib.prof_read(k, reset=True)
    if n:
        print(f"{k:30s} {ms / n * 1e3:8.1f} us per launch over {n} launches (event scope, incl. event overhead)")
print(f"bytes per input row: {D * 4} read twice (count, scatter) + {D * 4} written for a kept row; box test per scene row: "
      f"up to 40 boxes x ~10 flops")
