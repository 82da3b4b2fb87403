"""The tracking metric (ops.track_metric.evaluate_tracks, csrc/track_metric.hip) at validation size: 150 scenes x 40
frames, about 200 tracked candidates per frame over the 7 tracking classes with matching ground-truth tracks, from the seeded
generator of tests/track_metric_reference.py (the dynamics of tools/time_tracking.py's generator plus the objects themselves);
the ids are the device tracker's.  Prints one JSON line: `device_ms` -- HIP events around the whole enqueue, warmed, median of the
repeats -- and `reference_ms`, the float64 reference of
tests/track_metric_reference.py on the same machine's CPU.  The reference is Python loops plus scipy: it is timed on the first
`--ref-scenes` scenes, with `--ref-thresholds` recall thresholds, and scaled by scenes and passes to the whole; its integer outputs
on those scenes must equal the device's on the same subset.
Run it under a time limit:  timeout -k 10 500 python tools/time_track_metric.py"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import track_metric_reference as R
from unidistill_amd.ops import track_metric as M
from unidistill_amd.ops import tracking as T

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", type=int, default=150)
ap.add_argument("--frames", type=int, default=40)
ap.add_argument("--objects", type=int, default=285)
ap.add_argument("--ref-scenes", type=int, default=2)
ap.add_argument("--ref-thresholds", type=int, default=40)
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
assert torch.cuda.is_available(), "time_track_metric.py measures on the GPU only"
dev = torch.device("cuda:0")
tracked, rng = R.default_config()
classes = [c for c, on in enumerate(tracked) if on]
MAX_DIST = {"car": 4.0, "truck": 4.0, "bus": 5.5, "trailer": 3.0, "pedestrian": 1.0, "motorcycle": 13.0, "bicycle": 3.0}


def case(num_scenes):
    d = R.make_case(0, num_scenes=num_scenes, num_frames=args.frames, num_objects=args.objects, classes=classes, spread=80.0,
                    extra_classes=(2, 5, 9), false_pos=12)
    fs, off, dt = T.scene_frames(d["scene"], d["timestamp_us"])
    rec, cls = torch.from_numpy(d["rec"]).to(dev), torch.from_numpy(d["cls"]).to(dev)
    ids, _, status = T.track_scenes(rec, cls, d["row_start"], d["row_count"], fs, off, dt, track_class=tracked,
                                    max_dist=[MAX_DIST.get(n, 0.0) for n in R.CLASS_NAMES])
    assert int(status.item()) == 0
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a.astype(t))).to(dev)
    gt = (up(d["gt_xyz"], np.float64), up(d["gt_cls"], np.int32), up(d["gt_num_pts"], np.int32), up(d["gt_keep"], np.uint8))
    ego = up(d["ego"], np.float64)

    def run(recall):
        return M.evaluate_tracks(rec, cls, ids, d["row_start"], d["row_count"], *gt, d["gt_instance"], d["gt_off"], ego,
                                 d["scene"], d["timestamp_us"], track_class=tracked, class_range=rng, recall=recall)
    return d, ids, run


recall = R.recall_thresholds()
d, ids, run = case(args.scenes)
for _ in range(2):
    out = run(recall)
torch.cuda.synchronize()
assert int(out["status"].item()) == 0
times = []
for _ in range(args.repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = run(recall)
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1))
counts = out["counts"].cpu().numpy()

# the reference on a smaller case of the same generator, compared with the device on that case
n_ref = max(1, min(args.ref_scenes, args.scenes))
ref_recall = recall if args.ref_thresholds >= len(recall) else recall[:: len(recall) // args.ref_thresholds][: args.ref_thresholds]
ds, ids_s, run_s = case(n_ref)
sub = run_s(ref_recall)
t0 = time.perf_counter()
ref = R.evaluate_reference(ds["rec"], ds["cls"], ids_s.cpu().numpy(), ds["row_start"], ds["row_count"], ds["gt_xyz"], ds["gt_cls"],
                           ds["gt_instance"], ds["gt_num_pts"], ds["gt_keep"], ds["gt_off"], ds["ego"], ds["scene"],
                           ds["timestamp_us"], tracked=tracked, class_range=rng, recall=ref_recall)
ref_s = time.perf_counter() - t0
assert int(sub["status"].item()) == ref["status"] == 0
equal = bool(np.array_equal(sub["counts"].cpu().numpy(), ref["counts"]) and
             sub["thresholds"].cpu().numpy().tobytes() == ref["thresholds"].tobytes())
assert equal, "device counts or thresholds differ from the reference"
scale = (args.scenes / n_ref) * ((len(recall) + 1) / (len(ref_recall) + 1))
tp = counts[:, 0, 2] + counts[:, 0, 3]
print(json.dumps({"tool": "time_track_metric", "scenes": args.scenes, "frames": args.frames, "rows": int(len(d["rec"])),
                  "gt_rows": int(len(d["gt_xyz"])), "tracked_rows_per_frame": round(float((ids > 0).sum()) / (args.scenes * args.frames), 1),
                  "thresholds": len(recall), "passes_run": int(out["valid"].sum().item()) * args.scenes,
                  "all_boxes_tp": int(tp.sum()), "all_boxes_ids": int(counts[:, 0, 3].sum()),
                  "device_ms": round(float(np.median(times)), 3), "device_ms_min": round(float(min(times)), 3),
                  "device_ms_max": round(float(max(times)), 3), "reference_ms": round(ref_s * 1e3 * scale, 1),
                  "reference_scenes_timed": n_ref, "reference_thresholds_timed": len(ref_recall),
                  "integers_equal_on_timed_scenes": equal}))
