"""The nuScenes tracking metric on the device (csrc/track_metric.hip): the counts behind AMOTA, AMOTP, MOTA, IDS
and the other figures of the devkit's TrackingEval, for every (class, recall threshold) at once.

``evaluate_tracks`` is the whole evaluation in one enqueue without a host wait: kept flags and track mean scores, the all-boxes
pass, the recall thresholds, the threshold passes and the sums over the scenes.  The host half here orders the frames
(``tracking.scene_frames``), numbers the GT instances densely per (scene, class) and checks the caps before anything is
launched.  The algorithm is stated in include/unidistill_hip.h and restated in tests/track_metric_reference.py."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .nus_eval import MAX_CLASSES, PRED_COLS
from .tracking import scene_frames

MAX_FRAME_ROWS = 512      # UD_TM_MAX_FRAME_ROWS
MAX_INSTANCES = 4096      # UD_TM_MAX_INSTANCES
MAX_THRESHOLDS = 64       # UD_TM_MAX_THRESHOLDS
COUNTS = ("frames", "objects", "matches", "switches", "fp", "miss", "mt", "ml", "frag", "tid", "lgd", "inst")
ST_NONFINITE, ST_BOXES, ST_RANGE, ST_ID, ST_INTERNAL = 1, 2, 4, 8, 16


class Cfg(ctypes.Structure):
    """UdTrackMetricCfg of include/unidistill_hip.h."""
    _fields_ = [("num_classes", ctypes.c_int), ("num_thresholds", ctypes.c_int), ("max_boxes_per_sample", ctypes.c_int),
                ("events_pass", ctypes.c_int), ("max_frame_rows", ctypes.c_int), ("max_instances", ctypes.c_int),
                ("num_rows", ctypes.c_int64), ("num_gt", ctypes.c_int64), ("num_samples", ctypes.c_int64),
                ("num_frames", ctypes.c_int64), ("num_scenes", ctypes.c_int64), ("max_scene_rows", ctypes.c_int64),
                ("dist_th_tp", ctypes.c_double), ("class_range", ctypes.c_double * MAX_CLASSES),
                ("class_gt", ctypes.c_int64 * MAX_CLASSES), ("track_class", ctypes.c_uint8 * (MAX_CLASSES + 1))]


def status_text(bits):
    out = []
    if bits & ST_NONFINITE:
        out.append("a row of a tracked class has a non-finite translation or score")
    if bits & ST_BOXES:
        out.append("a sample has more kept predictions than max_boxes_per_sample")
    if bits & ST_RANGE:
        out.append("a frame's sample, a sample's rows, a scene's frames or an instance number lie outside the inputs")
    if bits & ST_ID:
        out.append("a track id exceeds the number of prediction rows of its scene")
    if bits & ST_INTERNAL:
        out.append("the assignment solver stopped at its guard")
    return "; ".join(out)


def dense_instances(gt_instance, gt_cls, gt_sample, scene):
    """Host: instance ids (any int64, unique per object) -> (int32 numbers dense within each (scene, class), the largest count of
    one (scene, class)).  Raises if an object appears twice in one sample."""
    inst = np.asarray(gt_instance, dtype=np.int64).reshape(-1)
    cls = np.asarray(gt_cls, dtype=np.int64).reshape(-1)
    sample = np.asarray(gt_sample, dtype=np.int64).reshape(-1)
    if not len(inst):
        return np.zeros(0, np.int32), 0
    sc = np.asarray(scene, dtype=np.int64).reshape(-1)[sample]
    per_sample = np.stack([sample, cls, inst], 1)
    if len(np.unique(per_sample, axis=0)) != len(inst):
        raise ValueError("evaluate_tracks: a ground-truth instance appears twice in one sample")
    keys, inverse = np.unique(np.stack([sc, cls, inst], 1), axis=0, return_inverse=True)
    group_first = np.ones(len(keys), dtype=bool)
    group_first[1:] = (keys[1:, :2] != keys[:-1, :2]).any(1)
    start = np.maximum.accumulate(np.where(group_first, np.arange(len(keys)), 0))
    dense = (np.arange(len(keys)) - start).astype(np.int32)
    return dense[inverse.reshape(-1)], int(dense.max()) + 1


def _host_i64(x, n, name):
    a = np.array(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.int64).reshape(-1)
    if len(a) != n:
        raise ValueError(f"evaluate_tracks: {name} needs {n} entries, got {len(a)}")
    return a


def evaluate_tracks(rec, cls, track_id, row_start, row_count, gt_xyz, gt_cls, gt_num_pts, gt_keep, gt_instance, gt_off, ego,
                    scene, timestamp_us, *, track_class, class_range, recall, dist_th_tp=2.0, max_boxes_per_sample=500,
                    events_pass=None):
    """Device: rec f64 [P, 10], cls i32 [P], track_id i32 [P] (the evaluator's rows and the tracker's ids); gt_xyz f64 [G, 3],
    gt_cls i32 [G], gt_num_pts i32 [G], gt_keep u8 [G] (GT rows sorted by sample); ego f64 [S, 3].  Host: row_start / row_count
    [S], gt_instance int64 [G], gt_off [S + 1], scene / timestamp_us [S], recall [K].  track_class: a bool per class;
    class_range: metres per class.  events_pass: None, "none" (the all-boxes pass) or a threshold index.
    -> dict of device tensors: counts i64 [T, K + 1, 12] (``COUNTS``; T = tracked classes in class order, entry 0 of the second
    axis = all boxes), dist_sum f64 / valid i32 [T, K + 1], thresholds f64 [T, K], num_scores i64 [T], status i32 [1]
    (``status_text``), events_type / events_row i32 [G] or None; plus "classes": the class index of each of the T slots.
    Nothing is read back here."""
    _lib.require_gpu(rec, cls, track_id, gt_xyz, gt_cls, gt_num_pts, gt_keep, ego)
    dev = rec.device
    if rec.dtype != torch.float64 or rec.dim() != 2 or rec.shape[1] != PRED_COLS:
        raise ValueError(f"evaluate_tracks: rec must be float64 [P, {PRED_COLS}], got {rec.dtype} {tuple(rec.shape)}")
    P = int(rec.shape[0])
    for t, name in ((cls, "cls"), (track_id, "track_id")):
        if t.dtype != torch.int32 or tuple(t.shape) != (P,):
            raise ValueError(f"evaluate_tracks: {name} must be int32 [{P}], got {t.dtype} {tuple(t.shape)}")
    if gt_xyz.dtype != torch.float64 or gt_xyz.dim() != 2 or gt_xyz.shape[1] != 3:
        raise ValueError(f"evaluate_tracks: gt_xyz must be float64 [G, 3], got {gt_xyz.dtype} {tuple(gt_xyz.shape)}")
    G = int(gt_xyz.shape[0])
    for t, name, dt in ((gt_cls, "gt_cls", torch.int32), (gt_num_pts, "gt_num_pts", torch.int32), (gt_keep, "gt_keep", torch.uint8)):
        if t.dtype != dt or tuple(t.shape) != (G,):
            raise ValueError(f"evaluate_tracks: {name} must be {dt} [{G}], got {t.dtype} {tuple(t.shape)}")
    if ego.dtype != torch.float64 or ego.dim() != 2 or ego.shape[1] != 3 or ego.shape[0] < 1:
        raise ValueError(f"evaluate_tracks: ego must be float64 [S, 3], got {ego.dtype} {tuple(ego.shape)}")
    S = int(ego.shape[0])
    track_class = [bool(v) for v in track_class]
    class_range = [float(v) for v in class_range]
    C = len(track_class)
    if not 1 <= C <= MAX_CLASSES or len(class_range) != C or not any(track_class):
        raise ValueError(f"evaluate_tracks: 1 .. {MAX_CLASSES} classes with one range each and at least one tracked, got {C} "
                         f"and {len(class_range)}")
    if any(t and not r >= 0.0 for t, r in zip(track_class, class_range)):
        raise ValueError("evaluate_tracks: the range of a tracked class must not be NaN or negative")
    recall = np.array(recall, dtype=np.float64).reshape(-1)
    K = len(recall)
    if not 1 <= K <= MAX_THRESHOLDS or not np.isfinite(recall).all():
        raise ValueError(f"evaluate_tracks: 1 .. {MAX_THRESHOLDS} finite recall thresholds, got {K}")
    if not (dist_th_tp > 0.0 and np.isfinite(dist_th_tp)) or int(max_boxes_per_sample) < 1:
        raise ValueError("evaluate_tracks: dist_th_tp must be positive and finite, max_boxes_per_sample at least 1")
    if events_pass is None:
        ev = -2
    elif events_pass == "none":
        ev = -1
    elif isinstance(events_pass, (int, np.integer)) and 0 <= events_pass < K:
        ev = int(events_pass)
    else:
        raise ValueError(f"evaluate_tracks: events_pass must be None, 'none' or 0 .. {K - 1}, got {events_pass!r}")
    h_start, h_count = _host_i64(row_start, S, "row_start"), _host_i64(row_count, S, "row_count")
    h_off = _host_i64(gt_off, S + 1, "gt_off")
    h_inst = _host_i64(gt_instance, G, "gt_instance")
    h_scene, h_ts = _host_i64(scene, S, "scene"), _host_i64(timestamp_us, S, "timestamp_us")
    if h_count.min() < 0 or (h_start < 0).any() or (h_start + h_count > P).any():
        raise ValueError(f"evaluate_tracks: a sample's rows lie outside the {P} prediction rows")
    if h_off[0] != 0 or h_off[-1] != G or (np.diff(h_off) < 0).any():
        raise ValueError(f"evaluate_tracks: gt_off must ascend from 0 to the {G} ground-truth rows")
    g_count = np.diff(h_off)
    frame_rows = int(max(h_count.max(), g_count.max()))
    if frame_rows > MAX_FRAME_ROWS:
        raise ValueError(f"evaluate_tracks: a sample has {frame_rows} prediction or ground-truth rows, more than {MAX_FRAME_ROWS}")
    frame_sample, scene_off, _ = scene_frames(h_scene, h_ts)
    NS = len(scene_off) - 1
    if int(np.diff(scene_off).max()) > 65534:
        raise ValueError("evaluate_tracks: a scene has more than 65534 frames")
    h_gcls = gt_cls.cpu().numpy() if G else np.zeros(0, np.int32)          # GT comes from the host: this is no result read
    if G and (h_gcls.min() < 0 or h_gcls.max() >= C):
        raise ValueError(f"evaluate_tracks: ground-truth class id outside 0 .. {C - 1}")
    gt_sample = np.repeat(np.arange(S), g_count)
    dense, max_inst = dense_instances(h_inst, h_gcls, gt_sample, h_scene)
    if max_inst > MAX_INSTANCES:
        raise ValueError(f"evaluate_tracks: {max_inst} ground-truth instances in one (scene, class), more than {MAX_INSTANCES}")
    scene_rows = np.add.reduceat(h_count[frame_sample], scene_off[:-1])

    cfg = Cfg(num_classes=C, num_thresholds=K, max_boxes_per_sample=int(max_boxes_per_sample), events_pass=ev,
              max_frame_rows=frame_rows, max_instances=max_inst, num_rows=P, num_gt=G, num_samples=S, num_frames=S,
              num_scenes=NS, max_scene_rows=int(scene_rows.max()), dist_th_tp=float(dist_th_tp))
    per_class = np.bincount(h_gcls, minlength=C)
    for c in range(C):
        cfg.class_range[c] = class_range[c]
        cfg.class_gt[c] = int(per_class[c])
        cfg.track_class[c] = 1 if track_class[c] else 0
    slots = [c for c in range(C) if track_class[c]]
    T = len(slots)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_start, d_count, d_off, d_inst = up(h_start), up(h_count), up(h_off), up(dense)
    d_frames, d_scene_off, d_recall = up(frame_sample), up(scene_off), up(recall)
    out = {"counts": torch.empty((T, K + 1, len(COUNTS)), dtype=torch.int64, device=dev),
           "dist_sum": torch.empty((T, K + 1), dtype=torch.float64, device=dev),
           "valid": torch.empty((T, K + 1), dtype=torch.int32, device=dev),
           "thresholds": torch.empty((T, K), dtype=torch.float64, device=dev),
           "num_scores": torch.empty((T,), dtype=torch.int64, device=dev),
           "status": torch.zeros((1,), dtype=torch.int32, device=dev),
           "events_type": torch.empty((G,), dtype=torch.int32, device=dev) if ev != -2 else None,
           "events_row": torch.empty((G,), dtype=torch.int32, device=dev) if ev != -2 else None,
           "classes": slots}
    nbytes = _lib.load().ud_track_metric_workspace_bytes(ctypes.addressof(cfg))
    if nbytes == 0:
        raise ValueError("evaluate_tracks: the sizes are outside the supported range")
    ws = _lib.workspace(dev, nbytes, slot="track_metric")
    _lib.ud.ud_track_metric(rec.contiguous(), cls.contiguous(), track_id.contiguous(), d_start, d_count, gt_xyz.contiguous(),
                            gt_cls.contiguous(), gt_num_pts.contiguous(), gt_keep.contiguous(), d_inst, d_off, ego.contiguous(),
                            d_frames, d_scene_off, d_recall, ctypes.addressof(cfg), out["counts"], out["dist_sum"],
                            out["valid"], out["thresholds"], out["num_scores"], out["events_type"], out["events_row"],
                            out["status"], ws, ws.numel(), _lib.stream_of(rec))
    return out
