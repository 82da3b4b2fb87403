"""The nuScenes tracking metric on the device (csrc/track_metric.hip): the counts behind AMOTA, AMOTP, MOTA, IDS
and the other figures of the devkit's TrackingEval, for every (class, recall threshold) at once.

``evaluate_tracks`` is the whole evaluation in one enqueue without a host wait: kept flags and track mean scores, the all-boxes
pass, the recall thresholds, the threshold passes and the sums over the scenes.  The host half here orders the frames
(``tracking.scene_frames``), numbers the GT instances densely per (scene, class) and checks the caps before anything is
launched.  The algorithm is stated in include/unidistill_hip.h and restated in tests/track_metric_reference.py.

``interpolate_tracks`` (csrc/track_interp.hip) is the devkit's linear interpolation of predicted and ground-truth
tracks across missed frames -- a count call, one read of the counts, a fill call -- and ``evaluate_tracks_interpolated`` scores
its rows with ``evaluate_tracks``; tests/track_interp_reference.py restates both."""
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
                    events_pass=None, _prepared=None):
    """Device: rec f64 [P, 10], cls i32 [P], track_id i32 [P] (the evaluator's rows and the tracker's ids); gt_xyz f64 [G, 3],
    gt_cls i32 [G], gt_num_pts i32 [G], gt_keep u8 [G] (GT rows sorted by sample); ego f64 [S, 3].  Host: row_start / row_count
    [S], gt_instance int64 [G], gt_off [S + 1], scene / timestamp_us [S], recall [K].  track_class: a bool per class;
    class_range: metres per class.  events_pass: None, "none" (the all-boxes pass) or a threshold index.
    -> dict of device tensors: counts i64 [T, K + 1, 12] (``COUNTS``; T = tracked classes in class order, entry 0 of the second
    axis = all boxes), dist_sum f64 / valid i32 [T, K + 1], thresholds f64 [T, K], num_scores i64 [T], status i32 [1]
    (``status_text``), events_type / events_row i32 [G] or None; plus "classes": the class index of each of the T slots.
    Nothing is read back here.  ``_prepared`` (``evaluate_tracks_interpolated``): the ground truth's instance numbers already on
    the device, (gt_inst i32 [G], the bound of those numbers, GT rows per class, the largest track id) -- gt_instance is not read."""
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
    scene_rows = np.add.reduceat(h_count[frame_sample], scene_off[:-1])
    max_id = int(scene_rows.max())
    if _prepared is None:
        h_inst = _host_i64(gt_instance, G, "gt_instance")
        h_gcls = gt_cls.cpu().numpy() if G else np.zeros(0, np.int32)      # GT comes from the host: this is no result read
        if G and (h_gcls.min() < 0 or h_gcls.max() >= C):
            raise ValueError(f"evaluate_tracks: ground-truth class id outside 0 .. {C - 1}")
        gt_sample = np.repeat(np.arange(S), g_count)
        dense, max_inst = dense_instances(h_inst, h_gcls, gt_sample, h_scene)
        per_class = np.bincount(h_gcls, minlength=C)
    else:
        dense, max_inst, per_class, max_id = _prepared
    if max_inst > MAX_INSTANCES:
        raise ValueError(f"evaluate_tracks: {max_inst} ground-truth instances in one (scene, class), more than {MAX_INSTANCES}")

    cfg = Cfg(num_classes=C, num_thresholds=K, max_boxes_per_sample=int(max_boxes_per_sample), events_pass=ev,
              max_frame_rows=frame_rows, max_instances=max_inst, num_rows=P, num_gt=G, num_samples=S, num_frames=S,
              num_scenes=NS, max_scene_rows=max_id, dist_th_tp=float(dist_th_tp))
    for c in range(C):
        cfg.class_range[c] = class_range[c]
        cfg.class_gt[c] = int(per_class[c])
        cfg.track_class[c] = 1 if track_class[c] else 0
    slots = [c for c in range(C) if track_class[c]]
    T = len(slots)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_start, d_count, d_off = up(h_start), up(h_count), up(h_off)
    d_inst = dense if _prepared is not None else up(dense)
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


# ---- interpolation of tracks across missed frames (csrc/track_interp.hip) ---------------------------------------------
MAX_GT_KEYS = 4096        # UD_TI_MAX_GT_KEYS
MODES = {"devkit": 0, "linear": 1}
TI_NONFINITE, TI_BOXES, TI_RANGE, TI_KEY, TI_DUPLICATE = 1, 2, 4, 8, 16


class InterpCfg(ctypes.Structure):
    """UdTrackInterpCfg of include/unidistill_hip.h."""
    _fields_ = [("num_classes", ctypes.c_int), ("mode", ctypes.c_int), ("max_boxes_per_sample", ctypes.c_int),
                ("max_frame_rows", ctypes.c_int), ("num_rows", ctypes.c_int64), ("num_gt", ctypes.c_int64),
                ("num_samples", ctypes.c_int64), ("num_frames", ctypes.c_int64), ("num_scenes", ctypes.c_int64),
                ("max_scene_rows", ctypes.c_int64), ("max_gt_keys", ctypes.c_int64), ("num_out_pred", ctypes.c_int64),
                ("num_out_gt", ctypes.c_int64), ("class_range", ctypes.c_double * MAX_CLASSES),
                ("track_class", ctypes.c_uint8 * (MAX_CLASSES + 1))]


def interp_status_text(bits):
    out = []
    if bits & TI_NONFINITE:
        out.append("a row of a tracked class has a non-finite value")
    if bits & TI_BOXES:
        out.append("a sample has more kept predictions than max_boxes_per_sample")
    if bits & TI_RANGE:
        out.append("a frame's sample, a sample's rows, a scene's frames or the output layout do not fit the inputs")
    if bits & TI_KEY:
        out.append("a track id exceeds the number of prediction rows of its scene")
    if bits & TI_DUPLICATE:
        out.append("a track id or a ground-truth instance appears twice in one sample")
    return "; ".join(out)


def scene_keys(gt_instance, gt_sample, scene):
    """Host: instance ids (any int64, unique per object) -> (int32 numbers dense within each scene, the largest count of one
    scene)."""
    inst = np.asarray(gt_instance, dtype=np.int64).reshape(-1)
    if not len(inst):
        return np.zeros(0, np.int32), 0
    sc = np.asarray(scene, dtype=np.int64).reshape(-1)[np.asarray(gt_sample, dtype=np.int64).reshape(-1)]
    keys, inverse = np.unique(np.stack([sc, inst], 1), axis=0, return_inverse=True)
    first = np.ones(len(keys), dtype=bool)
    first[1:] = keys[1:, 0] != keys[:-1, 0]
    start = np.maximum.accumulate(np.where(first, np.arange(len(keys)), 0))
    dense = (np.arange(len(keys)) - start).astype(np.int32)
    return dense[inverse.reshape(-1)], int(dense.max()) + 1


def interpolate_tracks(rec, cls, track_id, row_start, row_count, gt_xyz, gt_cls, gt_num_pts, gt_keep, gt_instance, gt_off, ego,
                       scene, timestamp_us, *, track_class, class_range, mode="devkit", max_boxes_per_sample=500):
    """The devkit's linear interpolation of every predicted and every ground-truth track across the frames that miss it, on the
    device; the inputs are those of ``evaluate_tracks``.  mode: "devkit" (the weight from the right timestamp, as the devkit is
    recalled to compute it) or "linear".
    -> dict: "pred" {rec f64 [P', 10], cls, key (the track id), src_row i32 [P'] (the original row, -1: interpolated)} and "gt"
    {xyz f64 [G', 3], cls, key (dense within the scene), src_row i32 [G']} on the device, each with start / count (host int64
    [S]) and num_interpolated; "gt_class_rows" (host int64 per class), "max_gt_keys", "max_id", "status" i32 [1] of the fill
    call on the device (``interp_status_text``).  Only kept rows are in the output, in their order, each sample's interpolated
    rows after them in ascending key.
    The counts of the two sides are read back in ONE copy between the count call and the fill call: the output's size depends on
    the data.  That is the only host wait; it also brings the count call's status, and a non-zero status raises ValueError."""
    _lib.require_gpu(rec, cls, track_id, gt_xyz, gt_cls, gt_num_pts, gt_keep, ego)
    dev = rec.device
    if rec.dtype != torch.float64 or rec.dim() != 2 or rec.shape[1] != PRED_COLS:
        raise ValueError(f"interpolate_tracks: rec must be float64 [P, {PRED_COLS}], got {rec.dtype} {tuple(rec.shape)}")
    P = int(rec.shape[0])
    for t, name in ((cls, "cls"), (track_id, "track_id")):
        if t.dtype != torch.int32 or tuple(t.shape) != (P,):
            raise ValueError(f"interpolate_tracks: {name} must be int32 [{P}], got {t.dtype} {tuple(t.shape)}")
    if gt_xyz.dtype != torch.float64 or gt_xyz.dim() != 2 or gt_xyz.shape[1] != 3:
        raise ValueError(f"interpolate_tracks: gt_xyz must be float64 [G, 3], got {gt_xyz.dtype} {tuple(gt_xyz.shape)}")
    G = int(gt_xyz.shape[0])
    for t, name, dt in ((gt_cls, "gt_cls", torch.int32), (gt_num_pts, "gt_num_pts", torch.int32), (gt_keep, "gt_keep", torch.uint8)):
        if t.dtype != dt or tuple(t.shape) != (G,):
            raise ValueError(f"interpolate_tracks: {name} must be {dt} [{G}], got {t.dtype} {tuple(t.shape)}")
    if ego.dtype != torch.float64 or ego.dim() != 2 or ego.shape[1] != 3 or ego.shape[0] < 1:
        raise ValueError(f"interpolate_tracks: ego must be float64 [S, 3], got {ego.dtype} {tuple(ego.shape)}")
    S = int(ego.shape[0])
    track_class = [bool(v) for v in track_class]
    class_range = [float(v) for v in class_range]
    C = len(track_class)
    if not 1 <= C <= MAX_CLASSES or len(class_range) != C or not any(track_class):
        raise ValueError(f"interpolate_tracks: 1 .. {MAX_CLASSES} classes with one range each and at least one tracked, got {C} "
                         f"and {len(class_range)}")
    if any(t and not r >= 0.0 for t, r in zip(track_class, class_range)):
        raise ValueError("interpolate_tracks: the range of a tracked class must not be NaN or negative")
    if mode not in MODES:
        raise ValueError(f"interpolate_tracks: mode must be one of {sorted(MODES)}, got {mode!r}")
    if int(max_boxes_per_sample) < 1:
        raise ValueError("interpolate_tracks: max_boxes_per_sample must be at least 1")
    h_start, h_count = _host_i64(row_start, S, "row_start"), _host_i64(row_count, S, "row_count")
    h_off = _host_i64(gt_off, S + 1, "gt_off")
    h_inst = _host_i64(gt_instance, G, "gt_instance")
    h_scene, h_ts = _host_i64(scene, S, "scene"), _host_i64(timestamp_us, S, "timestamp_us")
    if h_count.min() < 0 or (h_start < 0).any() or (h_start + h_count > P).any():
        raise ValueError(f"interpolate_tracks: a sample's rows lie outside the {P} prediction rows")
    if h_off[0] != 0 or h_off[-1] != G or (np.diff(h_off) < 0).any():
        raise ValueError(f"interpolate_tracks: gt_off must ascend from 0 to the {G} ground-truth rows")
    g_count = np.diff(h_off)
    frame_rows = int(max(h_count.max(), g_count.max()))
    if frame_rows > MAX_FRAME_ROWS:
        raise ValueError(f"interpolate_tracks: a sample has {frame_rows} prediction or ground-truth rows, more than {MAX_FRAME_ROWS}")
    frame_sample, scene_off, _ = scene_frames(h_scene, h_ts)
    NS = len(scene_off) - 1
    frame_ts = h_ts[frame_sample]
    same = np.nonzero((frame_ts[1:] == frame_ts[:-1]) & (h_scene[frame_sample][1:] == h_scene[frame_sample][:-1]))[0]
    if len(same):
        raise ValueError(f"interpolate_tracks: samples {int(frame_sample[same[0]])} and {int(frame_sample[same[0] + 1])} of one "
                         "scene have the same timestamp")
    keys, max_keys = scene_keys(h_inst, np.repeat(np.arange(S), g_count), h_scene)
    if max_keys > MAX_GT_KEYS:
        raise ValueError(f"interpolate_tracks: {max_keys} ground-truth instances in one scene, more than {MAX_GT_KEYS}")
    max_id = int(np.add.reduceat(h_count[frame_sample], scene_off[:-1]).max())

    cfg = InterpCfg(num_classes=C, mode=MODES[mode], max_boxes_per_sample=int(max_boxes_per_sample), max_frame_rows=frame_rows,
                    num_rows=P, num_gt=G, num_samples=S, num_frames=S, num_scenes=NS, max_scene_rows=max_id,
                    max_gt_keys=max_keys, num_out_pred=0, num_out_gt=0)
    for c in range(C):
        cfg.class_range[c] = class_range[c]
        cfg.track_class[c] = 1 if track_class[c] else 0
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lib = _lib.load()
    nbytes = lib.ud_track_interp_workspace_bytes(ctypes.addressof(cfg))
    if nbytes == 0:
        raise ValueError("interpolate_tracks: the sizes are outside the supported range")
    ws = _lib.workspace(dev, nbytes, slot="track_interp")
    inputs = (rec.contiguous(), cls.contiguous(), track_id.contiguous(), up(h_start), up(h_count), gt_xyz.contiguous(),
              gt_cls.contiguous(), gt_num_pts.contiguous(), gt_keep.contiguous(), up(keys), up(h_off), ego.contiguous(),
              up(frame_sample), up(scene_off), up(frame_ts))
    # the counts and, in the low half of the last entry, the count call's status: one buffer, one copy
    counts = torch.zeros((2 * S + 2 + MAX_CLASSES + 1,), dtype=torch.int64, device=dev)
    _lib.ud.ud_track_interp_count(*inputs, ctypes.addressof(cfg), counts, counts[-1:].view(torch.int32), ws, ws.numel(),
                                  _lib.stream_of(rec))
    h = counts.cpu().numpy()                               # the host wait
    status = int(h[-1] & 0xFFFFFFFF)
    if status:
        raise ValueError(f"interpolate_tracks: {interp_status_text(status)}")
    p_count, g_out = h[:S].copy(), h[S:2 * S].copy()
    for name, n in (("prediction", p_count), ("ground-truth", g_out)):
        if n.max() > MAX_FRAME_ROWS:
            raise ValueError(f"interpolate_tracks: sample {int(n.argmax())} has {int(n.max())} {name} rows after interpolation, "
                             f"more than {MAX_FRAME_ROWS}")
    p_start, g_start = np.cumsum(p_count) - p_count, np.cumsum(g_out) - g_out
    P2, G2 = int(p_count.sum()), int(g_out.sum())
    cfg.num_out_pred, cfg.num_out_gt = P2, G2
    nbytes = lib.ud_track_interp_workspace_bytes(ctypes.addressof(cfg))
    if nbytes == 0:
        raise ValueError("interpolate_tracks: the output sizes are outside the supported range")
    ws = _lib.workspace(dev, nbytes, slot="track_interp")
    # ids stay what the tracker gave: up to max_id, which the metric bounds by its row count -- hence at least that many rows
    PA = max(P2, max_id)
    o_rec = torch.empty((PA, PRED_COLS), dtype=torch.float64, device=dev)
    o_pcls, o_pkey, o_psrc = (torch.empty((PA,), dtype=torch.int32, device=dev) for _ in range(3))
    o_xyz = torch.empty((G2, 3), dtype=torch.float64, device=dev)
    o_gcls, o_gkey, o_gsrc = (torch.empty((G2,), dtype=torch.int32, device=dev) for _ in range(3))
    st = torch.zeros((1,), dtype=torch.int32, device=dev)
    _lib.ud.ud_track_interp_fill(*inputs, ctypes.addressof(cfg), up(p_start), up(p_count), up(g_start), up(g_out), o_rec, o_pcls,
                                 o_pkey, o_psrc, o_xyz, o_gcls, o_gkey, o_gsrc, st, ws, ws.numel(), _lib.stream_of(rec))
    return {"pred": {"rec": o_rec[:P2], "cls": o_pcls[:P2], "key": o_pkey[:P2], "src_row": o_psrc[:P2], "start": p_start,
                     "count": p_count, "num_interpolated": int(h[2 * S])},
            "gt": {"xyz": o_xyz, "cls": o_gcls, "key": o_gkey, "src_row": o_gsrc, "start": g_start, "count": g_out,
                   "num_interpolated": int(h[2 * S + 1])},
            "gt_class_rows": h[2 * S + 2:2 * S + 2 + C].copy(), "max_gt_keys": max_keys, "max_id": max_id, "status": st,
            "_padded": (o_rec, o_pcls, o_pkey)}


def evaluate_tracks_interpolated(rec, cls, track_id, row_start, row_count, gt_xyz, gt_cls, gt_num_pts, gt_keep, gt_instance,
                                 gt_off, ego, scene, timestamp_us, *, track_class, class_range, recall, dist_th_tp=2.0,
                                 max_boxes_per_sample=500, events_pass=None, mode="devkit"):
    """``interpolate_tracks`` on both sides, then ``evaluate_tracks`` on the result with nothing filtered a second time, as the
    devkit scores what its load step left: every output row counts as kept (gt_keep = gt_num_pts = 1, an infinite class range),
    max_boxes_per_sample -- tested by the interpolation on the kept rows -- is raised to the fullest new sample.
    -> the dict of ``evaluate_tracks`` (events_type / events_row refer to the NEW rows) plus "pred_src_row" / "gt_src_row"
    (device i32: new row -> original row or -1), "num_interpolated_pred" / "num_interpolated_gt", "interp_status" (device i32
    [1], ``interp_status_text``) and "interpolated" (the dict of ``interpolate_tracks``)."""
    it = interpolate_tracks(rec, cls, track_id, row_start, row_count, gt_xyz, gt_cls, gt_num_pts, gt_keep, gt_instance, gt_off,
                            ego, scene, timestamp_us, track_class=track_class, class_range=class_range, mode=mode,
                            max_boxes_per_sample=max_boxes_per_sample)
    p, g = it["pred"], it["gt"]
    G2 = int(g["xyz"].shape[0])
    o_rec, o_cls, o_key = it["_padded"]
    ones = torch.ones((G2,), dtype=torch.int32, device=rec.device)
    off = np.concatenate([[0], np.cumsum(g["count"])]).astype(np.int64)
    wide = [float("inf") if t else float(r) for t, r in zip(track_class, class_range)]
    out = evaluate_tracks(o_rec, o_cls, o_key, p["start"], p["count"], g["xyz"], g["cls"], ones, ones.to(torch.uint8), None, off,
                          ego, scene, timestamp_us, track_class=track_class, class_range=wide, recall=recall,
                          dist_th_tp=dist_th_tp, max_boxes_per_sample=max(int(max_boxes_per_sample), int(p["count"].max())),
                          events_pass=events_pass,
                          _prepared=(g["key"], it["max_gt_keys"], it["gt_class_rows"], it["max_id"]))
    out.update(pred_src_row=p["src_row"], gt_src_row=g["src_row"], num_interpolated_pred=p["num_interpolated"],
               num_interpolated_gt=g["num_interpolated"], interp_status=it["status"], interpolated=it)
    return out
