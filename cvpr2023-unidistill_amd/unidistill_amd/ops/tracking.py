"""Multi-object tracking of the evaluator's prediction rows (csrc/track.hip): CenterPoint's greedy,
velocity-compensated centre association, every scene of a validation run in one launch.

``scene_frames`` is the host half: it groups the samples by scene and orders each scene's frames by time (numpy over a few
thousand integers).  ``track_scenes`` is the device half: one workgroup per scene walks the scene's frames in order and writes
one track id per candidate row.  The algorithm is stated in include/unidistill_hip.h and restated in
tests/tracking_reference.py; ids and hits agree with that restatement exactly.

Two deliberate differences from CenterPoint's ``pub_tracker.py``:
  * a track coasts by the current frame's ``dt``, not by the ``dt`` of the frame that last saw it;
  * candidates are explicitly ordered by descending score (equal scores by row), and equal distances go to the lowest slot.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .nus_eval import MAX_BOXES, MAX_CLASSES, PRED_COLS

MAX_AGE = 8               # UD_TRACK_MAX_AGE
ST_NONFINITE, ST_COUNT, ST_RANGE = 1, 2, 4


class Cfg(ctypes.Structure):
    """UdTrackCfg of include/unidistill_hip.h."""
    _fields_ = [("num_classes", ctypes.c_int), ("max_age", ctypes.c_int), ("num_rows", ctypes.c_int64),
                ("num_samples", ctypes.c_int64), ("num_frames", ctypes.c_int64), ("num_scenes", ctypes.c_int64),
                ("score_threshold", ctypes.c_double), ("max_dist", ctypes.c_double * MAX_CLASSES),
                ("track_class", ctypes.c_uint8 * (MAX_CLASSES + 1))]


def status_text(bits):
    out = []
    if bits & ST_NONFINITE:
        out.append("a row of a tracked class has a non-finite translation, velocity or score")
    if bits & ST_COUNT:
        out.append(f"a frame has more than {MAX_BOXES} rows")
    if bits & ST_RANGE:
        out.append("a frame's sample, a sample's rows or a scene's frames lie outside the inputs")
    return "; ".join(out)


def scene_frames(scene, timestamp_us):
    """Host grouping and ordering.  scene [S] (any integers), timestamp_us [S] (int64 microseconds) per sample ->
    (frame_sample int64 [S]: the sample of every frame, scene after scene in ascending scene value, a scene's frames by
    (timestamp_us, sample index); scene_off int64 [NS + 1]; frame_dt float64 [S]: (ts - ts_prev) * 1e-6 within a scene, 0 for
    its first frame)."""
    scene = np.asarray(scene, dtype=np.int64).reshape(-1)
    ts = np.asarray(timestamp_us, dtype=np.int64).reshape(-1)
    if len(scene) != len(ts):
        raise ValueError(f"{len(scene)} scene values for {len(ts)} timestamps")
    frame_sample = np.lexsort((np.arange(len(scene)), ts, scene)).astype(np.int64)
    s_sorted, t_sorted = scene[frame_sample], ts[frame_sample]
    first = np.ones(len(scene), dtype=bool)
    first[1:] = s_sorted[1:] != s_sorted[:-1]
    scene_off = np.append(np.nonzero(first)[0], len(scene)).astype(np.int64)
    frame_dt = np.zeros(len(scene), dtype=np.float64)
    if len(scene) > 1:
        frame_dt[1:] = (t_sorted[1:] - t_sorted[:-1]).astype(np.float64) * 1e-6
    frame_dt[first] = 0.0
    return frame_sample, scene_off, frame_dt


def _index_array(x, name, dev):
    """An int64 index array given on the host (checked by the caller, uploaded here) or already on the device (the kernel's own
    range checks report through the status word) -> (device tensor, host array or None)."""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        if x.dtype != torch.int64 or x.dim() != 1:
            raise ValueError(f"track_scenes: {name} on the device must be int64 [n], got {x.dtype} {tuple(x.shape)}")
        return x.contiguous(), None
    host = np.array(x.numpy() if isinstance(x, torch.Tensor) else x, dtype=np.int64).reshape(-1)      # a copy: may be read-only
    return torch.from_numpy(host).to(dev), host


def track_scenes(rec, cls, row_start, row_count, frame_sample, scene_off, frame_dt, *, track_class, max_dist, max_age=3,
                 score_threshold=0.0, out=None):
    """rec f64 [P, 10] and cls i32 [P] on the device (the evaluator's rows); row_start / row_count [S] per sample; frame_sample
    [F], scene_off [NS + 1], frame_dt [F] as ``scene_frames`` returns them -> (track_id i32 [P], track_hits i32 [P], status
    i32 [1]) on the device.  track_class: a bool per class, max_dist: metres per class.  No host read: the layout arrays are
    checked here when they are given on the host (numpy, lists, CPU tensors) and uploaded; given as device tensors they are
    checked by the kernel, which reports through ``status`` (``status_text``).  ``out``: (track_id, track_hits) to write into."""
    _lib.require_gpu(rec, cls)
    dev = rec.device
    if rec.dtype != torch.float64 or rec.dim() != 2 or rec.shape[1] != PRED_COLS:
        raise ValueError(f"track_scenes: rec must be float64 [P, {PRED_COLS}], got {rec.dtype} {tuple(rec.shape)}")
    P = int(rec.shape[0])
    if cls.dtype != torch.int32 or tuple(cls.shape) != (P,):
        raise ValueError(f"track_scenes: cls must be int32 [{P}], got {cls.dtype} {tuple(cls.shape)}")
    track_class = [bool(v) for v in track_class]
    max_dist = [float(v) for v in max_dist]
    C, max_age, score_threshold = len(track_class), int(max_age), float(score_threshold)
    if not 1 <= C <= MAX_CLASSES or len(max_dist) != C:
        raise ValueError(f"track_scenes: 1 .. {MAX_CLASSES} classes with one max_dist each, got {C} and {len(max_dist)}")
    if not 1 <= max_age <= MAX_AGE:
        raise ValueError(f"track_scenes: max_age must be in 1 .. {MAX_AGE}, got {max_age}")
    if score_threshold != score_threshold or any(t and not d >= 0.0 for t, d in zip(track_class, max_dist)):
        raise ValueError("track_scenes: score_threshold must not be NaN and max_dist of a tracked class not NaN or negative")
    row_start, h_start = _index_array(row_start, "row_start", dev)
    row_count, h_count = _index_array(row_count, "row_count", dev)
    frame_sample, h_frames = _index_array(frame_sample, "frame_sample", dev)
    scene_off, h_off = _index_array(scene_off, "scene_off", dev)
    S, F, NS = int(row_start.shape[0]), int(frame_sample.shape[0]), int(scene_off.shape[0]) - 1
    if row_count.shape[0] != S or S < 1 or NS < 1:
        raise ValueError(f"track_scenes: {S} row_start and {int(row_count.shape[0])} row_count entries, {NS} scenes")
    if h_count is not None and (h_count.max() > MAX_BOXES or h_count.min() < 0):
        raise ValueError(f"track_scenes: a frame has {int(h_count.max())} rows, more than {MAX_BOXES} (or a negative count)")
    if h_start is not None and h_count is not None and ((h_start < 0) | (h_start + h_count > P)).any():
        raise ValueError(f"track_scenes: a sample's rows lie outside the {P} prediction rows")
    if h_frames is not None and F and (h_frames.min() < 0 or h_frames.max() >= S):
        raise ValueError(f"track_scenes: frame_sample outside 0 .. {S - 1}")
    if h_off is not None and (h_off[0] != 0 or h_off[-1] != F or (np.diff(h_off) < 0).any()):
        raise ValueError(f"track_scenes: scene_off must ascend from 0 to the {F} frames")
    if isinstance(frame_dt, torch.Tensor) and frame_dt.is_cuda:
        frame_dt = frame_dt.contiguous()
    else:
        frame_dt = torch.from_numpy(np.array(frame_dt, dtype=np.float64).reshape(-1)).to(dev)
    if frame_dt.dtype != torch.float64 or tuple(frame_dt.shape) != (F,):
        raise ValueError(f"track_scenes: frame_dt must be float64 [{F}], got {frame_dt.dtype} {tuple(frame_dt.shape)}")
    if out is None:
        out = (torch.empty((P,), dtype=torch.int32, device=dev), torch.empty((P,), dtype=torch.int32, device=dev))
    track_id, track_hits = out
    _lib.require_gpu(track_id, track_hits)
    for t in (track_id, track_hits):
        if t.dtype != torch.int32 or tuple(t.shape) != (P,) or not t.is_contiguous():
            raise ValueError(f"track_scenes: out must be two contiguous int32 [{P}] tensors")
    cfg = Cfg(num_classes=C, max_age=max_age, num_rows=P, num_samples=S, num_frames=F, num_scenes=NS,
              score_threshold=score_threshold)
    for c in range(C):
        cfg.max_dist[c] = max_dist[c]
        cfg.track_class[c] = 1 if track_class[c] else 0
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    nbytes = _lib.load().ud_track_workspace_bytes(NS, max_age)
    if nbytes == 0:
        raise ValueError(f"track_scenes: {NS} scenes / max_age {max_age} are outside the supported sizes")
    ws = _lib.workspace(dev, nbytes, slot="track")
    _lib.ud.ud_track_scenes(rec.contiguous(), cls.contiguous(), row_start, row_count, frame_sample, scene_off, frame_dt,
                            ctypes.addressof(cfg), track_id, track_hits, status, ws, ws.numel(), _lib.stream_of(rec))
    return track_id, track_hits, status
