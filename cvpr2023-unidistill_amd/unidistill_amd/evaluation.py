"""nuScenes detection metric (mAP, TP errors, NDS) without the devkit, on the GPU.

The reference's validation_epoch_end -> NuscenesMultiModalData.evaluation -> generate_submission_results +
get_evaluation_results (data/multisensorfusion/nuscenes_multimodal.py:336-393, eval_utils.py) ends in the devkit's
DetectionEval with the ``detection_cvpr_2019`` config.  Here the predictions stay on the device: ``add_batch`` converts
each batch's ``pred_dicts`` to the global frame with one kernel, and ``compute`` runs the matching, the global score
order and the curves (csrc/nus_eval.hip), copies back the per-class curves and reduces them to the devkit's
``metrics_summary`` in numpy.  tests/nus_eval_reference.py restates the devkit; the kernels match it.

Differences from the devkit, by design:
  * Bike-rack filtering needs the map and is not ported: ``add_ground_truth(keep=...)`` takes the caller's mask instead.
  * Predictions of equal score are ordered as ``np.argsort(conf, kind="stable")[::-1]`` orders them over the list in
    (sample, box) order: a later sample first, and within a sample a later box first.  The devkit sorts with numpy's
    unstable default over a sample order that depends on a multiprocessing queue, so its order on exact ties is not
    reproducible.
  * Centre distances are sqrt(dx * dx + dy * dy) evaluated without fused multiply-adds.
"""
import json
import time

import numpy as np
import torch

from . import config
from .ops import nus_eval as K

CLASS_NAMES = list(config.CLASS_NAMES)
ATTRIBUTE_NAMES = ["cycle.with_rider", "cycle.without_rider", "pedestrian.moving", "pedestrian.sitting_lying_down",
                   "pedestrian.standing", "vehicle.moving", "vehicle.parked", "vehicle.stopped"]
TP_METRICS = ["trans_err", "scale_err", "orient_err", "vel_err", "attr_err"]
DEFAULT_ATTRIBUTE = {"car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked",
                     "truck": "vehicle.parked", "bus": "vehicle.moving", "motorcycle": "cycle.without_rider",
                     "construction_vehicle": "vehicle.parked", "bicycle": "cycle.without_rider", "barrier": "",
                     "traffic_cone": ""}
DETECTION_CVPR_2019 = {
    "class_range": {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40,
                    "motorcycle": 40, "bicycle": 40, "traffic_cone": 30, "barrier": 30},
    "dist_fcn": "center_distance",
    "dist_ths": [0.5, 1.0, 2.0, 4.0],
    "dist_th_tp": 2.0,
    "min_recall": 0.1,
    "min_precision": 0.1,
    "max_boxes_per_sample": 500,
    "mean_ap_weight": 5,
}
# The nuScenes tracking classes and CenterPoint's per-class association radius in metres (NuScenesTracker).
TRACKING_NAMES = ["bicycle", "bus", "car", "motorcycle", "pedestrian", "trailer", "truck"]
TRACKING_MAX_DIST = {"car": 4.0, "truck": 4.0, "bus": 5.5, "trailer": 3.0, "pedestrian": 1.0, "motorcycle": 13.0,
                     "bicycle": 3.0}
# The devkit's tracking_nips_2019 config as NuScenesTrackingEval reads it.
TRACKING_NIPS_2019 = {
    "tracking_names": TRACKING_NAMES,
    "class_range": {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "pedestrian": 40, "motorcycle": 40, "bicycle": 40},
    "dist_fcn": "center_distance",
    "dist_th_tp": 2.0,
    "min_recall": 0.1,
    "num_thresholds": 40,
    "max_boxes_per_sample": 500,
    "frame_period_s": 0.5,
    "metric_worst": {"amota": 0.0, "amotp": 2.0, "recall": 0.0, "motar": 0.0, "gt": -1, "mota": 0.0, "motp": 2.0, "mt": 0.0,
                     "ml": -1, "faf": 500, "tp": 0.0, "fp": -1, "fn": -1, "ids": -1, "frag": -1, "tid": 20, "lgd": 20},
}
TRACKING_SUMMED = ("mt", "ml", "tp", "fp", "fn", "ids", "frag", "gt")


def attr_id(name):
    return ATTRIBUTE_NAMES.index(name) if name else -1


def attribute_tables(class_names):
    """Per class the attribute id eval_utils.box3d_to_nuscenesbox assigns above 0.2 m/s and otherwise."""
    moving, still = [], []
    for n in class_names:
        default = DEFAULT_ATTRIBUTE.get(n, "")
        if n in ("car", "construction_vehicle", "bus", "truck", "trailer"):
            moving.append(attr_id("vehicle.moving"))
        elif n in ("bicycle", "motorcycle"):
            moving.append(attr_id("cycle.with_rider"))
        else:
            moving.append(attr_id(default))
        if n == "pedestrian":
            still.append(attr_id("pedestrian.standing"))
        elif n == "bus":
            still.append(attr_id("vehicle.stopped"))
        else:
            still.append(attr_id(default))
    return moving, still


def calc_ap(prec, min_recall, min_precision):
    # The devkit's slice: prec[round(100 * min_recall) + 1:] = prec[11:] for min_recall 0.1, the same first index as
    # calc_tp.  (The feature request wrote prec[12:]; the devkit's code, followed here, starts at 11.)
    p = np.copy(prec)[round(100 * min_recall) + 1:]
    p -= min_precision
    p[p < 0] = 0
    return float(np.mean(p)) / (1.0 - min_precision)


def calc_tp(curve, max_recall_ind, min_recall):
    first = round(100 * min_recall) + 1
    if max_recall_ind < first:
        return 1.0
    return float(np.mean(curve[first: max_recall_ind + 1]))


def max_recall_index(conf):
    nz = np.nonzero(conf)[0]
    return int(nz[-1]) if len(nz) else 0


def summarize(prec, conf, tp_err, class_names, cfg):
    """Per-class curves (prec / conf [C, 4, 101], tp_err [C, 5, 101]) -> the devkit's metrics_summary."""
    ths = list(cfg["dist_ths"])
    ti = ths.index(cfg["dist_th_tp"])
    label_aps, label_tp = {}, {}
    for c, name in enumerate(class_names):
        label_aps[name] = {th: calc_ap(prec[c, w], cfg["min_recall"], cfg["min_precision"]) for w, th in enumerate(ths)}
        mri = max_recall_index(conf[c, ti])
        label_tp[name] = {}
        for m, metric in enumerate(TP_METRICS):
            if name == "traffic_cone" and metric in ("attr_err", "vel_err", "orient_err"):
                label_tp[name][metric] = float("nan")
            elif name == "barrier" and metric in ("attr_err", "vel_err"):
                label_tp[name][metric] = float("nan")
            else:
                label_tp[name][metric] = calc_tp(tp_err[c, m], mri, cfg["min_recall"])
    mean_dist_aps = {n: float(np.mean(list(d.values()))) for n, d in label_aps.items()}
    mean_ap = float(np.mean(list(mean_dist_aps.values())))
    tp_errors = {m: float(np.nanmean([label_tp[n][m] for n in class_names])) for m in TP_METRICS}
    tp_scores = {m: max(0.0, 1.0 - tp_errors[m]) for m in TP_METRICS}
    nd = float(cfg["mean_ap_weight"] * mean_ap + np.sum(list(tp_scores.values())))
    nd /= float(cfg["mean_ap_weight"] + len(tp_scores))
    return {"label_aps": label_aps, "mean_dist_aps": mean_dist_aps, "mean_ap": mean_ap, "label_tp_errors": label_tp,
            "tp_errors": tp_errors, "tp_scores": tp_scores, "nd_score": nd}


def lidar_to_global_from_info(info):
    """global <- LiDAR (float64 [4, 4]) and the ego translation from an info's ``ref_from_car`` / ``car_from_global``."""
    car_from_global = np.asarray(info["car_from_global"], dtype=np.float64)
    ref_from_car = np.asarray(info["ref_from_car"], dtype=np.float64)
    global_from_car = np.linalg.inv(car_from_global)
    return global_from_car @ np.linalg.inv(ref_from_car), global_from_car[:3, 3].copy()


def boxes_to_global(boxes, l2g):
    """LiDAR-frame boxes [n, 7 | 9] (x y z dx dy dz rot [vx vy]) -> (translation [n, 3], wlh [n, 3], yaw [n],
    velocity [n, 2]) in the global frame, with the expressions of k_nus_pred_prep."""
    b = np.asarray(boxes, dtype=np.float64)
    M = np.asarray(l2g, dtype=np.float64)
    x, y, z, rot = b[:, 0], b[:, 1], b[:, 2], b[:, 6]
    t = np.stack([M[r, 0] * x + M[r, 1] * y + M[r, 2] * z + M[r, 3] for r in range(3)], 1)
    wlh = b[:, [4, 3, 5]]
    c, s = np.cos(rot), np.sin(rot)
    yaw = np.arctan2(M[1, 0] * c + M[1, 1] * s, M[0, 0] * c + M[0, 1] * s)
    if b.shape[1] >= 9:
        vel = np.stack([M[0, 0] * b[:, 7] + M[0, 1] * b[:, 8], M[1, 0] * b[:, 7] + M[1, 1] * b[:, 8]], 1)
    else:
        vel = np.full((len(b), 2), np.nan)
    return t, wlh, yaw, vel


def gt_from_infos(infos, class_names=CLASS_NAMES):
    """Keyword arguments of ``add_ground_truth`` from the reference's info dicts (sample i = infos[i]).

    Uses ``gt_boxes`` (LiDAR frame, 9 values; 7 gives NaN velocities), ``gt_names`` (boxes of other names are dropped,
    as the devkit loads only its detection classes), ``num_lidar_pts + num_radar_pts``, ``ref_from_car`` and
    ``car_from_global``.  The infos carry no attribute names, so every attribute is '' (attr_err is then NaN per match
    and 1 per class, unless the caller passes real attribute ids to ``add_ground_truth`` instead)."""
    cols = {k: [] for k in ("translation", "size", "yaw", "velocity", "cls", "attr", "num_pts", "sample")}
    ego = []
    for i, info in enumerate(infos):
        l2g, e = lidar_to_global_from_info(info)
        ego.append(e)
        names = np.asarray(info["gt_names"])
        sel = np.array([n in class_names for n in names], dtype=bool)
        boxes = np.asarray(info["gt_boxes"], dtype=np.float64).reshape(len(names), -1)[sel]
        t, wlh, yaw, vel = boxes_to_global(boxes, l2g) if len(boxes) else (np.zeros((0, 3)),) * 2 + (
            np.zeros(0), np.zeros((0, 2)))
        cols["translation"].append(t)
        cols["size"].append(wlh)
        cols["yaw"].append(yaw)
        cols["velocity"].append(vel)
        cols["cls"].append(np.array([class_names.index(n) for n in names[sel]], dtype=np.int64))
        cols["attr"].append(np.full(int(sel.sum()), -1, dtype=np.int64))
        npts = np.asarray(info["num_lidar_pts"]) + np.asarray(info["num_radar_pts"])
        cols["num_pts"].append(npts[sel].astype(np.int64))
        cols["sample"].append(np.full(int(sel.sum()), i, dtype=np.int64))
    out = {k: np.concatenate(v) for k, v in cols.items()}
    out["ego_translation"] = np.stack(ego) if ego else np.zeros((0, 3))
    return out


class NuScenesDetectionEval:
    """Accumulates the eval forward's ``pred_dicts`` on the device and computes the devkit's ``metrics_summary``.

        ev = NuScenesDetectionEval(device=dev)
        ev.add_ground_truth(**gt_from_infos(val_infos))
        for ids, batch in loader:  ev.add_batch(ids, model(...)["pred_dicts"], lidar_to_global)
        summary = ev.compute()     # rank 0 under torch.distributed; None on the other ranks
    """

    def __init__(self, class_names=CLASS_NAMES, cfg=DETECTION_CVPR_2019, device=None):
        self.class_names = list(class_names)
        self.cfg = dict(cfg)
        C = len(self.class_names)
        if not 1 <= C <= K.MAX_CLASSES:
            raise ValueError(f"1 .. {K.MAX_CLASSES} classes supported, got {C}")
        missing = [n for n in self.class_names if n not in self.cfg["class_range"]]
        if missing:
            raise ValueError(f"cfg['class_range'] has no range for {missing}")
        if self.cfg["dist_th_tp"] not in self.cfg["dist_ths"] or len(self.cfg["dist_ths"]) != 4:
            raise ValueError("cfg needs four dist_ths, dist_th_tp among them")
        if not 0 < self.cfg["max_boxes_per_sample"] <= K.MAX_BOXES:
            raise ValueError(f"max_boxes_per_sample must be in 1 .. {K.MAX_BOXES}")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError("unidistill_amd ops run on the GPU only (no CPU fallback); "
                               f"got device {self.device}")
        self.attr_moving, self.attr_still = attribute_tables(self.class_names)
        self.gt = None
        self.num_samples = 0
        self.reset()

    def reset(self):
        """Drops the accumulated predictions (the ground truth stays)."""
        self._batches = []          # (rec, cls, attr) device tensors per add_batch
        self._meta = []             # per add_batch: [(sample id, box count), ...]
        self._status = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._computed = False      # compute() has run since the last reset
        self._last = None           # rank 0: the rows and (sample, box) layout the last compute() evaluated

    def add_ground_truth(self, translation, size, yaw, velocity, cls, attr, num_pts, sample, ego_translation, keep=None):
        """Global-frame GT boxes: translation [G, 3], size wlh [G, 3], yaw [G], velocity [G, 2] (NaN allowed), class id
        [G], attribute id [G] (-1 = ''), num_pts [G], sample index [G] in 0 .. S-1; ego_translation [S, 3] (global) per
        sample; keep [G] (bool, optional): the caller's filter, e.g. the devkit's bike-rack test, which needs the map
        and is not ported.  Replaces any earlier ground truth."""
        ego = np.asarray(ego_translation, dtype=np.float64).reshape(-1, 3)
        S = len(ego)
        sample = np.asarray(sample, dtype=np.int64).reshape(-1)
        G = len(sample)
        cls = np.asarray(cls, dtype=np.int64).reshape(-1)
        attr = np.asarray(attr, dtype=np.int64).reshape(-1)
        rec = np.concatenate([np.asarray(translation, np.float64).reshape(G, 3), np.asarray(size, np.float64).reshape(G, 3),
                              np.asarray(yaw, np.float64).reshape(G, 1), np.asarray(velocity, np.float64).reshape(G, 2)], 1)
        num_pts = np.asarray(num_pts, dtype=np.int64).reshape(-1)
        keep = np.ones(G, dtype=bool) if keep is None else np.asarray(keep, dtype=bool).reshape(-1)
        if S < 1:
            raise ValueError("ground truth needs at least one sample (ego_translation [S, 3])")
        if not (len(cls) == len(attr) == len(num_pts) == len(keep) == G):
            raise ValueError("ground-truth columns differ in length")
        if G and (sample.min() < 0 or sample.max() >= S):
            raise ValueError(f"ground-truth sample index outside 0 .. {S - 1}")
        if G and (cls.min() < 0 or cls.max() >= len(self.class_names)):
            raise ValueError(f"ground-truth class id outside 0 .. {len(self.class_names) - 1}")
        if G and (attr.min() < -1 or attr.max() >= len(ATTRIBUTE_NAMES)):
            raise ValueError(f"ground-truth attribute id outside -1 .. {len(ATTRIBUTE_NAMES) - 1}")
        order = np.argsort(sample, kind="stable")
        off = np.zeros(S + 1, dtype=np.int64)
        np.cumsum(np.bincount(sample, minlength=S), out=off[1:])
        if G and np.diff(off).max() > K.MAX_BOXES:
            raise ValueError(f"a sample has more than {K.MAX_BOXES} ground-truth boxes")
        d = self.device
        self.gt = {"rec": torch.from_numpy(np.ascontiguousarray(rec[order])).to(d),
                   "cls": torch.from_numpy(cls[order].astype(np.int32)).to(d),
                   "attr": torch.from_numpy(attr[order].astype(np.int32)).to(d),
                   "num_pts": torch.from_numpy(np.clip(num_pts[order], -1, 1 << 30).astype(np.int32)).to(d),
                   "keep": torch.from_numpy(keep[order].astype(np.uint8)).to(d),
                   "off": torch.from_numpy(off).to(d), "ego": torch.from_numpy(ego).to(d)}
        self.gt_order = order        # row r of the device GT = row gt_order[r] of the caller's arrays
        self.num_samples = S

    def add_batch(self, sample_ids, pred_dicts, lidar_to_global):
        """``pred_dicts`` of the eval forward as returned (device tensors; labels start at 1), ``sample_ids`` the host
        sample indices of the batch, ``lidar_to_global`` float64 [B, 4, 4] (calibrated sensor, then ego pose)."""
        ids = [int(i) for i in (sample_ids.tolist() if hasattr(sample_ids, "tolist") else sample_ids)]
        if len(ids) != len(pred_dicts):
            raise ValueError(f"{len(ids)} sample ids for {len(pred_dicts)} pred_dicts")
        if not ids:
            return
        counts = [int(pd["pred_boxes"].shape[0]) for pd in pred_dicts]
        cap = self.cfg["max_boxes_per_sample"]
        for i, n in zip(ids, counts):
            if n > cap:
                raise ValueError(f"sample {i}: {n} predictions, more than max_boxes_per_sample = {cap}")
        ncols = {int(pd["pred_boxes"].shape[1]) for pd in pred_dicts if pd["pred_boxes"].shape[0]}
        if len(ncols) > 1:
            raise ValueError(f"pred_boxes of one batch differ in width: {sorted(ncols)}")
        boxes = torch.cat([pd["pred_boxes"] for pd in pred_dicts]) if sum(counts) else None
        if boxes is None:
            rec = torch.empty((0, K.PRED_COLS), dtype=torch.float64, device=self.device)
            cls = attr = torch.empty((0,), dtype=torch.int32, device=self.device)
        else:
            scores = torch.cat([pd["pred_scores"] for pd in pred_dicts])
            labels = torch.cat([pd["pred_labels"] for pd in pred_dicts])
            rec, cls, attr = K.pred_to_global(boxes, scores, labels, counts, lidar_to_global, self.attr_moving,
                                              self.attr_still, self._status)
        self._batches.append((rec, cls, attr))
        self._meta.append(list(zip(ids, counts)))

    def _gather(self):
        """Every rank's rows and metadata on rank 0 (padded all_gather); (rec, cls, attr, meta) or None off rank 0."""
        import torch.distributed as dist
        rows = sum(r.shape[0] for r, _, _ in self._batches)
        meta = [m for ms in self._meta for m in ms]
        rec, cls, attr = self._local()
        world = dist.get_world_size()
        sizes = [None] * world
        dist.all_gather_object(sizes, (rows, meta))
        pad = max(max(n for n, _ in sizes), 1)

        def padded(t, shape_tail, dtype):
            out = torch.zeros((pad,) + shape_tail, dtype=dtype, device=self.device)
            out[:t.shape[0]] = t
            return out

        parts = [padded(rec, (K.PRED_COLS,), torch.float64), padded(cls, (), torch.int32),
                 padded(attr, (), torch.int32), self._status.clone()]
        host_backend = dist.get_backend() == "gloo"            # gloo moves host buffers: stage through the host
        gathered = []
        for p in parts:
            p = p.cpu() if host_backend else p
            bufs = [torch.empty_like(p) for _ in range(world)]
            dist.all_gather(bufs, p)
            gathered.append([b.to(self.device) for b in bufs])
        if dist.get_rank() != 0:
            return None
        recs = [g[:n] for g, (n, _) in zip(gathered[0], sizes)]
        clss = [g[:n] for g, (n, _) in zip(gathered[1], sizes)]
        attrs = [g[:n] for g, (n, _) in zip(gathered[2], sizes)]
        status = torch.stack(gathered[3]).amax(0)
        return torch.cat(recs), torch.cat(clss), torch.cat(attrs), [m for _, ms in sizes for m in ms], status

    def _local(self):
        if not self._batches:
            e = torch.empty((0,), dtype=torch.int32, device=self.device)
            return torch.empty((0, K.PRED_COLS), dtype=torch.float64, device=self.device), e, e
        return (torch.cat([b[0] for b in self._batches]), torch.cat([b[1] for b in self._batches]),
                torch.cat([b[2] for b in self._batches]))

    def _device_config(self):
        cfg = K.Cfg()
        cfg.num_classes = len(self.class_names)
        ths = list(self.cfg["dist_ths"])
        cfg.dist_th_tp_index = ths.index(self.cfg["dist_th_tp"])
        cfg.pi_period_class = self.class_names.index("barrier") if "barrier" in self.class_names else -1
        for c, n in enumerate(self.class_names):
            cfg.class_range[c] = float(self.cfg["class_range"][n])
        for w, th in enumerate(ths):
            cfg.dist_th[w] = float(th)
        for i, v in enumerate(np.linspace(0, 1, K.POINTS)):
            cfg.rec_pts[i] = float(v)
        return cfg

    def compute_curves(self):
        """Runs the device metric; -> (device outputs of ops.nus_eval.evaluate, pred rows, (sample, box) layout) on
        rank 0, None on the other ranks."""
        import torch.distributed as dist
        if self.gt is None:
            raise RuntimeError("add_ground_truth() first")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            got = self._gather()
            if got is None:
                return None
            rec, cls, attr, meta, status = got
        else:
            rec, cls, attr = self._local()
            meta = [m for ms in self._meta for m in ms]
            status = self._status
        S = self.num_samples
        start = np.full(S, -1, dtype=np.int64)
        count = np.zeros(S, dtype=np.int64)
        row = 0
        for sid, n in meta:          # the first occurrence of a sample wins (DistributedSampler pads with repeats)
            if not 0 <= sid < S:
                raise ValueError(f"prediction sample id {sid} outside the {S} ground-truth samples")
            if start[sid] < 0:
                start[sid], count[sid] = row, n
            row += n
        if (start < 0).any():
            missing = np.nonzero(start < 0)[0]
            raise ValueError(f"samples in the ground truth but not in the predictions: {missing[:10].tolist()}"
                             f"{' ...' if len(missing) > 10 else ''} ({len(missing)} of {S})")
        off = np.zeros(S + 1, dtype=np.int64)
        np.cumsum(count, out=off[1:])
        P = int(off[-1])
        d = self.device
        pred = {"rec": rec, "cls": cls, "attr": attr, "src": torch.from_numpy(np.maximum(start, 0)).to(d),
                "off": torch.from_numpy(off).to(d)}
        out = K.evaluate(self._device_config(), pred, self.gt, S, P)
        out["status"] = out["status"] | status
        layout = {"start": start, "count": count, "off": off}
        return out, pred, layout

    def compute(self):
        """The devkit's metrics_summary (rank 0; None on the other ranks under torch.distributed, where every rank must
        call it: it gathers the predictions to rank 0)."""
        t0 = time.time()
        self._computed, self._last = False, None
        got = self.compute_curves()
        if got is None:
            self._computed = True
            return None
        out, pred, layout = got
        status = int(out["status"].item())
        if status:
            raise ValueError(f"nuScenes eval: {K.status_text(status)}")
        self._computed, self._last = True, (pred, layout)
        prec, conf, tp_err = (out[k].cpu().numpy() for k in ("prec", "conf", "tp_err"))
        summary = summarize(prec, conf, tp_err, self.class_names, self.cfg)
        summary["eval_time"] = time.time() - t0
        summary["cfg"] = dict(self.cfg)
        return summary

    def last_predictions(self):
        """What the last ``compute()`` evaluated, for consumers of the rows (``NuScenesTracker``): (pred, layout) on rank 0 --
        pred["rec"] f64 [rows, 10] and pred["cls"] i32 [rows] on the device, layout["start"] / ["count"] per sample on the host
        -- and None on the other ranks.  Raises if ``compute()`` has not run since the last reset."""
        if not self._computed:
            raise RuntimeError("no evaluated predictions: call compute() first")
        return self._last

    def write_submission(self, path, sample_tokens):
        """The devkit's results JSON (generate_submission_results with meta_type_list ["use_camera", "use_lidar"]):
        sample_tokens[s] names sample s.  ``rotation`` is the yaw-only quaternion [cos(yaw/2), 0, 0, sin(yaw/2)]; the
        detection eval reads only its yaw.  Writes the predictions the last ``compute()`` evaluated, without any
        collective: call it on rank 0 alone or on every rank (the other ranks write nothing and get None)."""
        if not self._computed:
            raise RuntimeError("write_submission() writes what compute() evaluated: call compute() first")
        if self._last is None:
            return None
        pred, layout = self._last
        rec = pred["rec"].cpu().numpy()
        cls = pred["cls"].cpu().numpy()
        attr = pred["attr"].cpu().numpy()
        if len(sample_tokens) != self.num_samples:
            raise ValueError(f"{len(sample_tokens)} sample tokens for {self.num_samples} samples")
        results = {}
        for s, tok in enumerate(sample_tokens):
            boxes = []
            for r in range(layout["start"][s], layout["start"][s] + layout["count"][s]):
                x = rec[r]
                boxes.append({"sample_token": tok, "translation": x[0:3].tolist(), "size": x[3:6].tolist(),
                              "rotation": [float(np.cos(x[6] / 2)), 0.0, 0.0, float(np.sin(x[6] / 2))],
                              "velocity": x[7:9].tolist(), "detection_name": self.class_names[cls[r]],
                              "detection_score": float(x[9]),
                              "attribute_name": ATTRIBUTE_NAMES[attr[r]] if attr[r] >= 0 else ""})
            results[tok] = boxes
        sub = {"meta": {"use_camera": True, "use_lidar": True, "use_radar": False, "use_map": False,
                        "use_external": False}, "results": results}
        with open(path, "w") as f:
            json.dump(sub, f)
        return sub


class NuScenesTracker:
    """CenterPoint's greedy, velocity-compensated centre tracker over the predictions a ``NuScenesDetectionEval`` holds on the
    device (ops/tracking.py): a detector's validation run becomes a nuScenes tracking submission.

        tr = NuScenesTracker()
        ids = tr.track(evaluator, scene, timestamp_us)      # after evaluator.compute(); one launch for all scenes
        tr.write_submission(path, sample_tokens)

    ``max_dist``: {class name: metres}, None = ``TRACKING_MAX_DIST``; a class is tracked iff it has an entry.  Differences from
    CenterPoint's pub_tracker.py, by design: a track coasts by the current frame's dt (not by the dt of the frame that last saw
    it); detections are matched in descending score order (equal scores in row order) and equal distances go to the track
    earlier in the list.  Coasting tracks are not emitted."""

    def __init__(self, class_names=CLASS_NAMES, max_dist=None, max_age=3, score_threshold=0.0):
        from .ops import tracking as T
        self.class_names = list(class_names)
        if max_dist is None:
            max_dist = TRACKING_MAX_DIST
        elif any(n not in self.class_names for n in max_dist):
            raise ValueError(f"max_dist names classes that are not in class_names: "
                             f"{[n for n in max_dist if n not in self.class_names]}")
        self.track_class = [n in max_dist for n in self.class_names]
        self.max_dist = [float(max_dist.get(n, 0.0)) for n in self.class_names]
        self.max_age, self.score_threshold = int(max_age), float(score_threshold)
        if not 1 <= len(self.class_names) <= T.MAX_CLASSES:
            raise ValueError(f"1 .. {T.MAX_CLASSES} classes supported, got {len(self.class_names)}")
        if not 1 <= self.max_age <= T.MAX_AGE:
            raise ValueError(f"max_age must be in 1 .. {T.MAX_AGE}, got {max_age}")
        self._result = None
        self._tracked = False       # track() has run (its result is None off rank 0)

    def track(self, evaluator, scene, timestamp_us):
        """scene [S] (an integer per sample) and timestamp_us [S] (int64) for the evaluator's S samples -> {"track_id",
        "track_hits"}: int32 device tensors aligned with the evaluator's prediction rows (0 = not tracked).  Rank 0 under
        torch.distributed; None on the other ranks, without any collective.  Raises if ``compute()`` has not run, and
        ValueError on a non-zero device status (a non-finite velocity, for instance: 7-value boxes carry none)."""
        from .ops import tracking as T
        self._result, self._tracked = None, False
        last = evaluator.last_predictions()
        if last is None:
            self._tracked = True
            return None
        pred, layout = last
        S = evaluator.num_samples
        scene = np.asarray(scene, dtype=np.int64).reshape(-1)
        if len(scene) != S or len(np.asarray(timestamp_us).reshape(-1)) != S:
            raise ValueError(f"scene and timestamp_us need one entry for each of the {S} samples")
        frame_sample, scene_off, frame_dt = T.scene_frames(scene, timestamp_us)
        ids, hits, status = T.track_scenes(pred["rec"], pred["cls"], layout["start"], layout["count"], frame_sample, scene_off,
                                           frame_dt, track_class=self.track_class, max_dist=self.max_dist,
                                           max_age=self.max_age, score_threshold=self.score_threshold)
        status = int(status.item())
        if status:
            raise ValueError(f"nuScenes tracking: {T.status_text(status)}")
        self._result, self._tracked = (pred, layout, ids, scene), True
        return {"track_id": ids, "track_hits": hits}

    def last_tracks(self):
        """What the last ``track()`` stored, for consumers of the ids (``NuScenesTrackingEval``): (pred, layout, ids, scene) on
        rank 0 -- the evaluator's rows and layout, the int32 ids on the device, the scene per sample -- and None on the other
        ranks.  Raises before ``track()``."""
        if not self._tracked:
            raise RuntimeError("no tracks: call track() first")
        return self._result

    def write_submission(self, path, sample_tokens):
        """The devkit's tracking results JSON of the last ``track()``: per tracked row sample_token, translation, size, rotation
        (the detection file's yaw-only quaternion), velocity, tracking_id "{scene}_{id}", tracking_name, tracking_score (the
        detection score); a sample without a tracked box maps to [].  The other ranks write nothing and get None."""
        if self._result is None:
            return None
        pred, layout, ids, scene = self._result
        if len(sample_tokens) != len(scene):
            raise ValueError(f"{len(sample_tokens)} sample tokens for {len(scene)} samples")
        rec, cls, ids = pred["rec"].cpu().numpy(), pred["cls"].cpu().numpy(), ids.cpu().numpy()
        results = {}
        for s, tok in enumerate(sample_tokens):
            boxes = []
            for r in range(layout["start"][s], layout["start"][s] + layout["count"][s]):
                if ids[r] <= 0:
                    continue
                x = rec[r]
                boxes.append({"sample_token": tok, "translation": x[0:3].tolist(), "size": x[3:6].tolist(),
                              "rotation": [float(np.cos(x[6] / 2)), 0.0, 0.0, float(np.sin(x[6] / 2))],
                              "velocity": x[7:9].tolist(), "tracking_id": f"{int(scene[s])}_{int(ids[r])}",
                              "tracking_name": self.class_names[cls[r]], "tracking_score": float(x[9])})
            results[tok] = boxes
        sub = {"meta": {"use_camera": True, "use_lidar": True, "use_radar": False, "use_map": False,
                        "use_external": False}, "results": results}
        with open(path, "w") as f:
            json.dump(sub, f)
        return sub


def tracking_pass_metrics(counts, dist_sum, valid, recall, frame_period_s):
    """One class: counts int64 [K + 1, 12] (ops.track_metric.COUNTS), dist_sum / valid [K + 1] (entry 0 = all boxes), recall [K]
    -> {metric: float64 [K]} over the threshold passes, NaN where the pass was not run."""
    c = {n: counts[1:, i].astype(np.float64) for i, n in enumerate(("frames", "objects", "matches", "switches", "fp", "miss",
                                                                   "mt", "ml", "frag", "tid", "lgd", "inst"))}
    ok = np.asarray(valid[1:]) != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        P, tp = c["objects"], c["matches"] + c["switches"]
        fp, fn, ids = c["fp"], c["miss"], c["switches"]
        m = {"tp": tp, "fp": fp, "fn": fn, "ids": ids, "gt": P, "recall": tp / P,
             "mota": np.maximum(0.0, 1.0 - (fn + ids + fp) / P),
             "motar": np.where(tp > 0, np.maximum(0.0, 1.0 - (ids + fp + fn - (1.0 - tp / P) * P) / (tp / P * P)), np.nan),
             "motp": np.where(tp > 0, np.asarray(dist_sum[1:], np.float64) / tp, np.nan), "faf": 100.0 * fp / c["frames"],
             "mt": c["mt"], "ml": c["ml"], "frag": c["frag"],
             "tid": np.where(c["inst"] > 0, c["tid"] / c["inst"] * frame_period_s, np.nan),
             "lgd": np.where(c["inst"] > 0, c["lgd"] / c["inst"] * frame_period_s, np.nan)}
    return {k: np.where(ok, v, np.nan) for k, v in m.items()}


def summarize_tracking(curves, names, cfg):
    """``NuScenesTrackingEval.last_curves()`` -> the devkit's tracking summary: per class amota / amotp over the thresholds (NaN
    -> the worst value) and every other metric at the threshold of the best mota; over the classes sums of the counts and means
    of the rest, NaN-aware."""
    worst = cfg["metric_worst"]
    label = {m: {} for m in worst}
    for t, name in enumerate(names):
        pm = tracking_pass_metrics(curves["counts"][t], curves["dist_sum"][t], curves["valid"][t], curves["recall"],
                                   cfg["frame_period_s"])
        if np.all(np.isnan(pm["mota"])):
            for m, w in worst.items():
                label[m][name] = float("nan") if w == -1 else float(w)
            continue
        best = int(np.nanargmax(pm["mota"]))
        label["amota"][name] = float(np.mean(np.where(np.isnan(pm["motar"]), worst["amota"], pm["motar"])))
        label["amotp"][name] = float(np.mean(np.where(np.isnan(pm["motp"]), worst["amotp"], pm["motp"])))
        for m, v in pm.items():
            label[m][name] = float(v[best])
    summary = {"label_metrics": label}
    for m in worst:
        vals = np.array(list(label[m].values()), dtype=np.float64)
        if np.all(np.isnan(vals)):
            summary[m] = float("nan")
        else:
            summary[m] = float(np.nansum(vals)) if m in TRACKING_SUMMED else float(np.nanmean(vals))
    return summary


class NuScenesTrackingEval:
    """The nuScenes tracking metric (AMOTA, AMOTP, MOTA, IDS ...) over the tracks a ``NuScenesTracker`` holds on the device,
    without the devkit (ops/track_metric.py).

        ev = NuScenesTrackingEval(class_names=CLASS_NAMES, cfg=TRACKING_NIPS_2019, device=dev)
        ev.add_ground_truth(translation, cls, instance, num_pts, sample, ego_translation, scene, timestamp_us)
        summary = ev.compute(tracker)     # after tracker.track(evaluator, ...); rank 0, None on the other ranks, no collective

    Classes of ``class_names`` outside cfg["tracking_names"] are ignored.  With ``interpolate=False`` (the default) the tracks
    are scored as given.  ``interpolate=True`` first fills the holes of every predicted and every ground-truth track by linear
    interpolation, as the devkit does between its filters and its metric (ops.track_metric.interpolate_tracks):
    a re-acquired track then no longer costs a MISS and a FRAG per coasted frame, and a ground-truth object that drops to
    ``num_pts == 0`` for a frame stays in the evaluation.  That costs one host wait (the output's size depends on the data).
    ``interpolate_mode``: "devkit" -- the weight from the right timestamp, as the devkit is recalled to compute it (unverified)
    -- or "linear"; they differ only where frames are unevenly spaced or a hole is longer than one frame.  The tracker's rows
    and its submission file are never interpolated (the devkit interpolates when it loads the file).  The devkit's bike-rack
    filter is not ported (``keep`` stands in for it)."""

    def __init__(self, class_names=CLASS_NAMES, cfg=TRACKING_NIPS_2019, device=None, interpolate=False,
                 interpolate_mode="devkit"):
        from .ops import track_metric as M
        self.interpolate = bool(interpolate)
        self.interpolate_mode = str(interpolate_mode)
        if self.interpolate_mode not in M.MODES:
            raise ValueError(f"interpolate_mode must be one of {sorted(M.MODES)}, got {interpolate_mode!r}")
        self.class_names = list(class_names)
        self.cfg = dict(cfg)
        if not 1 <= len(self.class_names) <= M.MAX_CLASSES:
            raise ValueError(f"1 .. {M.MAX_CLASSES} classes supported, got {len(self.class_names)}")
        self.track_class = [n in self.cfg["tracking_names"] for n in self.class_names]
        if not any(self.track_class):
            raise ValueError("none of class_names is in cfg['tracking_names']")
        missing = [n for n, t in zip(self.class_names, self.track_class) if t and n not in self.cfg["class_range"]]
        if missing:
            raise ValueError(f"cfg['class_range'] has no range for {missing}")
        if not 1 <= self.cfg["num_thresholds"] <= M.MAX_THRESHOLDS:
            raise ValueError(f"num_thresholds must be in 1 .. {M.MAX_THRESHOLDS}")
        self.class_range = [float(self.cfg["class_range"].get(n, 0.0)) for n in self.class_names]
        self.recall = np.round(np.linspace(self.cfg["min_recall"], 1.0, self.cfg["num_thresholds"]), 12)
        self.device = _lib_device(device)
        self.gt = None
        self._curves = None

    def add_ground_truth(self, translation, cls, instance, num_pts, sample, ego_translation, scene, timestamp_us, keep=None):
        """Global-frame GT: translation [G, 3], class id [G], instance [G] (int64, unique per object over the split), num_pts
        [G], sample index [G] in 0 .. S-1; per sample ego_translation [S, 3], scene [S], timestamp_us [S]; keep [G] (bool,
        optional): the caller's filter.  Replaces any earlier ground truth."""
        ego = np.asarray(ego_translation, dtype=np.float64).reshape(-1, 3)
        S = len(ego)
        sample = np.asarray(sample, dtype=np.int64).reshape(-1)
        G = len(sample)
        cls = np.asarray(cls, dtype=np.int64).reshape(-1)
        instance = np.asarray(instance, dtype=np.int64).reshape(-1)
        num_pts = np.asarray(num_pts, dtype=np.int64).reshape(-1)
        keep = np.ones(G, dtype=bool) if keep is None else np.asarray(keep, dtype=bool).reshape(-1)
        xyz = np.asarray(translation, dtype=np.float64).reshape(G, 3)
        scene = np.asarray(scene, dtype=np.int64).reshape(-1)
        ts = np.asarray(timestamp_us, dtype=np.int64).reshape(-1)
        if S < 1 or len(scene) != S or len(ts) != S:
            raise ValueError("ground truth needs ego_translation [S, 3], scene [S] and timestamp_us [S] for S >= 1 samples")
        if not (len(cls) == len(instance) == len(num_pts) == len(keep) == G):
            raise ValueError("ground-truth columns differ in length")
        if G and (sample.min() < 0 or sample.max() >= S):
            raise ValueError(f"ground-truth sample index outside 0 .. {S - 1}")
        if G and (cls.min() < 0 or cls.max() >= len(self.class_names)):
            raise ValueError(f"ground-truth class id outside 0 .. {len(self.class_names) - 1}")
        order = np.argsort(sample, kind="stable")
        off = np.zeros(S + 1, dtype=np.int64)
        np.cumsum(np.bincount(sample, minlength=S), out=off[1:])
        d = self.device
        self.gt = {"xyz": torch.from_numpy(np.ascontiguousarray(xyz[order])).to(d),
                   "cls": torch.from_numpy(cls[order].astype(np.int32)).to(d),
                   "num_pts": torch.from_numpy(np.clip(num_pts[order], -1, 1 << 30).astype(np.int32)).to(d),
                   "keep": torch.from_numpy(keep[order].astype(np.uint8)).to(d), "ego": torch.from_numpy(ego).to(d),
                   "instance": instance[order], "off": off, "scene": scene, "timestamp_us": ts}
        self.gt_order = order        # row r of the device GT = row gt_order[r] of the caller's arrays
        self.num_samples = S

    def compute_curves(self, tracker, events_pass=None):
        """Runs the device metric over ``tracker.last_tracks()`` -> the device outputs of ops.track_metric.evaluate_tracks (with
        ``interpolate``: of evaluate_tracks_interpolated, whose events and src_row maps refer to the interpolated rows) on rank
        0, None on the other ranks."""
        from .ops import track_metric as M
        if self.gt is None:
            raise RuntimeError("add_ground_truth() first")
        last = tracker.last_tracks()
        if last is None:
            return None
        pred, layout, ids, scene = last
        g = self.gt
        if len(scene) != self.num_samples or not np.array_equal(np.asarray(scene, np.int64), g["scene"]):
            raise ValueError("the tracker's scene per sample differs from the ground truth's")
        extra = {"mode": self.interpolate_mode} if self.interpolate else {}
        run = M.evaluate_tracks_interpolated if self.interpolate else M.evaluate_tracks
        return run(pred["rec"], pred["cls"], ids, layout["start"], layout["count"], g["xyz"], g["cls"], g["num_pts"], g["keep"],
                   g["instance"], g["off"], g["ego"], g["scene"], g["timestamp_us"], track_class=self.track_class,
                   class_range=self.class_range, recall=self.recall, dist_th_tp=self.cfg["dist_th_tp"],
                   max_boxes_per_sample=self.cfg["max_boxes_per_sample"], events_pass=events_pass, **extra)

    def compute(self, tracker):
        """The tracking summary: summary["label_metrics"][metric][class] and summary[metric], plus eval_time and cfg -- with
        ``interpolate`` also "interpolate": True and "interpolate_mode" -- (rank 0; None on the other ranks, without any
        collective)."""
        from .ops import track_metric as M
        t0 = time.time()
        self._curves = None
        out = self.compute_curves(tracker)
        if out is None:
            return None
        if self.interpolate:                      # both status words in the one read
            status, filled = (int(v) for v in torch.cat([out["status"], out["interp_status"]]).cpu())
            if filled:
                raise ValueError(f"nuScenes tracking eval: {M.interp_status_text(filled)}")
        else:
            status = int(out["status"].item())
        if status:
            raise ValueError(f"nuScenes tracking eval: {M.status_text(status)}")
        self._curves = {k: out[k].cpu().numpy() for k in ("counts", "dist_sum", "valid", "thresholds", "num_scores")}
        self._curves["recall"] = self.recall.copy()
        self._curves["classes"] = [self.class_names[c] for c in out["classes"]]
        summary = summarize_tracking(self._curves, self._curves["classes"], self.cfg)
        if self.interpolate:
            self._curves["num_interpolated_pred"] = out["num_interpolated_pred"]
            self._curves["num_interpolated_gt"] = out["num_interpolated_gt"]
            summary["interpolate"], summary["interpolate_mode"] = True, self.interpolate_mode
        summary["eval_time"] = time.time() - t0
        summary["cfg"] = dict(self.cfg)
        return summary

    def last_curves(self):
        """The per (class, threshold) arrays of the last ``compute()`` on the host: counts [T, K + 1, 12], dist_sum, valid,
        thresholds [T, K], num_scores [T], recall [K], classes (names), with ``interpolate`` also num_interpolated_pred /
        num_interpolated_gt (the interpolated rows of the two sides); None off rank 0."""
        return self._curves


def _lib_device(device):
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if device.type != "cuda":
        raise RuntimeError(f"unidistill_amd ops run on the GPU only (no CPU fallback); got device {device}")
    return device


def depth_figures(terms):
    """The twelve sums of ops.depth_metric (float64 [12]) -> the figures; NaN for every ratio of an empty set, n = 0."""
    t = [float(v) for v in terms]
    n = t[0]
    mean = (lambda v: v / n) if n > 0 else (lambda v: float("nan"))
    root = (lambda v: float(np.sqrt(v / n))) if n > 0 else (lambda v: float("nan"))
    return {"n": int(round(n)), "abs_rel": mean(t[2]), "sq_rel": mean(t[3]), "rmse": root(t[4]), "rmse_log": root(t[5]),
            "mae": mean(t[1]), "d1": mean(t[6]), "d2": mean(t[7]), "d3": mean(t[8]), "bin_acc": mean(t[9]),
            "bin_acc1": mean(t[10]), "nll": mean(t[11])}


class DepthMetric:
    """The camera lift's depth distribution against the LiDAR minimum depth, accumulated on the device.

        m = DepthMetric(d_bound, ncam=6, range_edges=[2, 20, 40, 58], per_camera=True, device=dev)
        for batch in loader:  m.add_batch(depth_logits, dmin)          # or train.ValidationStep(..., depth_metric=m)
        figures = m.compute()          # every rank under torch.distributed (one all_reduce of the state)

    ``logits`` [B * ncam, D, fH, fW] are ``LSSFPN(..., is_return_depth="logits")``'s, ``dmin`` is
    ``LSSFPN.lidar_depth_labels(...)[0]``.  The predicted depth is the softmax's expectation over the bin CENTRES
    d_lo + (j + 0.5) * d_step.  ``range_edges=None`` is the single bucket [d_lo, d_lo + D * d_step); a labelled pixel outside
    every bucket of explicit edges is counted nowhere.  ``compute()`` returns n, abs_rel, sq_rel, rmse, rmse_log, mae, d1, d2,
    d3 (delta < 1.25^k), bin_acc, bin_acc1 (arg-max bin equal to / within one of the label bin) and nll (-ln p of the label
    bin) over everything counted, formed from the summed terms; with explicit edges ``"ranges"``: a list of the same figures
    per bucket (plus ``lo``, ``hi``), with per_camera ``"cameras"``: a list per camera."""

    def __init__(self, d_bound, ncam=1, range_edges=None, per_camera=False, device=None):
        from .ops import depth_metric as op
        self.d_bound = [float(v) for v in d_bound]
        lo, step, D = op.depth_bins(self.d_bound)
        self.explicit_ranges = range_edges is not None
        self.range_edges = [float(v) for v in range_edges] if self.explicit_ranges else [lo, lo + D * step]
        R = len(self.range_edges) - 1
        if not 1 <= R <= op.MAX_RANGES:
            raise ValueError(f"1 .. {op.MAX_RANGES} range buckets supported, got {R}")
        if any(not b > a for a, b in zip(self.range_edges, self.range_edges[1:])):
            raise ValueError(f"range_edges must ascend, got {self.range_edges}")
        self.ncam = int(ncam)
        if self.ncam < 1:
            raise ValueError(f"ncam must be at least 1, got {ncam}")
        self.per_camera = bool(per_camera)
        self.groups = self.ncam if self.per_camera else 1
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.state = torch.zeros((self.groups, R, len(op.TERMS)), dtype=torch.float64, device=self.device)

    def reset(self):
        self.state.zero_()

    def add_batch(self, logits, dmin):
        """logits [B * ncam, D, fH, fW], dmin f32[B, ncam, fH, fW] (or [B * ncam, fH, fW]); nothing is read back."""
        from .ops import depth_metric as op
        if logits.shape[0] % self.ncam:
            raise ValueError(f"{logits.shape[0]} images are not a multiple of ncam = {self.ncam}")
        op.depth_metric_accumulate(logits, dmin, self.state, self.d_bound, self.range_edges, self.groups)

    def _reduced_state(self):
        """The state summed over the ranks, on the host: the single read."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            host_backend = dist.get_backend() == "gloo"            # gloo moves host buffers: stage through the host
            buf = self.state.to("cpu", copy=True) if host_backend else self.state.clone()   # the state itself stays local
            dist.all_reduce(buf, op=dist.ReduceOp.SUM)
            return buf.cpu()
        return self.state.cpu()

    def compute(self):
        s = self._reduced_state().numpy()                          # [groups, ranges, 12]
        out = depth_figures(s.sum((0, 1)))
        if self.explicit_ranges:
            out["ranges"] = [dict(depth_figures(s[:, r].sum(0)), lo=self.range_edges[r], hi=self.range_edges[r + 1])
                             for r in range(s.shape[1])]
        if self.per_camera:
            out["cameras"] = [depth_figures(s[g].sum(0)) for g in range(s.shape[0])]
        return out
