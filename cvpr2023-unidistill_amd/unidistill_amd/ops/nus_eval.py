"""Device half of the nuScenes detection metric (csrc/nus_eval.hip): the prediction conversion of one
batch and the per-class curves.  unidistill_amd.evaluation builds the evaluator on top."""
import ctypes

import torch

from .. import _lib

MAX_CLASSES = 15
MAX_BOXES = 1024          # UD_NUS_MAX_BOXES: predictions, and GT boxes, of one sample
PRED_COLS, GT_COLS, POINTS = 10, 9, 101
ST_CLASS, ST_SIZE, ST_COUNT = 1, 2, 4


class Cfg(ctypes.Structure):
    """UdNusCfg of include/unidistill_hip.h."""
    _fields_ = [("num_classes", ctypes.c_int), ("dist_th_tp_index", ctypes.c_int), ("pi_period_class", ctypes.c_int),
                ("pad_", ctypes.c_int), ("class_range", ctypes.c_double * MAX_CLASSES),
                ("dist_th", ctypes.c_double * 4), ("rec_pts", ctypes.c_double * POINTS)]


class Io(ctypes.Structure):
    """UdNusEvalIo of include/unidistill_hip.h (device pointers)."""
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "pred_rec", "pred_cls", "pred_attr", "pred_src", "pred_off", "gt_rec", "gt_cls", "gt_attr", "gt_num_pts",
        "gt_keep", "gt_off", "ego", "prec", "conf", "tp_err", "tp", "match_gt", "order", "counts", "status")]


def status_text(bits):
    out = []
    if bits & ST_CLASS:
        out.append("a class id is out of range")
    if bits & ST_SIZE:
        out.append("a matched pair has a size <= 0")
    if bits & ST_COUNT:
        out.append(f"a sample has more than {MAX_BOXES} boxes")
    return "; ".join(out)


def pred_to_global(boxes, scores, labels, counts, l2g, attr_moving, attr_still, status):
    """One batch: boxes f32 [n, 7 | 9], scores f32 [n], labels int64 [n] (starting at 1), sample b owning the next
    counts[b] rows, l2g f64 [B, 4, 4] on the device -> (rec f64 [n, 10], cls int32 [n], attr int32 [n]).
    A label outside 1 .. C ORs ST_CLASS into status (int32 [1], device)."""
    _lib.require_gpu(boxes, scores, labels, l2g, status)
    dev = boxes.device
    n, ncol = boxes.shape
    if ncol not in (7, 9) or scores.shape != (n,) or labels.shape != (n,):
        raise ValueError(f"boxes [n, 7 | 9], scores [n], labels [n] expected, got {tuple(boxes.shape)}, "
                         f"{tuple(scores.shape)}, {tuple(labels.shape)}")
    B = len(counts)
    if l2g.dtype != torch.float64 or tuple(l2g.shape) != (B, 4, 4):
        raise ValueError(f"lidar_to_global must be float64 [{B}, 4, 4], got {l2g.dtype} {tuple(l2g.shape)}")
    C = len(attr_moving)
    rec = torch.empty((n, PRED_COLS), dtype=torch.float64, device=dev)
    cls = torch.empty((n,), dtype=torch.int32, device=dev)
    attr = torch.empty((n,), dtype=torch.int32, device=dev)
    off = [0]
    for c in counts:
        off.append(off[-1] + int(c))
    off_dev = torch.tensor(off, dtype=torch.int32).to(dev, non_blocking=True)
    boxes = boxes.contiguous().float()
    scores = scores.contiguous().float()
    labels = labels.contiguous().long()
    l2g = l2g.contiguous()
    mv = (ctypes.c_int32 * C)(*attr_moving)
    st = (ctypes.c_int32 * C)(*attr_still)
    _lib.ud.ud_nus_pred_to_global(boxes, n, ncol, scores, labels, off_dev, max(B, 1), l2g, C, ctypes.addressof(mv),
                                  ctypes.addressof(st), rec, cls, attr, status, _lib.stream_of(rec))
    return rec, cls, attr


def evaluate(cfg, pred, gt, S, P):
    """cfg: Cfg; pred: dict rec / cls / attr (rows) + src (int64 [S]) + off (int64 [S + 1], P = off[S]); gt: dict rec / cls / attr /
    num_pts / keep / off / ego, all on one device.  -> dict of device tensors: prec / conf [C, 4, 101], tp_err [C, 5, 101],
    tp uint8 [4, P], match_gt / order int32 [P], counts int32 [2, C], status int32 [1]."""
    dev = gt["rec"].device
    _lib.require_gpu(*[v for v in pred.values()], *[v for v in gt.values()])
    C = cfg.num_classes
    out = {"prec": torch.empty((C, 4, POINTS), dtype=torch.float64, device=dev),
           "conf": torch.empty((C, 4, POINTS), dtype=torch.float64, device=dev),
           "tp_err": torch.empty((C, 5, POINTS), dtype=torch.float64, device=dev),
           "tp": torch.empty((4, max(P, 1)), dtype=torch.uint8, device=dev),
           "match_gt": torch.empty((max(P, 1),), dtype=torch.int32, device=dev),
           "order": torch.empty((max(P, 1),), dtype=torch.int32, device=dev),
           "counts": torch.empty((2, C), dtype=torch.int32, device=dev),
           "status": torch.zeros((1,), dtype=torch.int32, device=dev)}
    # struct fields, not call arguments: the addresses are stored as integers (pred, gt and out outlive the call)
    io = Io(pred_rec=_lib.ptr(pred["rec"]), pred_cls=_lib.ptr(pred["cls"]), pred_attr=_lib.ptr(pred["attr"]),
            pred_src=_lib.ptr(pred["src"]), pred_off=_lib.ptr(pred["off"]), gt_rec=_lib.ptr(gt["rec"]),
            gt_cls=_lib.ptr(gt["cls"]), gt_attr=_lib.ptr(gt["attr"]), gt_num_pts=_lib.ptr(gt["num_pts"]),
            gt_keep=_lib.ptr(gt["keep"]), gt_off=_lib.ptr(gt["off"]), ego=_lib.ptr(gt["ego"]),
            prec=_lib.ptr(out["prec"]), conf=_lib.ptr(out["conf"]), tp_err=_lib.ptr(out["tp_err"]),
            tp=_lib.ptr(out["tp"]), match_gt=_lib.ptr(out["match_gt"]), order=_lib.ptr(out["order"]),
            counts=_lib.ptr(out["counts"]), status=_lib.ptr(out["status"]))
    lib = _lib.load()
    nbytes = lib.ud_nus_eval_workspace_bytes(P, C)
    if nbytes == 0:
        raise ValueError(f"ud_nus_eval: {P} predictions / {C} classes are outside the supported sizes")
    ws = _lib.workspace(dev, nbytes, slot="nus_eval")
    _lib.ud.ud_nus_eval(ctypes.addressof(cfg), ctypes.addressof(io), S, P, ws, ws.numel(), _lib.stream_of(ws))
    out["tp"] = out["tp"][:, :P]
    out["match_gt"] = out["match_gt"][:P]
    out["order"] = out["order"][:P]
    return out
