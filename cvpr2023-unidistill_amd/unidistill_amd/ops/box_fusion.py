"""Box-level fusion (weighted box fusion) of the decoded boxes of TTA views or of several models (csrc/box_fusion.hip;
DESIGN §2.22).

Where ``ops.tta.merge`` averages the head's maps before the proposal layer, this fuses what the proposal layer returns: the
boxes of S sources per sample are brought back into the original frame, clustered by a greedy rotated-BEV NMS within each
label, and every cluster becomes one box: the confidence-weighted mean of its members, with the score scaled down by the
share of the sources that saw it.  Sources may be views of one model (``fuse_padded`` on the proposal layer's padded outputs
of the V * B batch) or different models (``fuse`` on their ``pred_dicts``): nothing has to share a grid.

Everything runs on the device in three launches (``ud_box_fusion``); the only host read is ``read_num`` of the per-sample
counts, which also checks the kernel's status words.
"""
import ctypes

import torch

from .. import _lib
from . import tta

MAX_SOURCES = 16
MAX_BOXES = 16384          # valid boxes per sample: the NMS scan's limit


def _source_table(S, views, weights):
    if not 1 <= S <= MAX_SOURCES:
        raise ValueError(f"box_fusion: between 1 and {MAX_SOURCES} sources can be fused, got {S}")
    if views is None:
        views = [(0.0, 1.0, 0, 0)] * S
    else:
        views = tta._as_general(tuple(tuple(v) for v in views))
    if weights is None:
        weights = [1.0] * S
    weights = [float(w) for w in weights]
    if len(views) != S or len(weights) != S:
        raise ValueError(f"box_fusion: {S} sources, but {len(views)} views and {len(weights)} weights")
    table = []
    for v in views:
        if len(v) != 4:
            raise ValueError(f"box_fusion: a view is (flip_dx, flip_dy) or (rot_deg, scale, flip_dx, flip_dy), got {v!r}")
        sn, cs = tta._sincos(float(v[0]))
        table += [float(v[0]), float(v[1]), 1.0 if v[2] else 0.0, 1.0 if v[3] else 0.0, sn, cs]
    return table, weights


def _run(rois, scores, labels, num, S, views, weights, iou_threshold, score_threshold, max_out, debug):
    lib = _lib.load()
    _lib.require_gpu(rois, scores, labels, num)
    if rois.dim() != 3:
        raise ValueError(f"box_fusion: rois is [S * B, R, box_dim], got {tuple(rois.shape)}")
    SB, R, box_dim = rois.shape
    table, weights = _source_table(int(S), views, weights)
    S = int(S)
    if box_dim not in (7, 9):
        raise ValueError(f"box_fusion: box_dim is 7 or 9, got {box_dim}")
    if SB == 0 or SB % S:
        raise ValueError(f"box_fusion: rois holds {SB} rows of boxes, not a positive multiple of the {S} sources")
    B = SB // S
    if tuple(scores.shape) != (SB, R) or tuple(labels.shape) != (SB, R) or tuple(num.shape) != (SB,):
        raise ValueError(f"box_fusion: scores / labels / num have shapes {tuple(scores.shape)}, {tuple(labels.shape)}, "
                         f"{tuple(num.shape)}, expected {(SB, R)}, {(SB, R)}, {(SB,)}")
    if rois.dtype != torch.float32 or scores.dtype != torch.float32 or labels.dtype != torch.int64 \
            or num.dtype != torch.int32:
        raise ValueError("box_fusion: rois and scores are float32, labels int64, num int32")
    iou_threshold, score_threshold, max_out = float(iou_threshold), float(score_threshold), int(max_out)
    if iou_threshold != iou_threshold or score_threshold != score_threshold or abs(iou_threshold) == float("inf"):
        raise ValueError(f"box_fusion: iou_threshold must be finite and score_threshold not NaN, got {iou_threshold}, "
                         f"{score_threshold}")
    if max_out < 1 or R < 1:
        raise ValueError(f"box_fusion: max_out and R must be at least 1, got {max_out}, {R}")
    rois, scores, labels, num = rois.contiguous(), scores.contiguous(), labels.contiguous(), num.contiguous()
    dev = rois.device
    out_rois = torch.empty((B, max_out, box_dim), dtype=torch.float32, device=dev)
    out_scores = torch.empty((B, max_out), dtype=torch.float32, device=dev)
    out_labels = torch.empty((B, max_out), dtype=torch.int64, device=dev)
    counts = torch.empty((2, B), dtype=torch.int32, device=dev)           # out_num, then the status words: one host read
    extra = torch.empty((2, B, max_out), dtype=torch.int32, device=dev) if debug else None
    nbytes = lib.ud_box_fusion_workspace_bytes(B, S, R)
    if nbytes == 0:
        raise ValueError(f"box_fusion: unsupported sizes B={B} S={S} R={R}")
    ws = _lib.workspace(dev, nbytes, "box_fusion")
    _lib.ud.ud_box_fusion(rois, scores, labels, num, B, S, R, box_dim, (ctypes.c_double * (6 * S))(*table),
                          (ctypes.c_double * S)(*weights), iou_threshold, score_threshold, max_out, out_rois, out_scores,
                          out_labels, counts[0], counts[1], None if extra is None else extra[0],
                          None if extra is None else extra[1], ws, ws.numel(), _lib.stream_of(rois))
    return out_rois, out_scores, out_labels, counts, extra


def fuse_padded(rois, scores, labels, num, S, *, views=None, weights=None, iou_threshold, score_threshold=0.0, max_out=500,
                return_clusters=False):
    """The padded boxes of S sources of B samples -- rois f32[S * B, R, box_dim], scores f32[S * B, R], labels i64[S * B, R],
    num i32[S * B], source s of sample b in row s * B + b, as the proposal layer returns them for the batch of
    ``ops.tta.flip_views`` -- fused per sample -> (out_rois f32[B, max_out, box_dim], out_scores f32[B, max_out], out_labels
    i64[B, max_out], out_num i32[B]), zero padded, by descending fused score.  No host synchronisation.

    ``views``: per source (flip_dx, flip_dy) or (rot_deg, scale, flip_dx, flip_dy), the frame its boxes are in; None: the
    identity for every source (a model ensemble).  ``weights``: per source, > 0; None: 1.  A box counts if all its entries are
    finite and its score is > score_threshold.  Read ``out_num`` with ``read_num``, which also raises for a sample that held
    more than 16384 valid boxes.  ``return_clusters``: also i32[B, max_out] anchor (s * R + r of each cluster's first box)
    and member count."""
    out_rois, out_scores, out_labels, counts, extra = _run(rois, scores, labels, num, S, views, weights, iou_threshold,
                                                           score_threshold, max_out, return_clusters)
    if return_clusters:
        return out_rois, out_scores, out_labels, counts[0], extra[0], extra[1]
    return out_rois, out_scores, out_labels, counts[0]


def read_num(out_num):
    """The per-sample counts of ``fuse_padded`` as a list: the op's one host read.  Raises if the kernel reported a sample with
    more valid boxes than it can cluster."""
    both = out_num._base if out_num._base is not None else out_num
    if both.dim() != 2 or both.shape[0] != 2:
        raise ValueError("box_fusion.read_num takes the out_num returned by fuse_padded")
    num, status = both.tolist()
    bad = [b for b, s in enumerate(status) if s]
    if bad:
        raise RuntimeError(f"box_fusion: samples {bad} hold more than {MAX_BOXES} valid boxes: raise score_threshold or "
                           f"lower the proposal layer's post-NMS size")
    return num


def pred_dicts_of(out_rois, out_scores, out_labels, out_num):
    """B ``pred_dicts`` from the padded outputs (one host read)."""
    return [{"pred_boxes": out_rois[b, :n].clone(), "pred_scores": out_scores[b, :n].clone(),
             "pred_labels": out_labels[b, :n].clone()} for b, n in enumerate(read_num(out_num))]


def fuse(pred_dicts_per_source, *, views=None, weights=None, iou_threshold, score_threshold=0.0, max_out=500):
    """The ensemble entry point: a list of S lists of B ``pred_dicts`` ({"pred_boxes" [n, box_dim], "pred_scores" [n],
    "pred_labels" [n]} on the GPU, n free per source and sample) -> B fused ``pred_dicts``.  The sources are padded and stacked
    on the device, fused by ``fuse_padded`` and sliced by the one host read of the counts."""
    S = len(pred_dicts_per_source)
    if S == 0:
        raise ValueError("box_fusion: no sources")
    B = len(pred_dicts_per_source[0])
    if B == 0 or any(len(p) != B for p in pred_dicts_per_source):
        raise ValueError("box_fusion: every source holds the pred_dicts of the same B >= 1 samples")
    first = pred_dicts_per_source[0][0]["pred_boxes"]
    _lib.require_gpu(first)
    box_dim, dev = first.shape[1], first.device
    counts = [int(pd["pred_boxes"].shape[0]) for src in pred_dicts_per_source for pd in src]
    R = max(max(counts), 1)
    rois = torch.zeros((S * B, R, box_dim), dtype=torch.float32, device=dev)
    scores = torch.zeros((S * B, R), dtype=torch.float32, device=dev)
    labels = torch.zeros((S * B, R), dtype=torch.int64, device=dev)
    for s, src in enumerate(pred_dicts_per_source):
        for b, pd in enumerate(src):
            n = counts[s * B + b]
            if tuple(pd["pred_boxes"].shape) != (n, box_dim):
                raise ValueError(f"box_fusion: source {s} sample {b} has boxes of shape {tuple(pd['pred_boxes'].shape)}, "
                                 f"expected [n, {box_dim}]")
            rois[s * B + b, :n] = pd["pred_boxes"]
            scores[s * B + b, :n] = pd["pred_scores"]
            labels[s * B + b, :n] = pd["pred_labels"]
    num = torch.tensor(counts, dtype=torch.int32).to(dev)
    return pred_dicts_of(*fuse_padded(rois, scores, labels, num, S, views=views, weights=weights,
                                      iou_threshold=iou_threshold, score_threshold=score_threshold, max_out=max_out))
