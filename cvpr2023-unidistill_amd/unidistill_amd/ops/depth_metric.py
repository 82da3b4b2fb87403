"""Depth metric of the camera student's lift (csrc/depth_metric.hip), accumulated on the device.

``depth_metric_accumulate`` adds, for the labelled pixels of one batch, the twelve sums behind abs-rel, sq-rel, RMSE,
RMSE-log, MAE, delta < 1.25^k, the depth-bin accuracies and the bin NLL to a float64 state tensor, per camera group and per
range bucket.  Two launches, nothing read back: ``evaluation.DepthMetric`` turns the state into figures once, at the end.
"""
import ctypes

import torch

from .. import _lib

TERMS = ("n", "abs_err", "abs_rel", "sq_rel", "sq_err", "sq_log", "d1", "d2", "d3", "bin_hit", "bin_hit1", "nll")
MAX_RANGES = 8


def depth_bins(d_bound):
    """(d_lo, d_step, D) of a frustum's d_bound = (lo, hi, step): D as LSSFPN.create_frustum counts it."""
    lo, hi, step = (float(v) for v in d_bound)
    return lo, step, int(torch.arange(lo, hi, step, dtype=torch.float).numel())


def depth_metric_accumulate(logits, dmin, state, d_bound, range_edges, ncam_groups=1):
    """logits [BN, D, fH, fW] (any strides: e.g. the first D channels of the depth net's NCHW or channels-last output; bf16 is
    widened, as ops.depth_sup.depth_loss does), dmin f32[BN, fH, fW] or [B, ncam, fH, fW] (ops.depth_sup.lidar_depth_labels; +inf =
    no LiDAR return), state f64[ncam_groups, len(range_edges) - 1, 12] on the device, range_edges ascending host floats.
    state += the sums of this batch (the order of TERMS); image n belongs to group n % ncam_groups.  Returns state."""
    _lib.require_gpu(logits, dmin, state)
    BN, D, fH, fW = logits.shape
    lo, step, _ = depth_bins(d_bound)
    edges = [float(v) for v in range_edges]
    R, G = len(edges) - 1, int(ncam_groups)
    assert dmin.dtype == torch.float32 and dmin.numel() == BN * fH * fW, (dmin.dtype, tuple(dmin.shape))
    assert state.dtype == torch.float64 and state.is_contiguous() and state.numel() == max(G, 0) * max(R, 0) * len(TERMS), \
        (state.dtype, tuple(state.shape), G, R)
    x = logits if logits.dtype == torch.float32 else logits.float()
    dmin = dmin.contiguous()
    lib = _lib.load()
    ws = _lib.workspace(x.device, lib.ud_depth_metric_workspace_bytes(BN, fH, fW), "depth_metric")
    sn, sc, sh, sw = x.stride()
    _lib.ud.ud_depth_metric_accumulate(x, sn, sc, sh, sw, dmin, BN, D, fH, fW, G, lo, step,
                                       (ctypes.c_double * (R + 1))(*edges), R, state, ws, ws.numel(), _lib.stream_of(state))
    return state
