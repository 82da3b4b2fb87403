"""LiDAR depth supervision of the camera student's lift (csrc/depth_sup.hip): the BEVDepth recipe.

``lidar_depth_labels`` projects the collated, post-BDA cloud into the key frame's images -- the inverse of the chain
``LSSFPN.get_geometry`` runs forward -- and keeps, per feature cell, the minimum depth and its depth bin
(BEVDepth's ``get_downsampled_gt_depth``; two points in one full-resolution pixel also resolve by minimum).
``depth_loss`` is ``binary_cross_entropy(softmax(logits), onehot(label))`` summed over the labelled pixels and divided by
their number, forward in two launches and backward in one; the probabilities are recomputed in the backward, never stored.
"""
import torch

from .. import _lib


def lidar_depth_labels(points, sensor2ego, intrin, ida, bda, d_bound, final_dim, downsample_factor):
    """points f32[B, Nmax, >= 3] (zero rows are padding); sensor2ego / intrin / ida [B, ncam, 4, 4] of the key frame;
    bda [B, 4, 4] or None; d_bound (lo, hi, step); final_dim (H, W)
    -> (dmin f32[B, ncam, fH, fW], +inf where no point fell; label i32[B, ncam, fH, fW], -1 there)."""
    _lib.require_gpu(points, sensor2ego, intrin, ida, bda)
    assert points.dim() == 3 and points.shape[2] >= 3, tuple(points.shape)
    assert sensor2ego.dim() == 4 and sensor2ego.shape[2:] == (4, 4), "key-frame matrices [B, ncam, 4, 4]"
    B, ncam = sensor2ego.shape[:2]
    assert points.shape[0] == B and intrin.shape == sensor2ego.shape and ida.shape == sensor2ego.shape
    pts = points if points.dtype == torch.float32 else points.float()
    if pts.shape[1] > 0 and pts.stride(2) != 1:
        pts = pts.contiguous()
    s2e, k, a = (t.contiguous().float() for t in (sensor2ego, intrin, ida))
    bd = None if bda is None else bda.contiguous().float()
    H, W = int(final_dim[0]), int(final_dim[1])
    ds = int(downsample_factor)
    lo, hi, step = (float(v) for v in d_bound)
    D = int(torch.arange(lo, hi, step, dtype=torch.float).numel())          # the frustum's depth count (LSSFPN.create_frustum)
    dev = pts.device
    dmin = torch.empty((B, ncam, H // ds, W // ds), dtype=torch.float32, device=dev)
    label = torch.empty((B, ncam, H // ds, W // ds), dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = _lib.workspace(dev, lib.ud_depth_labels_workspace_bytes(B, ncam), "depth_labels")
    _lib.ud.ud_depth_labels(pts if pts.shape[1] > 0 else None, pts.stride(0), pts.stride(1), B, pts.shape[1], s2e, k, a, bd,
                            ncam, H, W, ds, lo, hi, step, D, dmin, label, ws, ws.numel(), _lib.stream_of(dmin))
    return dmin, label


class DepthLoss(torch.autograd.Function):
    """logits f32[BN, D, fH, fW] (any strides: e.g. the first D channels of the depth net's NCHW or channels-last output),
    label i32[BN, fH, fW] (-1 = no LiDAR return) -> scalar.  Saves the logits and the labels; the 8-byte (loss, |fg|) result
    rides on the context."""

    @staticmethod
    def forward(ctx, logits, label):
        _lib.require_gpu(logits, label)
        BN, D, fH, fW = logits.shape
        assert label.dtype == torch.int32 and label.numel() == BN * fH * fW, (label.dtype, tuple(label.shape))
        label = label.contiguous()
        lib = _lib.load()
        res = torch.empty(2, dtype=torch.float32, device=logits.device)
        ws = _lib.workspace(logits.device, lib.ud_depth_loss_workspace_bytes(BN, fH, fW), "depth_loss")
        sn, sc, sh, sw = logits.stride()
        _lib.ud.ud_depth_loss_fwd(logits, sn, sc, sh, sw, label, BN, D, fH, fW, res, ws, ws.numel(), _lib.stream_of(logits))
        ctx.save_for_backward(logits, label)
        ctx.res = res
        return res[0]

    @staticmethod
    def backward(ctx, g):
        logits, label = ctx.saved_tensors
        BN, D, fH, fW = logits.shape
        g = g.contiguous().float()
        dx = torch.empty_like(logits)                    # the logits' own axis order, dense
        sn, sc, sh, sw = logits.stride()
        dn, dc, dh, dw = dx.stride()
        _lib.ud.ud_depth_loss_bwd(logits, sn, sc, sh, sw, label, ctx.res, g, dx, dn, dc, dh, dw, BN, D, fH, fW,
                                  _lib.stream_of(dx))
        return dx, None


def depth_loss(logits, label):
    """Mean over the labelled pixels of sum_j BCE(softmax(logits)_j, onehot(label)_j); exactly 0 without one.
    bf16 logits are widened first (as ops.lss.depth_ctx does)."""
    _lib.require_gpu(logits, label)
    x = logits if logits.dtype == torch.float32 else logits.float()
    return DepthLoss.apply(x, label)
