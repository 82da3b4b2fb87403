"""Flip test-time augmentation (csrc/tta_merge.hip).

The scene goes through the network once per view -- unflipped, x-flipped, y-flipped, xy-flipped -- as one batch of
V * B samples (``flip_views``); the head's maps of the views are un-flipped and averaged in the head's own parametrisation
by one kernel (``flip_merge``), so the proposal layer reads them like the maps of B plain samples.

A view is a pair ``(flip_dx, flip_dy)`` with the meaning of ``ops.lidar_prep.bev_transform_matrix``: flip_dx mirrors the x
axis.  Views are stacked view-major on the batch axis: view v of sample b is row v * B + b.
"""
import ctypes

import torch

from .. import _lib

DOUBLE_FLIP = ((0, 0), (0, 1), (1, 0), (1, 1))
MAX_VIEWS = 4
_HEADS = ("hm", "reg", "height", "dim", "rot", "vel", "iou")
_CHANNELS = {"reg": 2, "height": 1, "dim": 3, "rot": 2, "vel": 2, "iou": 1}


def resolve_views(views):
    """"double_flip" or a sequence of 1..4 flag pairs -> tuple of (flip_dx, flip_dy) ints."""
    if isinstance(views, str):
        if views != "double_flip":
            raise ValueError(f'tta: expected "double_flip" or a list of (flip_dx, flip_dy) pairs, got {views!r}')
        return DOUBLE_FLIP
    views = tuple(views)
    if not 1 <= len(views) <= MAX_VIEWS:
        raise ValueError(f"tta: between 1 and {MAX_VIEWS} views can be merged, got {len(views)}")
    out = []
    for v in views:
        v = tuple(v)
        if len(v) != 2:
            raise ValueError(f"tta: a view is a (flip_dx, flip_dy) pair, got {v!r}")
        out.append((int(bool(v[0])), int(bool(v[1]))))
    return tuple(out)


def check_symmetric_range(pc_range, views):
    """The un-flip rules are exact only when the BEV range is symmetric about 0 on every flipped axis."""
    for axis, name in ((0, "x"), (1, "y")):
        if any(v[axis] for v in views) and float(pc_range[axis]) != -float(pc_range[axis + 3]):
            raise ValueError(f"tta: a view flips the {name} axis, but the point-cloud range [{pc_range[axis]}, "
                             f"{pc_range[axis + 3]}] on it is not symmetric about 0: the flipped maps would not line up")


def flip_matrix(view, dtype=torch.float32, device=None):
    """F_v = diag(+-1, +-1, 1, 1): bev_transform_matrix(0, 1, 0, flip_dx, flip_dy)."""
    return torch.diag(torch.tensor([-1.0 if view[0] else 1.0, -1.0 if view[1] else 1.0, 1.0, 1.0], dtype=dtype)).to(device)


def _flip_points(p, view):
    sign = torch.ones(p.shape[-1], dtype=p.dtype, device=p.device)
    sign[0] = -1.0 if view[0] else 1.0
    sign[1] = -1.0 if view[1] else 1.0
    return p * sign


def flip_views(batch, views):
    """The V * B batch, view-major, of a collated batch of B samples: 'points' (a list of [N, D] clouds or the padded
    [B, N, D] tensor) with the x and / or y column negated, 'imgs' and every tensor of 'mats_dict' repeated, and
    mats_dict['bda_mat'] = F_v @ bda_mat (created as F_v when the batch has images and no bda_mat), so the camera branch
    lifts into the flipped frame.  Other keys are passed on as they are."""
    views = resolve_views(views)
    V = len(views)
    out = dict(batch)
    points = batch.get("points")
    if points is not None:
        if isinstance(points, (list, tuple)):
            out["points"] = [_flip_points(p, v) for v in views for p in points]
        else:
            out["points"] = torch.cat([_flip_points(points, v) for v in views], 0)
    imgs = batch.get("imgs")
    if imgs is not None:
        out["imgs"] = imgs.repeat(V, *([1] * (imgs.dim() - 1)))
    mats = batch.get("mats_dict")
    if mats is not None or imgs is not None:
        mats = dict(mats or {})
        bda = mats.pop("bda_mat", None)
        new = {k: (m.repeat(V, *([1] * (m.dim() - 1))) if torch.is_tensor(m) else m) for k, m in mats.items()}
        if bda is not None:
            new["bda_mat"] = torch.cat([flip_matrix(v, bda.dtype, bda.device) @ bda for v in views], 0)
        elif imgs is not None:
            B = imgs.shape[0]
            new["bda_mat"] = torch.cat([flip_matrix(v, torch.float32, imgs.device).expand(B, 4, 4) for v in views], 0)
        out["mats_dict"] = new
    return out


def flip_merge(pred_dicts, views, *, no_log, nbox):
    """pred_dicts: list over tasks of the head dicts of V * B samples (hm, reg, height, dim, rot, and vel / iou where
    the head has them; [V * B, c, H, W], NCHW or channel slices of the packed channels-last head output, read in place)
    -> list over tasks of head dicts for B samples, the views un-flipped and averaged (ud_tta_merge: one launch).
    hm comes back as a logit and dim as a log size (unless no_log), so the proposal layer takes the result as it is.
    vel is merged only for nbox == 9.  The outputs are channel slices of one packed buffer in the inputs' layout."""
    from ..layers.gen_proposals import _desc
    views = resolve_views(views)
    V, T = len(views), len(pred_dicts)
    if nbox not in (7, 9):
        raise ValueError(f"tta: nbox is 7 or 9, got {nbox}")
    hm0 = pred_dicts[0]["hm"]
    _lib.require_gpu(hm0)
    VB, _, H, W = hm0.shape
    if VB % V:
        raise ValueError(f"tta: the head maps hold {VB} samples, not a multiple of the {V} views")
    B = VB // V
    if B == 0:
        raise ValueError("tta: empty batch")
    src, names_of, ncs = [], [], []
    for pred in pred_dicts:
        names = [n for n in _HEADS if pred.get(n) is not None and not (n == "vel" and nbox == 7)]
        for n in names:
            c = pred["hm"].shape[1] if n == "hm" else _CHANNELS[n]
            if tuple(pred[n].shape) != (VB, c, H, W):
                raise ValueError(f"tta: head {n!r} has shape {tuple(pred[n].shape)}, expected {(VB, c, H, W)}")
            _lib.require_gpu(pred[n])
        names_of.append(names)
        ncs.append(int(pred["hm"].shape[1]))
    for pred, names in zip(pred_dicts, names_of):
        src.append({n: _desc(pred[n], H, W) for n in names})
    total = sum(t.shape[1] for heads in src for t, _ in heads.values())
    planes = src[0]["hm"][1][2] == 1                       # pixel stride 1: NCHW planes; the output follows the layout
    packed = torch.empty((B, total, H, W), dtype=torch.float32, device=hm0.device,
                         memory_format=torch.contiguous_format if planes else torch.channels_last)
    ptrs, strides, optrs, ostrides, outs, off = [], [], [], [], [], 0
    for heads in src:
        res = {}
        for n in _HEADS:
            if n not in heads:
                ptrs.append(None)
                optrs.append(None)
                strides += [0, 0, 0]
                ostrides += [0, 0, 0]
                continue
            t, st = heads[n]
            o = packed[:, off:off + t.shape[1]]
            off += t.shape[1]
            ob, oc, _, ow = o.stride()
            ptrs.append(t.data_ptr())
            optrs.append(o.data_ptr())
            strides += list(st)
            ostrides += [ob, oc, ow]
            res[n] = o
        outs.append(res)
    n = T * len(_HEADS)
    flips = [f for v in views for f in v]
    _lib.ud.ud_tta_merge((ctypes.c_void_p * n)(*ptrs), (ctypes.c_longlong * (3 * n))(*strides),
                         (ctypes.c_void_p * n)(*optrs), (ctypes.c_longlong * (3 * n))(*ostrides),
                         (ctypes.c_int * T)(*ncs), (ctypes.c_int * (2 * V))(*flips), V, B, T, H, W, 1 if no_log else 0,
                         _lib.stream_of(hm0))
    return outs
