"""Test-time augmentation: flips (csrc/tta_merge.hip), rotations and scales (csrc/tta_merge_affine.hip; §2.21).

The scene goes through the network once per view -- unflipped, x-flipped, y-flipped, xy-flipped -- as one batch of
V * B samples (``flip_views``); the head's maps of the views are un-flipped and averaged in the head's own parametrisation
by one kernel (``flip_merge``), so the proposal layer reads them like the maps of B plain samples.

A view is a pair ``(flip_dx, flip_dy)`` with the meaning of ``ops.lidar_prep.bev_transform_matrix``: flip_dx mirrors the x
axis.  Views are stacked view-major on the batch axis: view v of sample b is row v * B + b.

A general view is ``(rot_deg, scale, flip_dx, flip_dy)``: the scene under A_v = F S R (``view_matrix``; z scaled too, no
translation).  Its maps cannot be merged by index reversal: ``affine_merge`` resamples them onto the unrotated grid and
brings the values back into the original frame.  ``merge`` picks the kernel; a list of up to four pure flips takes the flip
path exactly as before.  ``views()`` builds the product of rotations, scales and flips.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _lib

DOUBLE_FLIP = ((0, 0), (0, 1), (1, 0), (1, 1))
MAX_VIEWS = 4
MAX_AFFINE_VIEWS = 16
_HEADS = ("hm", "reg", "height", "dim", "rot", "vel", "iou")
_CHANNELS = {"reg": 2, "height": 1, "dim": 3, "rot": 2, "vel": 2, "iou": 1}


def resolve_views(views):
    """"double_flip" or a sequence of 1..4 flag pairs -> tuple of (flip_dx, flip_dy) ints.  A sequence that holds general
    views (rot_deg, scale, flip_dx, flip_dy) -- 1..16 of them, pairs among them taken as pure flips -> tuple of
    (float, float, int, int); if all of them are pure flips and there are at most four, the tuple of pairs instead, so
    that they take the flip path.  scale is finite and > 0, rot_deg finite, and view 0 is a pure flip or the identity:
    it alone is sure to cover every output pixel."""
    if isinstance(views, str):
        if views != "double_flip":
            raise ValueError(f'tta: expected "double_flip" or a list of (flip_dx, flip_dy) pairs, got {views!r}')
        return DOUBLE_FLIP
    views = tuple(tuple(v) for v in views)
    if any(len(v) == 4 for v in views):
        return _resolve_general(views)
    if not 1 <= len(views) <= MAX_VIEWS:
        raise ValueError(f"tta: between 1 and {MAX_VIEWS} views can be merged, got {len(views)}")
    out = []
    for v in views:
        if len(v) != 2:
            raise ValueError(f"tta: a view is a (flip_dx, flip_dy) pair, got {v!r}")
        out.append((int(bool(v[0])), int(bool(v[1]))))
    return tuple(out)


def _resolve_general(views):
    if not 1 <= len(views) <= MAX_AFFINE_VIEWS:
        raise ValueError(f"tta: between 1 and {MAX_AFFINE_VIEWS} rotation / scale views can be merged, got {len(views)}")
    out = []
    for v in views:
        if len(v) == 2:
            v = (0.0, 1.0) + v
        if len(v) != 4:
            raise ValueError(f"tta: a view is (flip_dx, flip_dy) or (rot_deg, scale, flip_dx, flip_dy), got {v!r}")
        rot, scale = float(v[0]), float(v[1])
        if not math.isfinite(rot):
            raise ValueError(f"tta: the rotation of a view must be finite, got {v!r}")
        if not (math.isfinite(scale) and scale > 0):
            raise ValueError(f"tta: the scale of a view must be finite and > 0, got {v!r}")
        out.append((rot, scale, int(bool(v[2])), int(bool(v[3]))))
    if not _pure_flip(out[0]):
        raise ValueError(f"tta: view 0 must be a pure flip or the identity (rot_deg 0, scale 1), so that every output pixel "
                         f"is covered by at least one view; it is {out[0]}")
    if len(out) <= MAX_VIEWS and all(_pure_flip(v) for v in out):
        return tuple(v[2:] for v in out)
    return tuple(out)


def _pure_flip(view):
    return len(view) == 2 or (view[0] == 0.0 and view[1] == 1.0)


def _is_flip_list(views):
    """Resolved views that go the flip path (flip_merge)."""
    return all(len(v) == 2 for v in views)


def _as_general(views):
    return tuple((0.0, 1.0) + tuple(v) if len(v) == 2 else tuple(v) for v in views)


def is_identity(view):
    return _pure_flip(view) and not view[-2] and not view[-1]


def views(rotations=(0.0,), scales=(1.0,), flips="double"):
    """The product of rotations (degrees), scales and flips as a list of (rot_deg, scale, flip_dx, flip_dy): rotations
    outermost, then scales, the flips innermost -- ``"double"``: (0, 0), (0, 1), (1, 0), (1, 1); ``None``: (0, 0) alone; or a
    sequence of pairs.  rotations[0] must be 0, scales[0] must be 1 and the first flip (0, 0): the identity comes first."""
    flips = DOUBLE_FLIP if flips == "double" else ((0, 0),) if flips is None else resolve_views(flips)
    rotations, scales = tuple(float(r) for r in rotations), tuple(float(s) for s in scales)
    if not rotations or not scales or rotations[0] != 0.0 or scales[0] != 1.0 or tuple(flips[0]) != (0, 0):
        raise ValueError("tta: rotations start with 0, scales with 1 and flips with (0, 0), so that view 0 is the identity")
    return [(r, s, fx, fy) for r in rotations for s in scales for fx, fy in flips]


def _sincos(rot_deg):
    """sin, cos of an angle in degrees; exactly 0 / +-1 at multiples of 90."""
    q = rot_deg / 90.0
    if q == math.floor(q):
        return ((0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0))[int(q % 4)]
    a = rot_deg / 180 * np.pi
    return float(np.sin(a)), float(np.cos(a))


def view_matrix(view):
    """A_v = F S R (4x4 float64) of a view: ops.lidar_prep.bev_transform_matrix(rot_deg, scale, 0, flip_dx, flip_dy), with
    sin / cos exact at multiples of 90 degrees.  z is scaled too."""
    rot, scale, fx, fy = _as_general((view,))[0]
    s, c = _sincos(rot)
    m = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]) * np.array([scale, scale, scale, 1.0])[:, None]
    return np.diag([-1.0 if fx else 1.0, -1.0 if fy else 1.0, 1.0, 1.0]) @ m + 0.0


def _linear_inverse(view):
    """The inverse of A_v's xy block, R^T F / s, from the same exact sin / cos."""
    rot, scale, fx, fy = _as_general((view,))[0]
    s, c = _sincos(rot)
    return (np.array([[c, s], [-s, c]]) @ np.diag([-1.0 if fx else 1.0, -1.0 if fy else 1.0])) / scale + 0.0


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


def _view_points(p, view):
    """The cloud(s) of a view: a pure flip negates columns (as flip_views always did); anything else multiplies the xyz
    columns by the 3x3 block of A_v, one fp32 product and sum at a time; other columns are untouched."""
    if _pure_flip(view):
        return _flip_points(p, view[-2:])
    a = view_matrix(view)[:3, :3].astype(np.float32).tolist()
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    out = p.clone()
    out[..., 0] = a[0][0] * x + a[0][1] * y
    out[..., 1] = a[1][0] * x + a[1][1] * y
    out[..., 2] = a[2][2] * z
    return out


def _view_matrix_t(view, dtype, device):
    if _pure_flip(view):
        return flip_matrix(view[-2:], dtype, device)
    return torch.from_numpy(view_matrix(view)).to(dtype).to(device)


def flip_views(batch, views):
    """The V * B batch, view-major, of a collated batch of B samples: 'points' (a list of [N, D] clouds or the padded
    [B, N, D] tensor) with the x and / or y column negated, 'imgs' and every tensor of 'mats_dict' repeated, and
    mats_dict['bda_mat'] = F_v @ bda_mat (created as F_v when the batch has images and no bda_mat), so the camera branch
    lifts into the flipped frame.  Other keys are passed on as they are.  For a general view (rot_deg, scale, flip_dx,
    flip_dy) the xyz columns are multiplied by the 3x3 block of A_v = view_matrix(view) and bda_mat = A_v @ bda_mat."""
    views = resolve_views(views)
    V = len(views)
    out = dict(batch)
    points = batch.get("points")
    if points is not None:
        if isinstance(points, (list, tuple)):
            out["points"] = [_view_points(p, v) for v in views for p in points]
        else:
            out["points"] = torch.cat([_view_points(points, v) for v in views], 0)
    imgs = batch.get("imgs")
    if imgs is not None:
        out["imgs"] = imgs.repeat(V, *([1] * (imgs.dim() - 1)))
    mats = batch.get("mats_dict")
    if mats is not None or imgs is not None:
        mats = dict(mats or {})
        bda = mats.pop("bda_mat", None)
        new = {k: (m.repeat(V, *([1] * (m.dim() - 1))) if torch.is_tensor(m) else m) for k, m in mats.items()}
        if bda is not None:
            new["bda_mat"] = torch.cat([_view_matrix_t(v, bda.dtype, bda.device) @ bda for v in views], 0)
        elif imgs is not None:
            B = imgs.shape[0]
            new["bda_mat"] = torch.cat([_view_matrix_t(v, torch.float32, imgs.device).expand(B, 4, 4) for v in views], 0)
        out["mats_dict"] = new
    return out


def flip_merge(pred_dicts, views, *, no_log, nbox):
    """pred_dicts: list over tasks of the head dicts of V * B samples (hm, reg, height, dim, rot, and vel / iou where
    the head has them; [V * B, c, H, W], NCHW or channel slices of the packed channels-last head output, read in place)
    -> list over tasks of head dicts for B samples, the views un-flipped and averaged (ud_tta_merge: one launch).
    hm comes back as a logit and dim as a log size (unless no_log), so the proposal layer takes the result as it is.
    vel is merged only for nbox == 9.  The outputs are channel slices of one packed buffer in the inputs' layout."""
    views = resolve_views(views)
    if not _is_flip_list(views):
        raise ValueError(f"tta: flip_merge takes (flip_dx, flip_dy) views only; use merge() for {views}")
    V = len(views)
    B, T, H, W, tables, ncs, outs, hm0 = _tables(pred_dicts, V, nbox)
    flips = [f for v in views for f in v]
    _lib.ud.ud_tta_merge(*tables, (ctypes.c_int * T)(*ncs), (ctypes.c_int * (2 * V))(*flips), V, B, T, H, W,
                         1 if no_log else 0, _lib.stream_of(hm0))
    return outs


def _tables(pred_dicts, V, nbox):
    """The checked descriptor tables of ud_tta_merge / ud_tta_merge_affine for the head dicts of V * B samples, and the
    output dicts: channel slices of one packed buffer in the inputs' layout."""
    from ..layers.gen_proposals import _desc
    T = len(pred_dicts)
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
    tables = ((ctypes.c_void_p * n)(*ptrs), (ctypes.c_longlong * (3 * n))(*strides),
              (ctypes.c_void_p * n)(*optrs), (ctypes.c_longlong * (3 * n))(*ostrides))
    return B, T, H, W, tables, ncs, outs, hm0


def affine_params(views, pc_range, H, W):
    """The per-view table of ud_tta_merge_affine, float64 [V, 11]: T (2x3, original-frame cell units -> view-frame cell
    units: T = C^-1 A_v C with C: u -> u * cell + range_min), the inverse Ti (2x2) of T's linear part, and the scale; and
    cell_x / cell_y.  Cells need not be square nor the range symmetric.  sin / cos of multiples of 90 degrees are exactly
    0 / +-1, and an offset within 1e-9 cells of an integer is that integer (fl(fl(a * W) / a) can miss W by an ulp), so a flip
    or a quarter turn on a square symmetric grid hits cell indices exactly."""
    views = _as_general(resolve_views(views))
    x0, y0, x1, y1 = (float(pc_range[i]) for i in (0, 1, 3, 4))
    lo, size, n = np.array([x0, y0]), np.array([x1 - x0, y1 - y0]), np.array([float(W), float(H)])
    if not (size > 0).all():
        raise ValueError(f"tta: empty point-cloud range {list(pc_range)}")
    cell = size / n
    out = np.empty((len(views), 11), np.float64)
    for v, view in enumerate(views):
        L = view_matrix(view)[:2, :2]
        Li = _linear_inverse(view)
        for i in range(2):
            for j in range(2):
                ratio = 1.0 if cell[j] == cell[i] else cell[j] / cell[i]
                out[v, 3 * i + j] = L[i, j] * ratio
                out[v, 6 + 2 * i + j] = Li[i, j] * ratio
            off = (L[i, 0] * lo[0] + L[i, 1] * lo[1] - lo[i]) * n[i] / size[i]
            out[v, 3 * i + 2] = np.round(off) if abs(off - np.round(off)) < 1e-9 else off
        out[v, 10] = view[1]
    p = out[0]
    if not all((p[4 * a] == 1.0 and p[3 * a + 2] == 0.0) or (p[4 * a] == -1.0 and p[3 * a + 2] == n[a]) for a in range(2)):
        raise ValueError(f"tta: view 0 {views[0]} flips an axis on which the point-cloud range {list(pc_range)} is not "
                         f"symmetric about 0: it would not cover every output pixel")
    return out, float(cell[0] / cell[1])


def affine_merge(pred_dicts, views, pc_range, *, no_log, nbox):
    """flip_merge for general views (rot_deg, scale, flip_dx, flip_dy), pairs taken as pure flips: every view's maps are
    resampled bilinearly onto the unrotated grid of ``pc_range``, their values brought back into the original frame, and
    averaged over the views that cover a pixel (ud_tta_merge_affine: one launch, whatever the views).  Up to 16 views."""
    views = _as_general(resolve_views(views))
    hm0 = pred_dicts[0]["hm"]
    params, ratio = affine_params(views, pc_range, int(hm0.shape[2]), int(hm0.shape[3]))
    return affine_merge_table(pred_dicts, params, ratio, no_log=no_log, nbox=nbox)


def affine_merge_table(pred_dicts, params, cell_ratio, *, no_log, nbox):
    """affine_merge with the per-view table of affine_params given ([V, 11] float64; the C entry checks it)."""
    params = np.ascontiguousarray(params, np.float64).reshape(-1, 11)
    V = params.shape[0]
    if V == 0:
        raise ValueError("tta: no views")
    B, T, H, W, tables, ncs, outs, hm0 = _tables(pred_dicts, V, nbox)
    _lib.ud.ud_tta_merge_affine(*tables, (ctypes.c_int * T)(*ncs), (ctypes.c_double * (11 * V))(*params.reshape(-1).tolist()),
                                float(cell_ratio), V, B, T, H, W, 1 if no_log else 0, _lib.stream_of(hm0))
    return outs


def merge(pred_dicts, views, pc_range, *, no_log, nbox):
    """The merge of the head maps of the views: flip_merge (ud_tta_merge, after check_symmetric_range) for a list of up to
    four pure flips, affine_merge (ud_tta_merge_affine) for anything else."""
    views = resolve_views(views)
    if _is_flip_list(views):
        check_symmetric_range(pc_range, views)
        return flip_merge(pred_dicts, views, no_log=no_log, nbox=nbox)
    return affine_merge(pred_dicts, views, pc_range, no_log=no_log, nbox=nbox)
