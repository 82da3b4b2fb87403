"""LiDAR input side on the device: sweep collection and the BEV augmentation of points / boxes, and the
fused input chain after collate.

Mirrors the reference's numpy transforms (unidistill/data/multisensorfusion/transforms3d.py:379-443,
functional.py:595-646): the 4x4 matrices are built on the host in float64 exactly as the reference builds
them (they are a handful of flops), the per-point work runs in ONE ud_points_transform launch per batch.
"""
import numpy as np
import torch

from .. import _lib
from .staging import align16, staged_upload


def _check_points_seg(points, seg, min_len):
    """The device cloud and its segment offsets (at least ``min_len`` of them), checked.  -> seg as ints."""
    _lib.require_gpu(points)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] < 3 or not points.is_contiguous():
        raise ValueError("points must be a contiguous float32 [rows, D >= 3] tensor")
    seg = [int(v) for v in seg]
    if len(seg) < min_len or seg[0] != 0 or seg[-1] != points.shape[0] or any(b < a for a, b in zip(seg, seg[1:])):
        raise ValueError("seg must ascend from 0 to the number of rows")
    return seg


def points_transform(points, seg, mats, last=None, out=None):
    """points f32 [rows, D]; seg: row offsets of the S segments (S+1 ints); mats: [S,4,4] float64; last:
    optional per-segment value for the last column (NaN = keep).  Returns the transformed cloud."""
    seg = _check_points_seg(points, seg, 0)
    S = len(seg) - 1
    dev = points.device
    mats_d = torch.as_tensor(np.ascontiguousarray(np.asarray(mats, np.float64).reshape(S, 16)), device=dev)
    seg_d = torch.tensor(seg, dtype=torch.int64, device=dev)
    last_d = None if last is None else torch.as_tensor(np.asarray(last, np.float32).reshape(S), device=dev)
    out = torch.empty_like(points) if out is None else out
    max_rows = max((b - a for a, b in zip(seg, seg[1:])), default=0)
    _lib.ud.ud_points_transform(points, out, seg_d, mats_d, last_d, S, points.shape[1], max_rows, _lib.stream_of(points))
    return out


def sweep_to_key_matrix(key_lidar_to_ego, key_ego_to_global, sweep_pose):
    """transforms3d.py:394-400 (left-associative product, float64)."""
    L, G, S = (np.asarray(m, np.float64) for m in (key_lidar_to_ego, key_ego_to_global, sweep_pose))
    return np.linalg.inv(L) @ np.linalg.inv(G) @ S @ L


def collect_lidar_sweeps(points, sweep_points, info):
    """CollectLidarSweeps.forward for device clouds: ``points`` [N,D] and the list ``sweep_points``, ``info``
    as in the reference's data_dict["info"] (ego_to_global, lidar_to_ego, timestamp, sweep_lidar_infos).
    Returns the concatenated [N + sum(Ni), D] cloud; for D == 5 the last column is the time lag in seconds."""
    clouds = [points] + list(sweep_points)
    D = points.shape[1]
    mats = [np.eye(4)] + [sweep_to_key_matrix(info["lidar_to_ego"], info["ego_to_global"], s["sweep_lidar_to_ego"])
                          for s in info["sweep_lidar_infos"]]
    nan = float("nan")
    if D == 5:
        last = [0.0] + [(info["timestamp"] - s["sweep_lidar_timestamp"]) / 1e6 for s in info["sweep_lidar_infos"]]
    else:
        last = [nan] * len(clouds)
    seg = np.cumsum([0] + [c.shape[0] for c in clouds])
    return points_transform(torch.cat(clouds).contiguous(), seg, np.stack(mats), last)


def bev_transform_matrix(rotate_deg, scale, trans, flip_dx, flip_dy):
    """functional.bev_transform's matrix (functional.py:595-632), float64."""
    a = rotate_deg / 180 * np.pi
    s, c = np.sin(a), np.cos(a)
    rot = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    sc = np.diag([scale, scale, scale, 1.0])
    tr = np.eye(4)
    tr[:3, 3] = trans
    flip = np.eye(4)
    if flip_dx:
        flip = flip @ np.diag([-1.0, 1.0, 1.0, 1.0])
    if flip_dy:
        flip = flip @ np.diag([1.0, -1.0, 1.0, 1.0])
    return flip @ tr @ sc @ rot


def bev_affine(points, gt_boxes, rotate_deg, scale, trans, flip_dx, flip_dy):
    """BevAffineTransformation.forward with the drawn augmentation given: points [N,D] and gt_boxes [M,7|9]
    (float32, device) -> (points', gt_boxes', bda_mat float64 4x4).  Box arithmetic follows
    functional.py:633-646 in the reference's precisions (centres in float64, the rest in float32)."""
    rotate_deg, scale = float(rotate_deg), float(scale)
    mat = bev_transform_matrix(rotate_deg, scale, trans, flip_dx, flip_dy)
    out = points_transform(points, [0, points.shape[0]], mat[None])
    boxes = gt_boxes.clone()
    if boxes.shape[0] > 0:
        boxes[:, :7] = points_transform(boxes[:, :7].contiguous(), [0, boxes.shape[0]], mat[None])
        boxes[:, 3:6] = gt_boxes[:, 3:6] * scale
        yaw = gt_boxes[:, 6] + rotate_deg / 180 * np.pi
        if flip_dx:
            yaw = np.pi - yaw
        if flip_dy:
            yaw = -yaw
        boxes[:, 6] = yaw
        if boxes.shape[1] > 7:          # velocities through the 2x2 block: float64 products, one rounding to float32
            v = gt_boxes[:, 7:9].double()
            boxes[:, 7] = (float(mat[0, 0]) * v[:, 0] + float(mat[0, 1]) * v[:, 1]).float()
            boxes[:, 8] = (float(mat[1, 0]) * v[:, 0] + float(mat[1, 1]) * v[:, 1]).float()
    return out, boxes, mat


# ---- LiDAR input chain after collate -----------------------------------------------------------
# The reference's det augmentor runs CollectLidarSweeps -> BevAffineTransformation -> ObjectRangeFilter on every
# sample's points in the loader (transforms3d.py:379-443, :242-287).  Here the loader-side classes only draw the
# parameters, do the box-level work (a few dozen boxes) and record in data_dict["lidar_aug"] what the device must do
# with the points; collate_fn stages the raw clouds of the whole batch in pinned memory, copies them in one H2D copy
# and runs the per-point work in one fused pass (ud_lidar_prep_count + ud_lidar_prep_compact): sweep transform, BDA,
# range test, stable compaction and the zero-padded [B, Nmax, D] stack of fill_batch_tensor.
_SEG_PAR, _SMP_PAR, _MAX_SEG = 18, 24, 64          # include/unidistill_hip.h UD_LIDAR_*


def _pack(arrays):
    """[(name, array)] -> (uint8 buffer with 16-byte aligned sections, {name: (offset, array)})."""
    parts, off = {}, 0
    for name, a in arrays:
        parts[name] = (off, a)
        off = align16(off + a.nbytes)
    buf = np.zeros(off, np.uint8)
    for o, a in parts.values():
        buf[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return buf, parts


def _lidar_arrays(seg_rows, sample_nseg, seg_mats, seg_xform, seg_last, bdas, ranges):
    """Host plan of ud_lidar_prep_*: segment row offsets, per-sample segment offsets and the two parameter tables, as
    [(name, array)] in plan order."""
    S, B = len(seg_rows), len(sample_nseg)
    seg = np.zeros(S + 1, np.int64)
    seg[1:] = np.cumsum(seg_rows)
    sseg = np.zeros(B + 1, np.int64)
    sseg[1:] = np.cumsum(sample_nseg)
    sp = np.zeros((S, _SEG_PAR), np.float64)
    for s in range(S):
        if seg_xform[s]:
            sp[s, :16] = np.asarray(seg_mats[s], np.float64).reshape(16)
            sp[s, 17] = 1.0
        sp[s, 16] = seg_last[s]
    bp = np.zeros((B, _SMP_PAR), np.float64)
    for b in range(B):
        if bdas[b] is not None:
            bp[b, :16] = np.asarray(bdas[b], np.float64).reshape(16)
            bp[b, 22] = 1.0
        if ranges[b] is not None:
            bp[b, 16:22] = np.asarray(ranges[b], np.float32).reshape(6)       # float32 values, exact in float64
            bp[b, 23] = 1.0
    return [("seg", seg), ("sseg", sseg), ("seg_par", sp), ("smp_par", bp)]


def _lidar_tables(*plan):
    """_lidar_arrays packed into one byte buffer.  -> (bytes, {name: (offset, array)})."""
    return _pack(_lidar_arrays(*plan))


def _chain_setup(pts_ptr, rows, D, parts, plan_base, device):
    """-> (the arguments ud_lidar_prep_* and ud_lidar_paste_* begin with, (scratch of the two passes, its size as the
    entry points take it), {plan section: device address})."""
    seg, sseg = parts["seg"][1], parts["sseg"][1]
    S, B = len(seg) - 1, len(sseg) - 1
    p = {k: plan_base + o for k, (o, _) in parts.items()}
    ws_bytes = int(_lib.load().ud_lidar_prep_workspace_bytes(seg.ctypes.data, sseg.ctypes.data, S, B))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
    args = (pts_ptr, rows, D, seg.ctypes.data, sseg.ctypes.data, S, B, p["seg"], p["sseg"], p["seg_par"], p["smp_par"])
    return args, (ws, ws_bytes), p


def _two_pass(count, compact, args, result_d, ws, device, stream, out_compact):
    """The chain's two passes, plain (ud_lidar_prep_*) or with paste (ud_lidar_paste_*), all on ``stream`` (a
    torch.cuda.Stream, current while this runs): ``count(*args, ...)`` leaves the samples' int64 counts at the head of
    the uint8 device tensor ``result_d`` -> ONE readback of result_d (waits on ``stream`` only) -> the padded or
    compact output is allocated -> ``compact(*args, ...)``.
    -> (out, counts int64 numpy [B], the bytes of result_d behind the counts as uint8 numpy)."""
    D, B = args[2], args[6]                             # as _chain_setup lays them out
    hs = stream.cuda_stream
    count(*args, result_d, *ws, hs)
    result_h = torch.empty(result_d.numel(), dtype=torch.uint8, pin_memory=True)
    result_h.copy_(result_d, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(stream)
    ev.synchronize()                                    # this stream's work only, not the caller's queue
    rh = result_h.numpy()
    counts = rh[:8 * B].view(np.int64).copy()
    nmax = int(counts.max()) if B else 0
    if out_compact:
        out = torch.empty((int(counts.sum()), D), dtype=torch.float32, device=device)
    else:
        out = torch.empty((B, nmax, D), dtype=torch.float32, device=device)
    compact(*args, counts.ctypes.data, result_d, nmax, 1 if out_compact else 0, out, out.numel() // D, *ws, hs)
    return out, counts, rh[8 * B:]


def _lidar_run(pts_ptr, rows, D, parts, plan_base, device, stream, out_compact):
    """ud_lidar_prep_count -> counts read back -> ud_lidar_prep_compact (_two_pass).  -> (out, counts int64 numpy)."""
    args, ws, _ = _chain_setup(pts_ptr, rows, D, parts, plan_base, device)
    counts_d = torch.empty(8 * max(args[6], 1), dtype=torch.uint8, device=device)
    return _two_pass(_lib.ud.ud_lidar_prep_count, _lib.ud.ud_lidar_prep_compact, args, counts_d, ws, device, stream,
                     out_compact)[:2]


def points_range_filter(points, point_cloud_range, seg=None):
    """ObjectRangeFilter.mask_points_by_range + indexing (transforms3d.py:248-255) for a device cloud points f32
    [rows, D]: keeps x in [r0, r3] and y in [r1, r4] (float32 compares, z untested, NaN dropped), in order.  ``seg``:
    row offsets of segments (S + 1 ints) filtered each on its own, e.g. the samples of a concatenated batch.
    -> (kept rows f32 [K, D], per-segment kept counts int64 numpy [S]).  Runs on the current stream."""
    seg = _check_points_seg(points, [0, *points.shape[:1]] if seg is None else seg, 1)
    rows, D = points.shape
    S = len(seg) - 1
    rng = np.asarray(point_cloud_range, np.float32).reshape(6)
    buf, parts = _lidar_tables(np.diff(seg), [1] * S, [None] * S, [False] * S, [np.nan] * S, [None] * S, [rng] * S)
    device = points.device
    plan = torch.from_numpy(buf).to(device)
    stream = torch.cuda.current_stream(device)
    return _lidar_run(points, rows, D, parts, plan.data_ptr(), device, stream, True)


def sweep_time_lag(info, sweep):
    """The value CollectLidarSweeps writes into a sweep's last column (D == 5): float64 seconds, stored as float32."""
    return np.float32((info["timestamp"] - sweep["sweep_lidar_timestamp"]) / 1e6)


def _lidar_aug(data_dict):
    """data_dict["lidar_aug"], created for a lone key frame when no CollectLidarSweeps ran before."""
    a = data_dict.get("lidar_aug")
    if a is None:
        a = data_dict["lidar_aug"] = {"segments": [len(data_dict["points"])], "sweep_mats": np.zeros((0, 4, 4)),
                                      "time_lags": np.zeros(0, np.float32), "bda_mat": None, "range": None}
    return a


class CollectLidarSweeps:
    """CollectLidarSweeps (transforms3d.py:379-414) split for the device: in the loader it records the sweep -> key
    matrices (sweep_to_key_matrix, float64) and the time lags in data_dict["lidar_aug"] and pops
    info["sweep_lidar_infos"] as the reference does; ``points`` and ``sweep_points`` stay raw.  The sample's
    ``points_raw`` = [points] + sweep_points then goes to collate_fn with the record."""

    def forward(self, data_dict):
        if data_dict.get("points", None) is not None:
            info = data_dict["info"]
            sweeps = list(data_dict.get("sweep_points", []))
            infos = info["sweep_lidar_infos"][:len(sweeps)]
            mats = [sweep_to_key_matrix(info["lidar_to_ego"], info["ego_to_global"], s["sweep_lidar_to_ego"])
                    for s in infos]
            data_dict["lidar_aug"] = {
                "segments": [len(data_dict["points"])] + [len(s) for s in sweeps],
                "sweep_mats": np.stack(mats) if mats else np.zeros((0, 4, 4)),
                "time_lags": np.array([sweep_time_lag(info, s) for s in infos], np.float32),
                "bda_mat": None, "range": None}
            info.pop("sweep_lidar_infos")
        return data_dict

    __call__ = forward


def bda_boxes(gt_boxes, mat, rotate_deg, scale, flip_dx, flip_dy):
    """functional.bev_transform's box arithmetic (functional.py:633-646) on host boxes float32 [M, 7 | 9], in the
    reference's precisions: centres through the float64 matrix, sizes * scale and yaw in float32 (numpy's rules for
    a Python-float operand), velocities through mat[:2, :2] in float64.  Returns a new array."""
    boxes = np.array(gt_boxes, copy=True)
    if boxes.shape[0] == 0:
        return boxes
    hc = np.ones((boxes.shape[0], 4))
    hc[:, :3] = boxes[:, :3]
    boxes[:, :3] = (mat @ hc.T).T[:, :3]
    boxes[:, 3:6] *= scale
    boxes[:, 6] += rotate_deg / 180 * np.pi
    if flip_dx:
        boxes[:, 6] = np.pi - boxes[:, 6]
    if flip_dy:
        boxes[:, 6] = -boxes[:, 6]
    if boxes.shape[1] > 7:
        boxes[:, 7:] = (mat[:2, :2] @ boxes[:, 7:].T).T
    return boxes


class BevAffineTransformation:
    """BevAffineTransformation (transforms3d.py:417-443) split for the device.  ``sample_augs`` draws from np.random
    in the reference's order; ``forward`` transforms gt_boxes on the host (bda_boxes), stores data_dict["bda_mat"]
    when ``imgs`` is present (the camera branch reads it) and records the matrix for the points in
    data_dict["lidar_aug"]; the points themselves are transformed on the device after collate."""

    def __init__(self, **bda_aug_conf):
        self.aug_conf = bda_aug_conf

    def sample_augs(self):
        c = self.aug_conf
        rotate = np.random.uniform(*c["rot_lim"])
        scale = np.random.uniform(*c["scale_lim"])
        trans = np.random.normal(scale=c["trans_lim"])
        flip_dx = np.random.uniform() < c["flip_dx_ratio"]
        flip_dy = np.random.uniform() < c["flip_dy_ratio"]
        return rotate, scale, trans, flip_dx, flip_dy

    def forward(self, data_dict):
        rotate, scale, trans, flip_dx, flip_dy = self.sample_augs()
        mat = bev_transform_matrix(rotate, scale, trans, flip_dx, flip_dy)
        data_dict["gt_boxes"] = bda_boxes(data_dict["gt_boxes"], mat, rotate, scale, flip_dx, flip_dy)
        if data_dict.get("points", None) is not None:
            a = _lidar_aug(data_dict)
            if a["bda_mat"] is not None or a["range"] is not None:
                raise ValueError("BevAffineTransformation must come once, before ObjectRangeFilter")
            a["bda_mat"] = mat
            a["bda_params"] = (rotate, scale, flip_dx, flip_dy)      # for boxes pasted after collate (gt_paste.py)
        if data_dict.get("imgs", None) is not None:
            data_dict["bda_mat"] = mat
        return data_dict

    __call__ = forward


_CORNERS = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]])


def boxes_in_range_mask(gt_boxes, point_cloud_range, min_num_corners=1):
    """ObjectRangeFilter's box test (transforms3d.py:258-271): a box stays when at least ``min_num_corners`` of its 8
    corners (origin (0.5, 0.5, 0.5), yaw about z) lie inside the range, bounds included.  float32 throughout, the
    rotation as the same einsum contraction the reference evaluates, so boundary corners decide alike."""
    b = np.asarray(gt_boxes)[:, :7]
    r = np.asarray(point_cloud_range, np.float32)
    dims = b[:, 3:6]
    unit = _CORNERS.astype(dims.dtype) - np.array((0.5, 0.5, 0.5), dtype=dims.dtype)
    local = dims.reshape(-1, 1, 3) * unit.reshape(1, 8, 3)
    c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
    zero, one = np.zeros_like(c), np.ones_like(c)
    rot_t = np.stack([[c, s, zero], [-s, c, zero], [zero, zero, one]])            # [3, 3, M]: row-vector rotation
    corners = np.einsum("aij,jka->aik", local, rot_t)
    corners += b[:, :3].reshape(-1, 1, 3)
    inside = ((corners >= r[:3]) & (corners <= r[3:])).all(axis=2)
    return inside.sum(axis=1) >= min_num_corners


class ObjectRangeFilter:
    """ObjectRangeFilter (transforms3d.py:242-287) split for the device: records the range for the points in
    data_dict["lidar_aug"] (applied after collate, after the BDA) and filters gt_boxes / gt_names / gt_labels on the
    host, so the dataset's filter_empty redraw sees the filtered box count.  The reference's ``self.training`` is
    always True (Compose keeps its transforms in a plain list, train() never reaches them)."""

    def __init__(self, point_cloud_range):
        self.point_cloud_range = np.array(point_cloud_range, dtype=np.float32)

    def forward(self, data_dict):
        if data_dict.get("points", None) is not None:
            _lidar_aug(data_dict)["range"] = self.point_cloud_range.copy()
        if len(data_dict.get("gt_boxes", [])) > 0:
            mask = boxes_in_range_mask(data_dict["gt_boxes"], self.point_cloud_range)
            data_dict["gt_boxes"] = data_dict["gt_boxes"][mask]
            for k in ("gt_names", "gt_labels"):
                if data_dict.get(k, None) is not None:
                    data_dict[k] = data_dict[k][mask]
        return data_dict

    __call__ = forward


def _plan_segments(clouds, aug, D):
    """Per segment (matrix, transform?, last-column value) and the sample's (BDA, range) from its lidar_aug record."""
    n = len(clouds)
    if aug is None:                         # rows copied as they are
        return [None] * n, [False] * n, [np.nan] * n, None, None
    segs = [int(v) for v in aug["segments"]]
    if segs != [len(c) for c in clouds]:
        raise ValueError(f"lidar_aug segments {segs} do not match the clouds' rows {[len(c) for c in clouds]}")
    mats = np.asarray(aug["sweep_mats"], np.float64).reshape(-1, 4, 4)
    lags = np.asarray(aug["time_lags"], np.float32).reshape(-1)
    if len(mats) != n - 1 or len(lags) != n - 1:
        raise ValueError("lidar_aug needs one sweep matrix and one time lag per sweep")
    last = [0.0] + [float(v) for v in lags] if D == 5 else [np.nan] * n
    return [None] + list(mats), [False] + [True] * (n - 1), last, aug.get("bda_mat"), aug.get("range")


def _host_clouds(clouds, plans):
    """The samples' clouds as numpy arrays, checked.  -> (arrays per sample, D)."""
    if len(clouds) != len(plans) or not clouds:
        raise ValueError("one plan per sample, at least one sample")
    arrs = [[np.asarray(c.numpy() if torch.is_tensor(c) else c) for c in cs] for cs in clouds]
    flat = [a for cs in arrs for a in cs]
    if not flat or any(a.dtype != np.float32 or a.ndim != 2 for a in flat):
        raise ValueError("clouds must be float32 [N, D] arrays")
    D = flat[0].shape[1]
    if D < 3 or any(a.shape[1] != D for a in flat):
        raise ValueError("clouds must share one D >= 3")
    if any(len(cs) == 0 or len(cs) > _MAX_SEG for cs in arrs):
        raise ValueError(f"every sample needs 1 .. {_MAX_SEG} clouds")
    return arrs, D


def _stage_clouds(host, arrs):
    """The samples' clouds back to back at the head of the staging bytes ``host``."""
    fv = host.view(np.float32)                          # every section is 16-byte aligned
    off = 0
    for cs in arrs:
        for a in cs:
            fv[off:off + a.size] = a.reshape(-1)
            off += a.size


def prep_host_clouds(clouds, plans, device):
    """lidar_prep_host_clouds (ops/collate.py) for a batch in which no plan carries a ``paste`` record: one staged
    upload of the clouds and the plan, then the two passes on the input stream."""
    device = _lib.require_gpu_device(device)
    arrs, D = _host_clouds(clouds, plans)
    per = [_plan_segments(cs, aug, D) for cs, aug in zip(arrs, plans)]      # (matrices, flags, last, BDA, range) each
    seg_rows = [len(a) for cs in arrs for a in cs]
    mats, xform, last = ([v for p in per for v in p[k]] for k in range(3))
    plan, parts = _lidar_tables(seg_rows, [len(cs) for cs in arrs], mats, xform, last, [p[3] for p in per],
                                [p[4] for p in per])
    rows = int(sum(seg_rows))
    pts_bytes = align16(rows * D * 4)

    def fill(host, dev):
        _stage_clouds(host, arrs)
        host[pts_bytes:] = plan

    def run(dev, s):
        return _lidar_run(dev.data_ptr(), rows, D, parts, dev.data_ptr() + pts_bytes, dev.device, s, False)

    return staged_upload(device, pts_bytes + plan.nbytes, fill, run)[0]
