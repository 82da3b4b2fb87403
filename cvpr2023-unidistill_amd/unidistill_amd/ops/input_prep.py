"""LiDAR input side on the device: sweep collection and the BEV augmentation of points / boxes.

Mirrors the reference's numpy transforms (unidistill/data/multisensorfusion/transforms3d.py:379-443,
functional.py:595-646): the 4x4 matrices are built on the host in float64 exactly as the reference builds
them (they are a handful of flops), the per-point work runs in ONE ud_points_transform launch per batch.
"""
import math

import numpy as np
import torch

from .. import _lib
from ..config import IMG_DIM


def points_transform(points, seg, mats, last=None, out=None):
    """points f32 [rows, D]; seg: row offsets of the S segments (S+1 ints); mats: [S,4,4] float64; last:
    optional per-segment value for the last column (NaN = keep).  Returns the transformed cloud."""
    _lib.require_gpu(points)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] < 3 or not points.is_contiguous():
        raise ValueError("points must be a contiguous float32 [rows, D >= 3] tensor")
    seg = [int(v) for v in seg]
    S = len(seg) - 1
    if seg[0] != 0 or seg[-1] != points.shape[0] or any(b < a for a, b in zip(seg, seg[1:])):
        raise ValueError("seg must ascend from 0 to the number of rows")
    dev = points.device
    mats_d = torch.as_tensor(np.ascontiguousarray(np.asarray(mats, np.float64).reshape(S, 16)), device=dev)
    seg_d = torch.tensor(seg, dtype=torch.int64, device=dev)
    last_d = None if last is None else torch.as_tensor(np.asarray(last, np.float32).reshape(S), device=dev)
    out = torch.empty_like(points) if out is None else out
    max_rows = max((b - a for a, b in zip(seg, seg[1:])), default=0)
    _lib.check(_lib.load().ud_points_transform(_lib.ptr(points), _lib.ptr(out), _lib.ptr(seg_d), _lib.ptr(mats_d),
                                               _lib.ptr(last_d), S, points.shape[1], max_rows, _lib.stream_of(points)),
               "ud_points_transform")
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


# ---- camera side + collate ---------------------------------------------------------------------
IMG_MEAN, IMG_STD, TO_RGB = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375), True    # base_nuscenes_cfg.py:31


def image_normalize(imgs_u8, mean=IMG_MEAN, std=IMG_STD, to_rgb=TO_RGB, channels_last=False):
    """ImageNormalize.forward (transforms3d.py:350-368 -> mmcv.imnormalize) + the dataset's HWC -> CHW permute /
    stack (nuscenes_multimodal.py:262-293) for uint8 images on the device: imgs_u8 [..., H, W, 3] -> float32
    [..., 3, H, W] (``channels_last``: same shape, NHWC memory)."""
    _lib.require_gpu(imgs_u8)
    if imgs_u8.dtype != torch.uint8 or imgs_u8.shape[-1] != 3 or imgs_u8.dim() < 3:
        raise ValueError("imgs_u8 must be uint8 [..., H, W, 3]")
    x = imgs_u8.contiguous()
    lead, (H, W) = x.shape[:-3], x.shape[-3:-1]
    NI = int(np.prod(lead)) if lead else 1
    import ctypes
    f3 = lambda v: (ctypes.c_float * 3)(*[float(a) for a in v])
    if channels_last:
        out = torch.empty((NI, H, W, 3), dtype=torch.float32, device=x.device)
    else:
        out = torch.empty((NI, 3, H, W), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().ud_image_normalize(_lib.ptr(x), _lib.ptr(out), f3(mean), f3(std), 1 if to_rgb else 0,
                                              NI, H, W, 1 if channels_last else 0, _lib.stream_of(x)),
               "ud_image_normalize")
    if channels_last:
        out = out.permute(0, 3, 1, 2)              # [NI, 3, H, W] view of the NHWC buffer
    return out.reshape(*lead, 3, H, W)             # only splits the leading axis: a view in both layouts


def _fill_batch_tensor(batch_data, device):
    """fill_batch_tensor of collate_fn (nuscenes_multimodal.py:441-463): stack equal-length samples, zero-pad
    ragged ones to the longest (one ud_collate_pad launch); float32 on ``device``."""
    ts = [d if torch.is_tensor(d) else torch.as_tensor(np.asarray(d)) for d in batch_data]
    lens = [len(t) for t in ts]
    if max(lens) == min(lens):
        return torch.stack([t.to(device=device, dtype=torch.float32, non_blocking=True) for t in ts])
    tail = next(tuple(t.shape[1:]) for t in ts if t.numel() != 0)
    W = int(np.prod(tail)) if tail else 1
    L, B = max(lens), len(ts)
    dev_ts = [t.to(device=device, dtype=torch.float32, non_blocking=True).contiguous() for t in ts]
    out = torch.empty((B, L) + tail, dtype=torch.float32, device=device)
    import ctypes
    ptrs = (ctypes.c_void_p * B)(*[t.data_ptr() if t.numel() else None for t in dev_ts])
    rows = (ctypes.c_int64 * B)(*[n if t.numel() else 0 for n, t in zip(lens, dev_ts)])
    _lib.check(_lib.load().ud_collate_pad(ptrs, rows, B, L, W, _lib.ptr(out), _lib.stream_of(out)), "ud_collate_pad")
    return out


def collate_fn(data, device="cuda", is_return_depth=False, with_points=True, ida_transform=None):
    """collate_fn of the reference (data/multisensorfusion/nuscenes_multimodal.py:418-495) with the batch
    assembled ON THE DEVICE: same keys, shapes and dtypes (float32) -- ``imgs`` [B, sweeps, cams, 3, h, w],
    ``points`` [B, Nmax, D] zero padded, ``gt_boxes`` [B, Mmax, S], ``gt_labels`` [B, Mmax], ``mats_dict`` of
    stacked 4x4 matrices, ``img_metas`` passed through.  A sample may carry ``imgs_u8`` ([sweeps, cams, H, W, 3]
    uint8, not yet normalised) instead of ``imgs``: normalisation + permute then run here in one launch.
    Or it carries the RAW camera frames ``imgs_raw`` ([sweeps, cams, H, W, 3] uint8, not yet augmented) with their
    ``ida_aug`` ([sweeps][cams] tuples from ImageAffineTransformation.sample_augs, as its loader-side forward stores
    them): the reference's ImageAffineTransformation + ImageNormalize then run here, in one image_affine launch for
    the batch (only each frame's crop row band travels), and ``mats_dict["ida_mats"]`` is built from the same augs.
    Samples without ``ida_aug`` draw theirs from ``ida_transform`` (an ImageAffineTransformation), camera by camera."""
    device = torch.device(device)
    batch = {}
    ida_mats = None
    if "imgs_raw" in data[0]:
        frames = [np.asarray(d["imgs_raw"]) for d in data]
        augs = []
        for d, f in zip(data, frames):
            a = d.get("ida_aug")
            if a is None:
                if ida_transform is None:
                    raise ValueError("imgs_raw needs ida_aug per sample or an ida_transform to draw it")
                a = [ida_transform.sample_augs() for _ in range(int(np.prod(f.shape[:-3])))]
            augs += _flat_augs(a)
        fdim = tuple(ida_transform.aug_conf["final_dim"]) if ida_transform is not None else IMG_DIM
        batch["imgs"], mats = image_affine_host_frames(frames, augs, device, final_dim=fdim)
        ida_mats = torch.from_numpy(mats).to(device=device, dtype=torch.float32)
    if "imgs_u8" in data[0]:
        u8 = torch.stack([torch.as_tensor(np.asarray(d["imgs_u8"])) for d in data]).to(device, non_blocking=True)
        batch["imgs"] = image_normalize(u8)
    for key in ("imgs", "points", "gt_boxes", "gt_labels"):
        if key in data[0] and key not in batch:
            batch[key] = _fill_batch_tensor([d[key] for d in data], device)
    if "mats_dict" in data[0]:
        batch["mats_dict"] = {}
        for key in ("sensor2ego_mats", "intrin_mats", "ida_mats", "sensor2sensor_mats", "bda_mat"):
            if key in data[0]["mats_dict"]:
                batch["mats_dict"][key] = torch.stack(
                    [torch.as_tensor(np.asarray(d["mats_dict"][key])) if not torch.is_tensor(d["mats_dict"][key])
                     else d["mats_dict"][key] for d in data]).to(device=device, dtype=torch.float32)
    if ida_mats is not None:
        batch.setdefault("mats_dict", {})["ida_mats"] = ida_mats
    batch["img_metas"] = [d.get("img_metas") for d in data]
    return batch


# ---- camera augmentation: ImageAffineTransformation on the device -------------------------------
# The reference (transforms3d.py:298-347 -> functional.img_transform, functional.py:560-592) runs every camera frame
# through PIL: resize (BICUBIC, a = -0.5) -> crop (zero fill) -> optional FLIP_LEFT_RIGHT -> rotate (NEAREST, centre,
# black fill).  The host builds what PIL's C code derives from the parameters -- the fixed-point resampling tables and
# the 16.16 rotation constants, in double exactly as Pillow does -- and one ud_image_affine launch does the pixel work
# for every frame of a batch with integer arithmetic only, so the uint8 result equals PIL's bit for bit.
_PREC = 22                      # Pillow's PRECISION_BITS for 8-bit resampling: 32 - 8 - 2
_HEADER = 2                     # per output index: lo, count, then ksize weights


def _bicubic(x):
    """Pillow's bicubic_filter (a = -0.5), in the C code's evaluation order."""
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resample_table(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for one axis (n_in -> n_out, BICUBIC): int32
    [n_out, 2 + ksize] rows of (lo, count, w_0 .. w_{ksize-1}), weights in 22-bit fixed point.  Output o is
    clip8(2^21 + sum_k in[lo + k] * w_k)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError("resample_table needs positive sizes")
    scale = float(n_in) / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    tab = np.zeros((n_out, _HEADER + ksize), np.int32)
    one = float(1 << _PREC)
    for o in range(n_out):
        c = (o + 0.5) * scale
        lo = max(int(c - support + 0.5), 0)
        cnt = min(int(c + support + 0.5), n_in) - lo
        w = [_bicubic((k + lo - c + 0.5) * ss) for k in range(cnt)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        tab[o, 0], tab[o, 1] = lo, cnt
        tab[o, _HEADER:_HEADER + cnt] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
    return tab


def rotate_constants(angle, w, h):
    """Image.rotate(angle) (NEAREST, expand=False, centre (w/2, h/2)) of a w x h image as the 16.16 constants
    (a0..a5) of Pillow's nearest-neighbour affine loop: output (x, y) reads ((a2 + a1 y + a0 x) >> 16,
    (a5 + a4 y + a3 x) >> 16) when that lies inside, else 0.  None for angle % 360 == 0 (a copy).  The transposes
    Pillow takes for 180 (and 90 / 270 on square images) are expressed as the same integer map."""
    angle = float(angle) % 360.0
    if angle == 0:
        return None
    W1, H1 = (w - 1) << 16, (h - 1) << 16
    if angle == 180:
        return (-65536, 0, W1, 0, -65536, H1)
    if angle in (90, 270) and w == h:
        # ROTATE_90 (counter-clockwise): out(x, y) = in(w-1-y, x); ROTATE_270: out(x, y) = in(y, h-1-x)
        return (0, -65536, W1, 65536, 0, 0) if angle == 90 else (0, 65536, 0, -65536, 0, H1)
    cx, cy = w / 2.0, h / 2.0
    t = -math.radians(angle)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    return (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
            fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def ida_matrix(resize, crop, flip, rotate):
    """The ida_mat functional.img_transform builds (functional.py:560-592): float64 4x4, same numpy operations."""
    rot = np.eye(2) * resize
    tran = np.zeros(2) - np.array(crop[:2])
    if flip:
        F = np.array([[-1, 0], [0, 1]])
        rot = F @ rot
        tran = F @ tran + np.array([crop[2] - crop[0], 0])
    ang = rotate / 180 * np.pi
    R = np.array([[np.cos(ang), np.sin(ang)], [-np.sin(ang), np.cos(ang)]])
    half = np.array([crop[2] - crop[0], crop[3] - crop[1]]) / 2
    half = R @ (-half) + half
    rot = R @ rot
    tran = R @ tran + half
    mat = np.zeros((4, 4))
    mat[3, 3] = 1
    mat[2, 2] = 1
    mat[:2, :2] = rot
    mat[:2, 3] = tran
    return mat


class ImageAffineTransformation:
    """ImageAffineTransformation (transforms3d.py:298-347) split for the device: ``sample_augs`` draws from
    np.random in the reference's order (the rand_flip draw short-circuits the same way), so a seeded loader
    yields the same parameters; ``forward(data_dict)`` runs in the loader and only draws -- per camera it stores
    the augs tuple in data_dict["ida_aug"] and the ida_mat in data_dict["ida_mat"], the frames stay raw.  Calling
    the object is ``forward``, as for the reference's nn.Module inside transforms3d.Compose; ``apply`` runs the
    transform on device frames (``image_affine``)."""

    def __init__(self, is_train=False, **ida_aug_conf):
        self.aug_conf = ida_aug_conf
        self.is_train = is_train

    def sample_augs(self):
        c = self.aug_conf
        H, W = c["H"], c["W"]
        fH, fW = c["final_dim"]
        if self.is_train:
            resize = np.random.uniform(*c["resize_lim"])
            newW, newH = int(W * resize), int(H * resize)
            crop_h = int((1 - np.random.uniform(*c["bot_pct_lim"])) * newH) - fH
            crop_w = int(np.random.uniform(0, max(0, newW - fW)))
            flip = bool(c["rand_flip"] and np.random.choice([0, 1]))
            rotate = np.random.uniform(*c["rot_lim"])
        else:
            resize = max(fH / H, fW / W)
            newW, newH = int(W * resize), int(H * resize)
            crop_h = int((1 - np.mean(c["bot_pct_lim"])) * newH) - fH
            crop_w = int(max(0, newW - fW) / 2)
            flip, rotate = False, 0
        return resize, (newW, newH), (crop_w, crop_h, crop_w + fW, crop_h + fH), flip, rotate

    def forward(self, data_dict):
        if data_dict.get("imgs", None) is not None:
            data_dict["ida_aug"], data_dict["ida_mat"] = {}, {}
            for cam in data_dict["imgs"].keys():
                augs = self.sample_augs()
                data_dict["ida_aug"][cam] = augs
                data_dict["ida_mat"][cam] = ida_matrix(augs[0], augs[2], augs[3], augs[4])
        return data_dict

    def __call__(self, data_dict):
        """The reference's call convention (transforms3d.Compose runs ``data_dict = t(data_dict)``)."""
        return self.forward(data_dict)

    def apply(self, imgs_u8, augs=None, **kw):
        """image_affine on device frames imgs_u8 [..., H, W, 3]; augs drawn here (frame order) when not given."""
        n = int(np.prod(imgs_u8.shape[:-3])) if imgs_u8.dim() > 3 else 1
        if augs is None:
            augs = [self.sample_augs() for _ in range(n)]
        return image_affine(imgs_u8, augs, final_dim=tuple(self.aug_conf["final_dim"]), **kw)


_tables = {}          # (device type, device index, n_in, n_out) -> (host table, device table)


def _table(device, n_in, n_out):
    index = device.index
    if index is None and device.type == "cuda":
        index = torch.cuda.current_device()              # 'cuda' means the current device: key the table by its index
    key = (device.type, index, int(n_in), int(n_out))
    t = _tables.get(key)
    if t is None:
        h = resample_table(n_in, n_out)
        t = _tables[key] = (h, torch.from_numpy(h).to(device))
    return t


# per-frame record of ud_image_affine (include/unidistill_hip.h, UdImageAffineFrame): 24 int64 fields
_FRAME_FIELDS = ("src_off", "src_row0", "src_rows", "ws_off", "htab", "vtab", "hk", "vk", "rw", "rh", "cx", "cy",
                 "col0", "ncols", "band0", "band_rows", "flip", "rotate", "a0", "a1", "a2", "a3", "a4", "a5")
_NFIELD = len(_FRAME_FIELDS)


def _check_augs(augs, H, W, fH, fW):
    resize, dims, crop, flip, rotate = augs
    newW, newH = int(dims[0]), int(dims[1])
    x0, y0, x1, y1 = (int(v) for v in crop)
    if newW <= 0 or newH <= 0 or x1 - x0 != fW or y1 - y0 != fH:
        raise ValueError(f"augs {augs!r} do not give a {fW}x{fH} crop of a positive resize")
    return float(resize), newW, newH, x0, y0, bool(flip), rotate


def plan_frames(augs, H, W, final_dim, device):
    """Host side of ud_image_affine: per frame the tables, the source row band the crop's vertical windows
    touch, the resized columns inside the crop, the rotation constants and the ida_mat.
    -> (records int64 [N, _NFIELD] with src_off / src_row0 / src_rows / ws_off still to fill,
        bands [(row0, rows)], ida_mats float64 [N, 4, 4])."""
    fH, fW = final_dim
    recs = np.zeros((len(augs), _NFIELD), np.int64)
    idx = {k: i for i, k in enumerate(_FRAME_FIELDS)}
    bands, mats = [], []
    for f, a in enumerate(augs):
        resize, newW, newH, x0, y0, flip, rotate = _check_augs(a, H, W, fH, fW)
        mats.append(ida_matrix(resize, (x0, y0, x0 + fW, y0 + fH), flip, rotate))
        htab_h, htab_d = _table(device, W, newW)
        vtab_h, vtab_d = _table(device, H, newH)
        c0, c1 = max(x0, 0), min(x0 + fW, newW)
        r0, r1 = max(y0, 0), min(y0 + fH, newH)
        if c1 > c0 and r1 > r0:
            rows = vtab_h[r0:r1]
            b0, b1 = int(rows[:, 0].min()), int((rows[:, 0] + rows[:, 1]).max())
        else:                                   # the crop misses the resized image: every pixel is fill
            c0 = c1 = 0
            b0 = b1 = 0
        rot = rotate_constants(rotate, fW, fH)
        r = recs[f]
        for k, v in (("htab", htab_d.data_ptr()), ("vtab", vtab_d.data_ptr()), ("hk", htab_h.shape[1] - _HEADER),
                     ("vk", vtab_h.shape[1] - _HEADER), ("rw", newW), ("rh", newH), ("cx", x0), ("cy", y0),
                     ("col0", c0), ("ncols", c1 - c0), ("band0", b0), ("band_rows", b1 - b0),
                     ("flip", int(flip)), ("rotate", 0 if rot is None else 1)):
            r[idx[k]] = v
        if rot is not None:
            r[idx["a0"]:idx["a5"] + 1] = rot
        bands.append((b0, b1 - b0))
    return recs, bands, np.stack(mats) if mats else np.zeros((0, 4, 4))


def _flat_augs(augs):
    """augs: one (resize, resize_dims, crop, flip, rotate) per frame, flat or nested like the frames' leading dims."""
    out = []

    def walk(a):
        if isinstance(a, (tuple, list)) and len(a) == 5 and isinstance(a[0], (int, float, np.number)):
            out.append(tuple(a))
        elif isinstance(a, (tuple, list, np.ndarray)):
            for b in a:
                walk(b)
        else:
            raise ValueError(f"not an augs tuple (resize, resize_dims, crop, flip, rotate): {a!r}")
    walk(augs)
    return out


def _affine_launch(img, img_bytes, H, W, row_stride, recs, final_dim, normalize, mean, std, to_rgb, channels_last,
                   device):
    fH, fW = final_dim
    N = recs.shape[0]
    idx = _FRAME_FIELDS.index
    ws_sizes = [(int(r[idx("band_rows")]) * ((int(r[idx("ncols")]) + 3) // 4 * 12) + 15) // 16 * 16 for r in recs]
    recs[:, idx("ws_off")] = np.concatenate([[0], np.cumsum(ws_sizes)[:-1]]) if N else []
    recs = np.ascontiguousarray(recs)
    lib = _lib.load()
    nbytes = int(lib.ud_image_affine_workspace_bytes(recs.ctypes.data, N))
    ws = _lib.workspace(device, nbytes, slot="image_affine")
    recs_d = torch.from_numpy(recs).to(device)
    if normalize:
        shape = (N, fH, fW, 3) if channels_last else (N, 3, fH, fW)
        out = torch.empty(shape, dtype=torch.float32, device=device)
        mode = 2 if channels_last else 1
    else:
        out = torch.empty((N, fH, fW, 3), dtype=torch.uint8, device=device)
        mode = 0
    import ctypes
    f3 = lambda v: (ctypes.c_float * 3)(*[float(a) for a in v])
    _lib.check(lib.ud_image_affine(img, img_bytes, H, W, row_stride, recs.ctypes.data, _lib.ptr(recs_d), N, fH, fW,
                                   mode, _lib.ptr(out), f3(mean), f3(std), 1 if to_rgb else 0, _lib.ptr(ws),
                                   ws.numel(), _lib.stream_of(out)), "ud_image_affine")
    if normalize and channels_last:
        out = out.permute(0, 3, 1, 2)              # [N, 3, fH, fW] view of the NHWC buffer
    return out


def image_affine(imgs_u8, augs, final_dim=(256, 704), normalize=True, mean=IMG_MEAN, std=IMG_STD, to_rgb=TO_RGB,
                 channels_last=False):
    """ImageAffineTransformation.forward (transforms3d.py:298-347 -> functional.img_transform) on the device, for
    uint8 frames imgs_u8 [..., H, W, 3] (rows may be strided; the 3 bytes of a pixel and the pixels of a row must be
    dense) and one augs tuple (resize, resize_dims, crop, flip, rotate) per frame, as sample_augs returns them.
    Returns (images, ida_mats): images uint8 [..., fH, fW, 3] bit-identical to PIL's, or with ``normalize`` the
    ImageNormalize output float32 [..., 3, fH, fW] fused into the same pass (``channels_last``: NHWC memory);
    ida_mats float64 [..., 4, 4] on the host, computed as img_transform computes them."""
    _lib.require_gpu(imgs_u8)
    if not torch.is_tensor(imgs_u8) or imgs_u8.dtype != torch.uint8 or imgs_u8.dim() < 3 or imgs_u8.shape[-1] != 3:
        raise ValueError("imgs_u8 must be a uint8 [..., H, W, 3] tensor")
    if imgs_u8.stride(-1) != 1 or imgs_u8.stride(-2) != 3:
        raise ValueError("imgs_u8 rows must hold dense RGB pixels (stride 3 between pixels, 1 between channels)")
    fH, fW = (int(v) for v in final_dim)
    if fH <= 0 or fW <= 0:
        raise ValueError("final_dim must be positive")
    lead, (H, W) = tuple(imgs_u8.shape[:-3]), tuple(imgs_u8.shape[-3:-1])
    N = int(np.prod(lead)) if lead else 1
    augs = _flat_augs(augs)
    if len(augs) != N:
        raise ValueError(f"{len(augs)} augs for {N} frames")
    if H == 0 or W == 0:
        raise ValueError("empty frames")
    recs, bands, mats = plan_frames(augs, H, W, (fH, fW), imgs_u8.device)
    idx = _FRAME_FIELDS.index
    if N:
        lead_strides = imgs_u8.stride()[:-3]
        offs = np.zeros(lead, np.int64)
        for d, (n, s) in enumerate(zip(lead, lead_strides)):
            offs = offs + (np.arange(n, dtype=np.int64) * s).reshape((n,) + (1,) * (len(lead) - d - 1))
        recs[:, idx("src_off")] = offs.reshape(-1)
        recs[:, idx("src_row0")] = 0
        recs[:, idx("src_rows")] = H
    img_bytes = 1 + sum((n - 1) * s for n, s in zip(imgs_u8.shape, imgs_u8.stride()))
    out = _affine_launch(_lib.ptr(imgs_u8), img_bytes, H, W, imgs_u8.stride(-3), recs, (fH, fW), normalize, mean, std,
                         to_rgb, channels_last, imgs_u8.device)
    if normalize:
        out = out.reshape(*lead, 3, fH, fW)
    else:
        out = out.reshape(*lead, fH, fW, 3)
    return out, mats.reshape(*lead, 4, 4)


def image_affine_host_frames(frames, augs, device, final_dim=(256, 704), **kw):
    """image_affine for frames in HOST memory (numpy / CPU tensor uint8 [..., H, W, 3], or a list of equally shaped
    ones, e.g. one per sample): only the source row band each frame's crop needs is packed into pinned memory and
    copied to ``device`` (HWC rows are contiguous), then one launch.  Same return values as image_affine."""
    if isinstance(frames, (list, tuple)):              # per-sample arrays: no stacked copy of whole frames
        parts = [np.asarray(f.numpy() if torch.is_tensor(f) else f) for f in frames]
        lead = (len(parts),) + (parts[0].shape[:-3] if parts else ())
    else:
        parts = [np.asarray(frames.numpy() if torch.is_tensor(frames) else frames)]
        lead = parts[0].shape[:-3]
    if not parts or any(p.dtype != np.uint8 or p.ndim < 3 or p.shape[-1] != 3 or p.shape[-3:] != parts[0].shape[-3:]
                        or p.shape[:-3] != parts[0].shape[:-3] for p in parts):
        raise ValueError("frames must be uint8 [..., H, W, 3] (a list: of equal shapes)")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("unidistill_amd ops run on the GPU only (no CPU fallback); got device " + str(device))
    H, W = parts[0].shape[-3:-1]
    flat = [f for p in parts for f in p.reshape(-1, H, W * 3)]
    N = len(flat)
    augs = _flat_augs(augs)
    if len(augs) != N:
        raise ValueError(f"{len(augs)} augs for {N} frames")
    fH, fW = (int(v) for v in final_dim)
    recs, bands, mats = plan_frames(augs, H, W, (fH, fW), device)
    row = W * 3
    total = sum(rows for _, rows in bands) * row
    host = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    idx = _FRAME_FIELDS.index
    off = 0
    for f, (b0, rows) in enumerate(bands):
        hv[off:off + rows * row] = flat[f][b0:b0 + rows].reshape(-1)
        recs[f, idx("src_off")], recs[f, idx("src_row0")], recs[f, idx("src_rows")] = off, b0, rows
        off += rows * row
    dev = host.to(device, non_blocking=True)
    out = _affine_launch(_lib.ptr(dev), dev.numel(), H, W, row, recs, (fH, fW), kw.get("normalize", True),
                         kw.get("mean", IMG_MEAN), kw.get("std", IMG_STD), kw.get("to_rgb", TO_RGB),
                         kw.get("channels_last", False), device)
    if kw.get("normalize", True):
        out = out.reshape(*lead, 3, fH, fW)
    else:
        out = out.reshape(*lead, fH, fW, 3)
    return out, mats.reshape(*lead, 4, 4)
