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
from .jpeg import JpegFrameError, jpeg_decode


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
    _lib.ud.ud_image_normalize(x, out, f3(mean), f3(std), 1 if to_rgb else 0, NI, H, W, 1 if channels_last else 0,
                               _lib.stream_of(x))
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
    _lib.ud.ud_collate_pad(ptrs, rows, B, L, W, out, _lib.stream_of(out))
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
    Samples without ``ida_aug`` draw theirs from ``ida_transform`` (an ImageAffineTransformation), camera by camera.
    A sample may carry its RAW clouds ``points_raw`` (key frame first, then its sweeps, float32 [Ni, D] arrays) with
    the ``lidar_aug`` record CollectLidarSweeps / BevAffineTransformation / ObjectRangeFilter leave in the loader:
    ``points`` is then built by lidar_prep_host_clouds, one H2D copy and one fused pass for the batch.  When that record
    holds a ``paste`` record (GTSampling, ops/gt_paste.py) the accepted database objects are pasted in the same pass
    and their boxes / labels are appended to the sample's ``gt_boxes`` / ``gt_labels`` (images are not edited).
    A sample may carry its camera frames as JPEG files ``imgs_jpeg`` ([sweeps][cams] of bytes, nested like imgs_raw)
    with ``ida_aug`` (or an ida_transform): they are decoded on the device (ops/jpeg.py, bit-exact to Pillow) and go
    through the same image_affine launch; a frame whose decode failed raises ValueError naming sample and camera."""
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
    if "imgs_jpeg" in data[0]:
        batch["imgs"], ida_mats = _collate_jpeg(data, device, ida_transform)
    if "points_raw" in data[0]:
        batch["points"] = lidar_prep_host_clouds([d["points_raw"] for d in data], [d.get("lidar_aug") for d in data],
                                                 device)
        if any(d.get("lidar_aug") is not None and d["lidar_aug"].get("paste") is not None for d in data):
            data = [append_pasted(d) for d in data]        # gt_boxes / gt_labels + the accepted candidates (§2.16)
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


def _collate_jpeg(data, device, ida_transform):
    """imgs_jpeg route of collate_fn: one jpeg_decode for the batch, the status read back once on the input stream,
    then image_affine on the decoded frames.  -> (imgs, ida_mats)."""
    nest, files, augs = None, [], []
    for b, d in enumerate(data):
        sweeps = d["imgs_jpeg"]
        shape = (len(sweeps), len(sweeps[0]) if len(sweeps) else 0)
        if nest is None:
            nest = shape
        if shape != nest or any(len(cams) != shape[1] for cams in sweeps) or not shape[0] or not shape[1]:
            raise ValueError("imgs_jpeg must be [sweeps][cams] of JPEG bytes, the same nesting in every sample")
        files += [f for cams in sweeps for f in cams]
        a = d.get("ida_aug")
        if a is None:
            if ida_transform is None:
                raise ValueError("imgs_jpeg needs ida_aug per sample or an ida_transform to draw it")
            a = [ida_transform.sample_augs() for _ in range(shape[0] * shape[1])]
        a = _flat_augs(a)
        if len(a) != shape[0] * shape[1]:
            raise ValueError(f"sample {b}: {len(a)} augs for {shape[0] * shape[1]} frames")
        augs += a
    device = torch.device(device)
    per = nest[0] * nest[1]
    name = lambda i: f"sample {i // per} sweep {i % per // nest[1]} camera {i % nest[1]}"
    try:
        frames, status = jpeg_decode(files, device)
    except JpegFrameError as e:
        raise ValueError(f"JPEG decode failed for {name(e.index)}: {e.reason}") from e
    s = input_stream(device)
    with torch.cuda.stream(s):       # the readback queues behind the decode only, not the training step
        st = status.to("cpu", non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(s)
    ev.synchronize()
    bad = np.nonzero(st.numpy())[0]
    if len(bad):
        where = ", ".join(f"{name(i)} (status {int(st[i])})" for i in bad)
        raise ValueError(f"JPEG decode failed for {where}")
    fdim = tuple(ida_transform.aug_conf["final_dim"]) if ida_transform is not None else IMG_DIM
    H, W = frames.shape[1:3]
    imgs, mats = image_affine(frames.view(len(data), nest[0], nest[1], H, W, 3), augs, final_dim=fdim)
    return imgs, torch.from_numpy(mats).to(device=device, dtype=torch.float32)


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
        """Draws per camera of data_dict["imgs"] (frames or their JPEG bytes: the values are not read), or of
        data_dict["imgs_jpeg"] when there is no "imgs"."""
        imgs = data_dict.get("imgs", None)
        if imgs is None:
            imgs = data_dict.get("imgs_jpeg", None)
        if imgs is not None:
            data_dict["ida_aug"], data_dict["ida_mat"] = {}, {}
            for cam in imgs.keys():
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
    _lib.ud.ud_image_affine(img, img_bytes, H, W, row_stride, recs.ctypes.data, recs_d, N, fH, fW, mode, out, f3(mean), f3(std),
                            1 if to_rgb else 0, ws, ws.numel(), _lib.stream_of(out))
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
    out = _affine_launch(imgs_u8, img_bytes, H, W, imgs_u8.stride(-3), recs, (fH, fW), normalize, mean, std,
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
    out = _affine_launch(dev, dev.numel(), H, W, row, recs, (fH, fW), kw.get("normalize", True),
                         kw.get("mean", IMG_MEAN), kw.get("std", IMG_STD), kw.get("to_rgb", TO_RGB),
                         kw.get("channels_last", False), device)
    if kw.get("normalize", True):
        out = out.reshape(*lead, 3, fH, fW)
    else:
        out = out.reshape(*lead, fH, fW, 3)
    return out, mats.reshape(*lead, 4, 4)


# ---- LiDAR input chain after collate -----------------------------------------------------------
# The reference's det augmentor runs CollectLidarSweeps -> BevAffineTransformation -> ObjectRangeFilter on every
# sample's points in the loader (transforms3d.py:379-443, :242-287).  Here the loader-side classes only draw the
# parameters, do the box-level work (a few dozen boxes) and record in data_dict["lidar_aug"] what the device must do
# with the points; collate_fn stages the raw clouds of the whole batch in pinned memory, copies them in one H2D copy
# and runs the per-point work in one fused pass (ud_lidar_prep_count + ud_lidar_prep_compact): sweep transform, BDA,
# range test, stable compaction and the zero-padded [B, Nmax, D] stack of fill_batch_tensor.
_SEG_PAR, _SMP_PAR, _MAX_SEG = 18, 24, 64          # include/unidistill_hip.h UD_LIDAR_*


def _align16(n):
    return (n + 15) // 16 * 16


def _lidar_tables(seg_rows, sample_nseg, seg_mats, seg_xform, seg_last, bdas, ranges):
    """Host plan of ud_lidar_prep_*: segment row offsets, per-sample segment offsets and the two parameter tables,
    packed into one byte buffer (16-byte aligned sections).  -> (bytes, {name: (offset, array)})."""
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
    parts, off = {}, 0
    for name, a in (("seg", seg), ("sseg", sseg), ("seg_par", sp), ("smp_par", bp)):
        parts[name] = (off, a)
        off = _align16(off + a.nbytes)
    buf = np.zeros(off, np.uint8)
    for o, a in parts.values():
        buf[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return buf, parts


def _lidar_run(pts_ptr, rows, D, parts, plan_base, device, stream, out_compact):
    """ud_lidar_prep_count -> counts read back (waits on ``stream`` only) -> ud_lidar_prep_compact, all on ``stream``
    (a torch.cuda.Stream, current while this runs).  -> (out, counts int64 numpy)."""
    lib = _lib.load()
    seg, sseg = parts["seg"][1], parts["sseg"][1]
    S, B = len(seg) - 1, len(sseg) - 1
    p = {k: plan_base + o for k, (o, _) in parts.items()}
    ws_bytes = int(lib.ud_lidar_prep_workspace_bytes(seg.ctypes.data, sseg.ctypes.data, S, B))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
    counts_d = torch.empty(max(B, 1), dtype=torch.int64, device=device)
    hs = stream.cuda_stream
    args = (pts_ptr, rows, D, seg.ctypes.data, sseg.ctypes.data, S, B, p["seg"], p["sseg"], p["seg_par"], p["smp_par"])
    _lib.ud.ud_lidar_prep_count(*args, counts_d, ws, ws_bytes, hs)
    counts_h = torch.empty(max(B, 1), dtype=torch.int64, pin_memory=True)
    counts_h.copy_(counts_d, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(stream)
    ev.synchronize()                                    # this stream's work only, not the caller's queue
    counts = counts_h.numpy()[:B].copy()
    nmax = int(counts.max()) if B else 0
    if out_compact:
        out = torch.empty((int(counts.sum()), D), dtype=torch.float32, device=device)
    else:
        out = torch.empty((B, nmax, D), dtype=torch.float32, device=device)
    out_rows = out.numel() // D
    _lib.ud.ud_lidar_prep_compact(*args, counts.ctypes.data, counts_d, nmax, 1 if out_compact else 0, out, out_rows, ws,
                                  ws_bytes, hs)
    return out, counts


def points_range_filter(points, point_cloud_range, seg=None):
    """ObjectRangeFilter.mask_points_by_range + indexing (transforms3d.py:248-255) for a device cloud points f32
    [rows, D]: keeps x in [r0, r3] and y in [r1, r4] (float32 compares, z untested, NaN dropped), in order.  ``seg``:
    row offsets of segments (S + 1 ints) filtered each on its own, e.g. the samples of a concatenated batch.
    -> (kept rows f32 [K, D], per-segment kept counts int64 numpy [S]).  Runs on the current stream."""
    _lib.require_gpu(points)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] < 3 or not points.is_contiguous():
        raise ValueError("points must be a contiguous float32 [rows, D >= 3] tensor")
    rows, D = points.shape
    seg = [0, rows] if seg is None else [int(v) for v in seg]
    if len(seg) < 1 or seg[0] != 0 or seg[-1] != rows or any(b < a for a, b in zip(seg, seg[1:])):
        raise ValueError("seg must ascend from 0 to the number of rows")
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

    def __call__(self, data_dict):
        return self.forward(data_dict)


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

    def __call__(self, data_dict):
        return self.forward(data_dict)


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

    def __call__(self, data_dict):
        return self.forward(data_dict)


_input_streams = {}       # device index -> torch.cuda.Stream for the input chain
_lidar_staging = {}       # device index -> [pinned uint8 buffer, event after its last H2D copy]


def _device_index(device):
    return device.index if device.index is not None else torch.cuda.current_device()


def input_stream(device):
    """The per-device stream the LiDAR input chain runs on: its H2D copy and passes never queue behind the training
    step on the caller's stream, so the count readback waits for them alone."""
    i = _device_index(device)
    s = _input_streams.get(i)
    if s is None:
        s = _input_streams[i] = torch.cuda.Stream(device=torch.device("cuda", i))
    return s


def _staging(i, nbytes):
    st = _lidar_staging.get(i)
    if st is None or st[0].numel() < nbytes:
        if st is not None:
            st[1].synchronize()
        st = _lidar_staging[i] = [torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True),
                                  torch.cuda.Event()]
        st[1].record(torch.cuda.current_stream(torch.device("cuda", i)))
    else:
        st[1].synchronize()                 # the previous batch's copy out of this buffer has finished
    return st


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


def lidar_prep_host_clouds(clouds, plans, device):
    """The reference's CollectLidarSweeps -> BevAffineTransformation -> ObjectRangeFilter on the points, then
    collate_fn's fill_batch_tensor, for host clouds: ``clouds`` one list per sample of float32 [Ni, D] arrays (key
    frame first, then its sweeps), ``plans`` the samples' data_dict["lidar_aug"] records (None: rows taken as they
    are).  All clouds are packed into a pinned buffer, copied in one H2D copy and processed in one fused pass on
    input_stream(device); the caller's current stream waits on the result.  -> float32 [B, Nmax, D] on ``device``,
    equal to fill_batch_tensor of the reference-processed clouds bit for bit.  When a plan carries a ``paste`` record
    (GTSampling) the batch goes through lidar_paste_host_clouds (ops/gt_paste.py), which also leaves each record's
    ``accept`` flags in it; a batch without one takes the path below unchanged."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("unidistill_amd ops run on the GPU only (no CPU fallback); got device " + str(device))
    arrs, D = _host_clouds(clouds, plans)
    if any(a is not None and a.get("paste") is not None for a in plans):      # GT sampling: DESIGN §2.16
        return lidar_paste_host_clouds(clouds, plans, device)[0]
    flat = [a for cs in arrs for a in cs]
    seg_rows, nseg, mats, xform, last, bdas, ranges = [], [], [], [], [], [], []
    for cs, aug in zip(arrs, plans):
        m, x, l, bda, rg = _plan_segments(cs, aug, D)
        seg_rows += [len(a) for a in cs]
        nseg.append(len(cs))
        mats += m
        xform += x
        last += l
        bdas.append(bda)
        ranges.append(rg)
    plan, parts = _lidar_tables(seg_rows, nseg, mats, xform, last, bdas, ranges)
    rows = int(sum(seg_rows))
    pts_bytes = _align16(rows * D * 4)
    i = _device_index(device)
    device = torch.device("cuda", i)
    host, copied = _staging(i, pts_bytes + plan.nbytes)
    hv = host.numpy()
    fv = hv[:rows * D * 4].view(np.float32)
    off = 0
    for a in flat:
        fv[off:off + a.size] = a.reshape(-1)
        off += a.size
    hv[pts_bytes:pts_bytes + plan.nbytes] = plan
    cur = torch.cuda.current_stream(device)
    s = input_stream(device)
    with torch.cuda.stream(s):
        dev = torch.empty(pts_bytes + plan.nbytes, dtype=torch.uint8, device=device)
        dev.copy_(host[:dev.numel()], non_blocking=True)
        copied.record(s)
        out, _ = _lidar_run(dev.data_ptr(), rows, D, parts, dev.data_ptr() + pts_bytes, device, s, False)
        done = torch.cuda.Event()
        done.record(s)
    cur.wait_event(done)
    out.record_stream(cur)
    return out


# ---- GT-sampling (database paste) in that chain: ops/gt_paste.py ----------------------------------
from .gt_paste import (GTSampling, ObjectDatabase, append_pasted, gt_paste,          # noqa: E402,F401
                       lidar_paste_host_clouds)
