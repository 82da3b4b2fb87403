"""Camera side of the input chain: ImageNormalize and ImageAffineTransformation on the device
(DESIGN §2.9)."""
import ctypes
import math

import numpy as np
import torch

from .. import _lib
from .staging import device_index

IMG_MEAN, IMG_STD, TO_RGB = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375), True    # base_nuscenes_cfg.py:31


def _f3(v):
    return (ctypes.c_float * 3)(*[float(a) for a in v])


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
    if channels_last:
        out = torch.empty((NI, H, W, 3), dtype=torch.float32, device=x.device)
    else:
        out = torch.empty((NI, 3, H, W), dtype=torch.float32, device=x.device)
    _lib.ud.ud_image_normalize(x, out, _f3(mean), _f3(std), 1 if to_rgb else 0, NI, H, W, 1 if channels_last else 0,
                               _lib.stream_of(x))
    if channels_last:
        out = out.permute(0, 3, 1, 2)              # [NI, 3, H, W] view of the NHWC buffer
    return out.reshape(*lead, 3, H, W)             # only splits the leading axis: a view in both layouts


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
    the object is ``forward``, the reference's call convention (transforms3d.Compose runs ``data_dict = t(data_dict)``
    on its nn.Modules); ``apply`` runs the transform on device frames (``image_affine``)."""

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

    __call__ = forward

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
        index = device_index(device)                     # 'cuda' means the current device: key the table by its index
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


def _affine_launch(img, img_bytes, H, W, row_stride, recs, mats, lead, final_dim, normalize, mean, std, to_rgb,
                   channels_last, device):
    """The launch both routes end in: ``recs`` complete but for ws_off.  -> (images [*lead, ...], ida_mats)."""
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
    _lib.ud.ud_image_affine(img, img_bytes, H, W, row_stride, recs.ctypes.data, recs_d, N, fH, fW, mode, out, _f3(mean),
                            _f3(std), 1 if to_rgb else 0, ws, ws.numel(), _lib.stream_of(out))
    if normalize and channels_last:
        out = out.permute(0, 3, 1, 2)              # [N, 3, fH, fW] view of the NHWC buffer
    out = out.reshape(*lead, 3, fH, fW) if normalize else out.reshape(*lead, fH, fW, 3)
    return out, mats.reshape(*lead, 4, 4)


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
    return _affine_launch(imgs_u8, img_bytes, H, W, imgs_u8.stride(-3), recs, mats, lead, (fH, fW), normalize, mean,
                          std, to_rgb, channels_last, imgs_u8.device)


def image_affine_host_frames(frames, augs, device, final_dim=(256, 704), normalize=True, mean=IMG_MEAN, std=IMG_STD,
                             to_rgb=TO_RGB, channels_last=False):
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
    device = _lib.require_gpu_device(device)
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
    return _affine_launch(dev, dev.numel(), H, W, row, recs, mats, lead, (fH, fW), normalize, mean, std, to_rgb,
                          channels_last, device)
