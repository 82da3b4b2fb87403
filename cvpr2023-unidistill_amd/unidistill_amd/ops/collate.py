"""Top layer of the input chain: collate_fn with the batch assembled on the device, and the routes that
sit above both the LiDAR chain and the GT-sampling paste."""
import ctypes

import numpy as np
import torch

from .. import _lib
from ..config import IMG_DIM
from .gt_paste import append_pasted, lidar_paste_host_clouds
from .image_affine import _flat_augs, image_affine, image_affine_host_frames, image_normalize
from .jpeg import JpegFrameError, jpeg_decode
from .lidar_prep import prep_host_clouds
from .staging import input_stream


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
    ptrs = (ctypes.c_void_p * B)(*[t.data_ptr() if t.numel() else None for t in dev_ts])
    rows = (ctypes.c_int64 * B)(*[n if t.numel() else 0 for n, t in zip(lens, dev_ts)])
    _lib.ud.ud_collate_pad(ptrs, rows, B, L, W, out, _lib.stream_of(out))
    return out


def lidar_prep_host_clouds(clouds, plans, device):
    """The reference's CollectLidarSweeps -> BevAffineTransformation -> ObjectRangeFilter on the points, then
    collate_fn's fill_batch_tensor, for host clouds: ``clouds`` one list per sample of float32 [Ni, D] arrays (key
    frame first, then its sweeps), ``plans`` the samples' data_dict["lidar_aug"] records (None: rows taken as they
    are).  All clouds are packed into a pinned buffer, copied in one H2D copy and processed in one fused pass on
    input_stream(device); the caller's current stream waits on the result.  -> float32 [B, Nmax, D] on ``device``,
    equal to fill_batch_tensor of the reference-processed clouds bit for bit.  When a plan carries a ``paste`` record
    (GTSampling) the batch goes through lidar_paste_host_clouds (ops/gt_paste.py), which also leaves each record's
    ``accept`` flags in it; a batch without one takes the paste-free route (ops/lidar_prep.py) unchanged."""
    if any(a is not None and a.get("paste") is not None for a in plans):      # GT sampling: DESIGN §2.16
        return lidar_paste_host_clouds(clouds, plans, device)[0]
    return prep_host_clouds(clouds, plans, device)


def _sample_augs(sample, key, frames, ida_transform):
    """The sample's ``ida_aug``, or one draw per frame from ``ida_transform``; flat, in frame order."""
    a = sample.get("ida_aug")
    if a is None:
        if ida_transform is None:
            raise ValueError(f"{key} needs ida_aug per sample or an ida_transform to draw it")
        a = [ida_transform.sample_augs() for _ in range(frames)]
    return _flat_augs(a)


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
            augs += _sample_augs(d, "imgs_raw", int(np.prod(f.shape[:-3])), ida_transform)
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
        a = _sample_augs(d, "imgs_jpeg", shape[0] * shape[1], ida_transform)
        if len(a) != shape[0] * shape[1]:
            raise ValueError(f"sample {b}: {len(a)} augs for {shape[0] * shape[1]} frames")
        augs += a
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
