"""GT-sampling (database paste) for the device LiDAR input chain.

The reference's GTSampling (transforms3d.py:162-207 -> OpenPCDet's DataBaseSampler) sits between CollectLidarSweeps and
BevAffineTransformation.  Split as the other LiDAR transforms are: in the loader ``GTSampling`` only draws candidate
indices (host, a handful of integers) and records them in data_dict["lidar_aug"]["paste"]; after collate one tiny launch
(ud_gt_paste_select) decides which candidates collide with nothing, and the fused chain (ud_lidar_paste_count /
ud_lidar_paste_compact) reads the accepted objects' clouds straight out of the device-resident ``ObjectDatabase``,
drops the scene's points inside their boxes and goes on with BDA, range filter, compaction and padding as before.
Images are not edited (the reference's MultiModalGTSampling is a no-op too): a camera branch sees the unpasted scene.

The database itself is built here too: ``ObjectDatabaseBuilder`` is OpenPCDet's
create_groundtruth_database on the device -- ``points_in_boxes`` (ud_points_in_boxes) over whole scenes, then a stable
per-object compaction (ud_gt_db_count / ud_gt_db_extract) -- and ``ObjectDatabase.save`` / ``load`` keep it in one .npz.
"""
import numpy as np
import torch

from .. import _lib
from . import lidar_prep as lp
from .staging import align16, staged_upload

MAX_CAND = 63            # include/unidistill_hip.h UD_GT_PASTE_MAX_CAND


def _parse_cfg(entries):
    """["car:5", ...] -> [("car", 5), ...]"""
    out = []
    for e in entries or []:
        name, num = str(e).split(":")
        out.append((name, int(num)))
    return out


class ObjectDatabase:
    """The ground-truth database of OpenPCDet's create_groundtruth_database, resident on the device: every object's
    box-centred cloud back to back in ``points`` f32 [P, D], ``offsets`` int64 [N + 1] (object i = rows offsets[i] ..
    offsets[i+1]), ``boxes`` f32 [N, W >= 7] with every column kept (velocity included) and ``class_ids`` int64 [N]
    into ``class_names``.  boxes / offsets / class_ids are held on the host as well (numpy: the sampler and the collate
    read a few dozen of them per sample) and on the device (``boxes_d``, ``offsets_d``, ``class_ids_d``).  Pickling a
    database (a loader worker returning a paste record) sends its name only; the receiving process must hold a database
    of that name."""

    _registry = {}

    def __init__(self, points, offsets, boxes, class_ids, class_names, device="cuda", name=None):
        pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points, np.float32))
        if pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] < 3:
            raise ValueError("points must be float32 [P, D >= 3]")
        self.offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        self.boxes = np.ascontiguousarray(boxes, np.float32)
        self.class_ids = np.ascontiguousarray(class_ids, np.int64).reshape(-1)
        self.class_names = [str(c) for c in class_names]
        n = len(self.class_ids)
        if self.boxes.ndim != 2 or self.boxes.shape[1] < 7 or self.boxes.shape[0] != n or len(self.offsets) != n + 1:
            raise ValueError("boxes must be [N, >= 7], class_ids [N], offsets [N + 1]")
        if self.offsets[0] != 0 or self.offsets[-1] != pts.shape[0] or (np.diff(self.offsets) < 0).any():
            raise ValueError("offsets must ascend from 0 to the number of points")
        if n and (self.class_ids.min() < 0 or self.class_ids.max() >= len(self.class_names)):
            raise ValueError("class_ids must index class_names")
        device = torch.device(device)
        self.points = pts.to(device).contiguous()
        self.boxes_d = torch.from_numpy(self.boxes).to(device)
        self.offsets_d = torch.from_numpy(self.offsets).to(device)
        self.class_ids_d = torch.from_numpy(self.class_ids).to(device)
        self.name = name if name is not None else f"db{len(ObjectDatabase._registry)}"
        ObjectDatabase._registry[self.name] = self

    @staticmethod
    def lookup(name):
        return ObjectDatabase._registry[name]

    def __reduce__(self):
        return ObjectDatabase.lookup, (self.name,)

    def __len__(self):
        return len(self.class_ids)

    @property
    def D(self):
        return int(self.points.shape[1])

    @property
    def rows(self):
        return np.diff(self.offsets)

    def indices_of(self, class_name):
        """Database indices of one class, ascending."""
        if class_name not in self.class_names:
            return np.zeros(0, np.int64)
        return np.nonzero(self.class_ids == self.class_names.index(class_name))[0]

    @classmethod
    def from_arrays(cls, points, offsets, boxes, class_ids, class_names, device="cuda", filter_by_min_points_cfg=None,
                    num_points=None, name=None):
        """``filter_by_min_points_cfg`` (["car:5", ...], OpenPCDet's filter_by_min_points) drops, at construction, the
        objects of a named class with fewer points than its threshold; ``num_points`` is the dbinfos' num_points_in_gt
        (default: the stored rows)."""
        pts = points.cpu().numpy() if torch.is_tensor(points) else np.asarray(points, np.float32)
        offsets = np.asarray(offsets, np.int64).reshape(-1)
        boxes, class_ids = np.asarray(boxes, np.float32), np.asarray(class_ids, np.int64).reshape(-1)
        class_names = [str(c) for c in class_names]
        rows = np.diff(offsets)
        npts = rows if num_points is None else np.asarray(num_points, np.int64).reshape(-1)
        keep = np.ones(len(class_ids), bool)
        for cname, least in _parse_cfg(filter_by_min_points_cfg):
            if cname in class_names:
                keep &= ~((class_ids == class_names.index(cname)) & (npts < least))
        if not keep.all():
            sel = np.nonzero(keep)[0]
            pts = np.concatenate([pts[offsets[i]:offsets[i + 1]] for i in sel]) if len(sel) else pts[:0]
            offsets = np.concatenate([[0], np.cumsum(rows[sel])]).astype(np.int64)
            boxes, class_ids = boxes[sel], class_ids[sel]
        return cls(np.ascontiguousarray(pts, np.float32), offsets, boxes, class_ids, class_names, device, name)

    @classmethod
    def from_infos(cls, db_infos, load_points, class_names=None, device="cuda", filter_by_min_points_cfg=None,
                   name=None):
        """OpenPCDet's dbinfos layout {class: [{"box3d_lidar", "num_points_in_gt", "path", ...}]}; ``load_points(info)``
        returns the object's box-centred float32 [n, D] cloud (e.g. np.fromfile(root / info["path"]).reshape(-1, D))."""
        class_names = list(db_infos.keys()) if class_names is None else [str(c) for c in class_names]
        clouds, boxes, ids, npts = [], [], [], []
        for k, cname in enumerate(class_names):
            for info in db_infos.get(cname, []):
                clouds.append(np.asarray(load_points(info), np.float32))
                boxes.append(np.asarray(info["box3d_lidar"], np.float32))
                ids.append(k)
                npts.append(int(info.get("num_points_in_gt", len(clouds[-1]))))
        if not clouds:
            raise ValueError("db_infos holds no object of class_names")
        offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
        return cls.from_arrays(np.concatenate(clouds), offsets, np.stack(boxes), ids, class_names, device,
                               filter_by_min_points_cfg, npts, name)

    def save(self, path):
        """The whole database as one .npz at ``path`` (written as given, no suffix added): points, offsets, boxes,
        class_ids, class_names.  ``load`` gives it back bit for bit."""
        with open(path, "wb") as f:
            np.savez(f, points=self.points.cpu().numpy(), offsets=self.offsets, boxes=self.boxes,
                     class_ids=self.class_ids, class_names=np.array(self.class_names, dtype=np.str_))

    @classmethod
    def load(cls, path, device="cuda", name=None):
        with np.load(path, allow_pickle=False) as z:
            return cls(z["points"], z["offsets"], z["boxes"], z["class_ids"], [str(c) for c in z["class_names"]], device,
                       name)


# ---- building the database on the device --------------------------------------------------------------
def _scene_offsets(points, seg, boxes, box_off):
    """Checks the scenes' layout.  -> (seg, box_off) as contiguous int64 numpy arrays of B + 1 entries."""
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] < 3 or (
            points.shape[0] > 1 and points.stride(1) != 1) or points.stride(0) < points.shape[1]:
        raise ValueError("points must be a float32 [rows, D >= 3] tensor with unit column stride")
    if boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] < 7 or not boxes.is_contiguous():
        raise ValueError("boxes must be a contiguous float32 [M, W >= 7] tensor")
    seg = np.ascontiguousarray([0, points.shape[0]] if seg is None else seg, np.int64).reshape(-1)
    if box_off is None:
        if len(seg) != 2:
            raise ValueError("box_off may be omitted for a single scene only")
        box_off = [0, boxes.shape[0]]
    box_off = np.ascontiguousarray(box_off, np.int64).reshape(-1)
    if len(seg) < 2 or seg[0] != 0 or seg[-1] != points.shape[0] or (np.diff(seg) < 0).any():
        raise ValueError("seg must ascend from 0 to the number of rows")
    if len(box_off) != len(seg) or box_off[0] != 0 or box_off[-1] != boxes.shape[0] or (np.diff(box_off) < 0).any():
        raise ValueError("box_off must have one entry per seg entry and ascend from 0 to the number of boxes")
    return seg, box_off


def _owner_launch(points, seg, boxes, box_off, out=None):
    """ud_points_in_boxes on the current stream.  -> (owner int32 [rows], device offsets (seg, box_off))."""
    rows, D = points.shape
    B = len(seg) - 1
    offs_d = torch.from_numpy(np.concatenate([seg, box_off])).to(points.device)
    seg_d, box_off_d = offs_d[:B + 1], offs_d[B + 1:]
    owner = torch.empty(rows, dtype=torch.int32, device=points.device) if out is None else out
    if owner.dtype != torch.int32 or owner.shape != (rows,) or not owner.is_contiguous() or owner.device != points.device:
        raise ValueError("out must be a contiguous int32 [rows] tensor on the points' device")
    _lib.ud.ud_points_in_boxes(points, rows, D, points.stride(0) if rows > 1 else D, seg.ctypes.data, seg_d, boxes,
                               boxes.shape[1], boxes.shape[1], box_off.ctypes.data, box_off_d, B, owner,
                               _lib.stream_of(points))
    return owner, (seg_d, box_off_d)


def _device_boxes(boxes, device):
    if torch.is_tensor(boxes):
        return boxes.to(device=device, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(boxes, np.float32)).to(device)


def points_in_boxes(points, seg, boxes, box_off=None, out=None):
    """OpenPCDet's points_in_boxes_gpu for scenes lying back to back: ``points`` f32 [rows, D >= 3] on the GPU, ``seg``
    the scenes' row offsets (B + 1 ints), ``boxes`` f32 [Mtot, W >= 7] (a device tensor or a host array), ``box_off``
    the scenes' box offsets; for a single scene ``seg`` and ``box_off`` may be None.  -> owner int32 [rows]: the index,
    within its scene, of the lowest-numbered box that contains the row, or -1 (the paste's inside test, float32; a
    non-finite box contains nothing, a non-finite row gets -1).  One launch on the current stream, no host wait;
    ``out``: the int32 tensor to fill."""
    _lib.require_gpu(points)
    boxes = _device_boxes(boxes, points.device)
    seg, box_off = _scene_offsets(points, seg, boxes, box_off)
    return _owner_launch(points, seg, boxes, box_off, out)[0]


def _extract_objects(points, seg, boxes, box_off):
    """Every box's points as a box-centred cloud: ud_points_in_boxes, ud_gt_db_count -> ONE readback of the counts ->
    ud_gt_db_extract, the shape of lidar_prep._two_pass, on the current stream.
    -> (clouds f32 [total, D] in (scene, box) order, rows per box int64 numpy [Mtot])."""
    rows, D = points.shape
    M, W = boxes.shape
    B = len(seg) - 1
    device = points.device
    stream = torch.cuda.current_stream(device)
    hs = stream.cuda_stream
    owner, (seg_d, box_off_d) = _owner_launch(points, seg, boxes, box_off)
    ws_bytes = int(_lib.load().ud_gt_db_workspace_bytes(rows, M))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
    counts_d = torch.empty(M + 1, dtype=torch.int64, device=device)
    _lib.ud.ud_gt_db_count(owner, rows, seg.ctypes.data, seg_d, box_off.ctypes.data, box_off_d, B, counts_d, ws, ws_bytes,
                           hs)
    counts_h = torch.empty(M + 1, dtype=torch.int64, pin_memory=True)
    counts_h.copy_(counts_d, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(stream)
    ev.synchronize()                                    # this stream's work only
    counts = counts_h.numpy().copy()
    out = torch.empty((int(counts[-1]), D), dtype=torch.float32, device=device)
    _lib.ud.ud_gt_db_extract(points, rows, D, points.stride(0) if rows > 1 else D, boxes, W, W, M, counts.ctypes.data, out,
                             out.shape[0], ws, ws_bytes, hs)
    return out, counts[:-1]


class ObjectDatabaseBuilder:
    """OpenPCDet's create_groundtruth_database on the device: per scene, which of ALL its boxes owns each point
    (points_in_boxes; the lowest index wins a shared point), then every box's points with the box centre subtracted.
    Afterwards the objects whose name is not in ``class_names`` (or not in ``used_classes``, when given) are left out --
    an ignored box still owns its points.  A box without points stays, with zero rows.  ``finish`` gives the
    device-resident ``ObjectDatabase`` the sampler and the paste read; the clouds never visit the host."""

    def __init__(self, class_names, device="cuda", used_classes=None):
        self.class_names = [str(c) for c in class_names]
        self.used_classes = None if used_classes is None else {str(c) for c in used_classes}
        self.device = torch.device(device)
        self.D = self.W = None
        self.scenes = 0
        self._clouds, self._rows, self._boxes, self._names, self._image_idx, self._gt_idx = [], [], [], [], [], []

    def _check_scene(self, scene, D, W):
        """One scene's arguments, host only.  -> (points, boxes f32 numpy [M, W], names object array [M], D, W)."""
        points, boxes = scene["points"], scene["gt_boxes"]
        names, labels = scene.get("gt_names"), scene.get("gt_labels")
        if (names is None) == (labels is None):
            raise ValueError("pass exactly one of gt_names and gt_labels")
        if not torch.is_tensor(points):
            points = np.asarray(points)
        f32 = torch.float32 if torch.is_tensor(points) else np.float32
        if points.ndim != 2 or points.shape[1] < 3 or points.dtype != f32:
            raise ValueError("points must be float32 [N, D >= 3]")
        if D is not None and points.shape[1] != D:
            raise ValueError(f"points have {points.shape[1]} columns, the scenes before {D}")
        boxes = np.asarray(boxes.cpu() if torch.is_tensor(boxes) else boxes, np.float32)
        boxes = boxes.reshape(0, W or 7) if boxes.size == 0 and boxes.ndim != 2 else boxes
        if boxes.ndim != 2 or boxes.shape[1] < 7:
            raise ValueError("gt_boxes must be [M, W >= 7]")
        if W is not None and boxes.shape[1] != W:
            raise ValueError(f"gt_boxes have {boxes.shape[1]} columns, the scenes before {W}")
        if names is None:
            labels = np.asarray(labels).reshape(-1)
            if len(labels) and (not np.issubdtype(labels.dtype, np.integer) or labels.min() < 0
                                or labels.max() >= len(self.class_names)):
                raise ValueError(f"unknown label: gt_labels must be integers in 0 .. {len(self.class_names) - 1}")
            names = np.asarray(self.class_names, object)[labels.astype(np.int64)]
        names = np.asarray([str(n) for n in np.asarray(names, object).reshape(-1)], object)
        if len(names) != len(boxes):
            raise ValueError(f"{len(boxes)} boxes, {len(names)} names / labels")
        return points, boxes, names, points.shape[1], boxes.shape[1]

    def add_scene(self, points, gt_boxes, gt_names=None, gt_labels=None, sample_idx=None):
        """One scene: ``points`` [N, D] (a device tensor or a host array; the sweeps already merged into the key frame),
        ``gt_boxes`` [M, W >= 7] with every column kept, exactly one of ``gt_names`` / ``gt_labels`` (indices into
        class_names), ``sample_idx`` for infos()["image_idx"] (default: the scene's running number)."""
        self.add_scenes([{"points": points, "gt_boxes": gt_boxes, "gt_names": gt_names, "gt_labels": gt_labels,
                          "sample_idx": sample_idx}])

    def add_scenes(self, scenes):
        """Several scenes (dicts with add_scene's arguments as keys) in one launch group with one readback."""
        D, W, checked = self.D, self.W, []
        for scene in scenes:                                # every argument check comes before any device work
            pts, boxes, names, D, W = self._check_scene(scene, D, W)
            checked.append((pts, boxes, names, scene.get("sample_idx")))
        if not checked:
            return
        device = _lib.require_gpu_device(self.device)
        clouds = []
        for pts, *_ in checked:
            if torch.is_tensor(pts) and pts.is_cuda:
                clouds.append(pts)
            else:
                clouds.append((pts if torch.is_tensor(pts) else torch.from_numpy(np.ascontiguousarray(pts))).to(device))
        points = clouds[0] if len(clouds) == 1 else torch.cat(clouds)
        if points.shape[0] > 1 and points.stride(1) != 1:
            points = points.contiguous()
        boxes = np.concatenate([b for _, b, _, _ in checked])
        seg = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
        box_off = np.concatenate([[0], np.cumsum([len(b) for _, b, _, _ in checked])]).astype(np.int64)
        with torch.cuda.device(points.device):
            out, rows = _extract_objects(points, seg, torch.from_numpy(boxes).to(points.device), box_off)
        self.D, self.W = D, W
        self._clouds.append(out)
        self._rows.append(rows)
        self._boxes.append(boxes)
        for _, b, names, idx in checked:
            self._names.append(names)
            self._image_idx.append(np.full(len(b), self.scenes if idx is None else idx, object))
            self._gt_idx.append(np.arange(len(b)))
            self.scenes += 1

    def _objects(self):
        """-> (rows, boxes, names, class ids, class-filter mask) of every box added so far, in (scene, box) order."""
        if not self._clouds:
            raise ValueError("no scene has been added")
        names = np.concatenate(self._names)
        ids = np.array([self.class_names.index(n) if n in self.class_names else -1 for n in names], np.int64)
        keep = ids >= 0
        if self.used_classes is not None:
            keep &= np.array([n in self.used_classes for n in names], bool)
        return np.concatenate(self._rows), np.concatenate(self._boxes), names, ids, keep

    def infos(self):
        """OpenPCDet's dbinfos layout {class: [{"name", "image_idx", "gt_idx", "box3d_lidar", "num_points_in_gt"}]} of
        the objects kept by the class filter (no "path": the clouds are in the database, not in files)."""
        rows, boxes, names, _, keep = self._objects()
        image_idx, gt_idx = np.concatenate(self._image_idx), np.concatenate(self._gt_idx)
        out = {}
        for i in np.nonzero(keep)[0]:
            out.setdefault(str(names[i]), []).append({"name": str(names[i]), "image_idx": image_idx[i],
                                                      "gt_idx": int(gt_idx[i]), "box3d_lidar": boxes[i].copy(),
                                                      "num_points_in_gt": int(rows[i])})
        return out

    def finish(self, filter_by_min_points_cfg=None, name=None):
        """-> the ObjectDatabase of the kept objects: the class filter, then ``filter_by_min_points_cfg`` (["car:5",
        ...]: the objects of a named class with fewer points are dropped, as ObjectDatabase.from_arrays does).  The
        clouds stay on the device; offsets, boxes and class ids are host arrays."""
        rows, boxes, _, ids, keep = self._objects()
        for cname, least in _parse_cfg(filter_by_min_points_cfg):
            if cname in self.class_names:
                keep &= ~((ids == self.class_names.index(cname)) & (rows < least))
        points = self._clouds[0] if len(self._clouds) == 1 else torch.cat(self._clouds)
        if not keep.all():
            points = points[torch.from_numpy(np.repeat(keep, rows)).to(points.device)]
        offsets = np.concatenate([[0], np.cumsum(rows[keep])]).astype(np.int64)
        return ObjectDatabase(points, offsets, boxes[keep], ids[keep], self.class_names, points.device, name)


class GTSampling:
    """GTSampling (transforms3d.py:162-207) split for the device: ``set_epoch`` / ``forward`` / ``stop_epoch`` as the
    reference (the identity from epoch + 1 >= stop_epoch on, and when ``points`` is absent).  In the loader it does the
    host part of DataBaseSampler only: per ``sampler_groups`` entry ("class:N") it draws N candidates -- max(0, N minus
    the class's boxes in the scene) with ``limit_whole_scene`` -- from a per-class shuffled index list with a moving
    pointer, reshuffled when exhausted (sample_with_fixed_number), with its own numpy Generator.  It records in
    data_dict["lidar_aug"]["paste"] the candidates' database indices, groups and labels, a copy of the pre-BDA gt_boxes,
    remove_extra_width and the database; ``points`` and ``gt_boxes`` are not changed.  Collision selection, point
    removal, paste and the appended boxes happen after collate (collate_fn / lidar_prep_host_clouds).  Must run before
    BevAffineTransformation and ObjectRangeFilter."""

    def __init__(self, database, class_names, sampler_groups, remove_extra_width=(0, 0, 0), limit_whole_scene=False,
                 stop_epoch=None, seed=None, use_road_plane=False):
        if use_road_plane:
            raise NotImplementedError("GTSampling: use_road_plane is not supported")
        self.database = database
        self.class_names = [str(c) for c in class_names]
        self.groups = [(g, name, num) for g, (name, num) in enumerate(_parse_cfg(sampler_groups))
                       if name in self.class_names]
        if sum(num for _, _, num in self.groups) > MAX_CAND:
            raise ValueError(f"sampler_groups ask for {sum(num for _, _, num in self.groups)} candidates per scene, "
                             f"the device selection takes at most {MAX_CAND}")
        self.remove_extra_width = tuple(float(v) for v in remove_extra_width)
        if len(self.remove_extra_width) != 3:
            raise ValueError("remove_extra_width needs three values")
        self.limit_whole_scene = bool(limit_whole_scene)
        self.stop_epoch = stop_epoch
        self.epoch = -1
        self.rng = np.random.default_rng(seed)
        # sample_with_fixed_number's state per class: the pointer starts past the end, so the first draw shuffles
        self.state = {}
        for _, name, _ in self.groups:
            ids = database.indices_of(name)
            self.state[name] = {"ids": ids, "pointer": len(ids), "indices": np.arange(len(ids))}

    def set_epoch(self, epoch):
        self.epoch = epoch

    def sample_with_fixed_number(self, class_name, num):
        """OpenPCDet's draw: a slice of the class's shuffled list at the pointer (short at the end of the list), the
        list reshuffled first when the pointer has reached its end.  -> database indices."""
        st = self.state[class_name]
        if st["pointer"] >= len(st["ids"]):
            st["indices"] = self.rng.permutation(len(st["ids"]))
            st["pointer"] = 0
        take = st["indices"][st["pointer"]:st["pointer"] + num]
        st["pointer"] += num
        return st["ids"][take]

    def _scene_counts(self, data_dict):
        names = data_dict.get("gt_names", None)
        if names is not None:
            names = np.asarray(names)
            return {n: int((names == n).sum()) for _, n, _ in self.groups}
        labels = data_dict.get("gt_labels", None)
        if labels is None:
            return {n: 0 for _, n, _ in self.groups}
        labels = np.asarray(labels)
        return {n: int((labels == self.class_names.index(n)).sum()) for _, n, _ in self.groups}

    def forward(self, data_dict):
        if self.stop_epoch is not None and (self.epoch + 1) >= self.stop_epoch:
            return data_dict
        if data_dict.get("points", None) is None:
            return data_dict
        a = lp._lidar_aug(data_dict)
        if a.get("bda_mat") is not None or a.get("range") is not None:
            raise ValueError("GTSampling must come before BevAffineTransformation and ObjectRangeFilter")
        counts = self._scene_counts(data_dict) if self.limit_whole_scene else None
        idx, grp = [], []
        for g, name, num in self.groups:
            n = max(0, num - counts[name]) if counts is not None else num
            if n <= 0 or len(self.state[name]["ids"]) == 0:
                continue
            got = self.sample_with_fixed_number(name, n)
            idx.append(got)
            grp.append(np.full(len(got), g, np.int32))
        idx = np.concatenate(idx).astype(np.int64) if idx else np.zeros(0, np.int64)
        grp = np.concatenate(grp) if grp else np.zeros(0, np.int32)
        db_names = np.asarray(self.database.class_names, object)[self.database.class_ids[idx]]
        a["paste"] = {"database": self.database, "cand_idx": idx, "cand_group": grp,
                      "cand_labels": np.array([self.class_names.index(n) for n in db_names], np.int64),
                      "gt_boxes": np.array(data_dict.get("gt_boxes", np.zeros((0, 7), np.float32)), np.float32,
                                           copy=True),
                      "remove_extra_width": self.remove_extra_width}
        return data_dict

    __call__ = forward


def check_segments(sweeps, candidates, sample=None):
    """The chain takes UD_LIDAR_MAX_SEGMENTS = 64 segments per sample: key frame + sweeps + candidates."""
    where = "" if sample is None else f"sample {sample}: "
    if candidates > MAX_CAND:
        raise ValueError(f"{where}{candidates} candidates, the device selection takes at most {MAX_CAND}")
    if 1 + sweeps + candidates > lp._MAX_SEG:
        raise ValueError(f"{where}1 key frame + {sweeps} sweeps + {candidates} candidates = "
                         f"{1 + sweeps + candidates} segments, the chain takes at most {lp._MAX_SEG}")


def _paste_plan(scenes, pastes, D):
    """Host plan of a paste batch.  scenes: per sample (rows per scene segment, matrices, transform flags, last-column
    values, BDA, range) as _plan_segments gives them; pastes: per sample the paste record or None.  Object segments go
    ahead of the sample's scene segments.  -> (packed plan with the pointers still relative, its parts, ncmax, scene
    rows); the ``pseg`` rows are (src, gate, object): src of an object segment is absolute (the database), src of a scene
    segment is the byte offset of its first row inside the scene buffer, gate the byte offset inside the accept block."""
    B = len(scenes)
    ncs = [0 if p is None else len(p["cand_idx"]) for p in pastes]
    for b, ((rows, *_), nc) in enumerate(zip(scenes, ncs)):
        check_segments(len(rows) - 1, nc, b)
    ncmax = max(ncs) if ncs else 0
    seg_rows, nseg, mats, xform, last, bdas, ranges, pseg = [], [], [], [], [], [], [], []
    gts, cands, rms, groups = [], [], [], []
    scene_row = 0
    for b, ((rows, m, x, l, bda, rg), p) in enumerate(zip(scenes, pastes)):
        if p is not None and ncs[b]:
            db = p["database"]
            if db.D != D:
                raise ValueError(f"the database's clouds have {db.D} columns, the scene's {D}")
            _lib.require_gpu(db.points)
            idx = np.asarray(p["cand_idx"], np.int64)
            boxes = db.boxes[idx, :7]
            for c, i in enumerate(idx):
                t = np.eye(4)
                t[:3, 3] = boxes[c, :3]                         # database clouds are box-centred
                mats.append(t)
                pseg.append((db.points.data_ptr() + int(db.offsets[i]) * D * 4, 1 + b * ncmax + c, 1))
            seg_rows += [int(v) for v in db.rows[idx]]
            xform += [True] * ncs[b]
            last += [np.nan] * ncs[b]                           # the time-lag column is kept as stored
            rm = boxes.copy()
            rm[:, 3:6] += np.asarray(p["remove_extra_width"], np.float32)
            cands.append(boxes)
            rms.append(rm)
            groups.append(np.asarray(p["cand_group"], np.int32))
        g = np.zeros((0, 7), np.float32) if p is None else np.asarray(p["gt_boxes"], np.float32)
        gts.append(g[:, :7] if g.ndim == 2 and len(g) else np.zeros((0, 7), np.float32))
        for r in rows:
            pseg.append((scene_row * D * 4, 0, 0))
            scene_row += int(r)
        seg_rows += [int(r) for r in rows]
        nseg.append(ncs[b] + len(rows))
        mats += list(m)
        xform += list(x)
        last += list(l)
        bdas.append(bda)
        ranges.append(rg)
    cat = lambda xs, w, dt: np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros((0,) + w, dt), dt)
    off = lambda ns: np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    arrays = lp._lidar_arrays(seg_rows, nseg, mats, xform, last, bdas, ranges)
    arrays += [("pseg", np.array(pseg, np.int64).reshape(-1, 3)), ("gt", cat(gts, (7,), np.float32)),
               ("gt_off", off([len(g) for g in gts])), ("cand", cat(cands, (7,), np.float32)),
               ("cand_off", off(ncs)), ("cand_group", cat(groups, (), np.int32)), ("rm", cat(rms, (7,), np.float32))]
    return (*lp._pack(arrays), ncmax, scene_row)


def _resolve(plan, parts, scene_ptr, accept_ptr):
    """Turns the relative pointers of the packed plan's ``pseg`` section into addresses, in place (gate 0 = no gate;
    stored offsets are 1-based)."""
    o, a = parts["pseg"]
    pseg = plan[o:o + a.nbytes].view(np.int64).reshape(-1, 3)
    scene = pseg[:, 2] == 0
    pseg[scene, 0] += scene_ptr
    pseg[~scene, 1] += accept_ptr - 1


def _paste_run(D, parts, plan_base, B, ncmax, result_d, device, stream, out_compact):
    """ud_gt_paste_select, then the chain's two passes (lidar_prep._two_pass) with ud_lidar_paste_count /
    ud_lidar_paste_compact: ONE readback of ``result_d`` = [counts | accept bytes], all on ``stream`` (current while
    this runs).  -> (out, counts int64 numpy [B], accept uint8 numpy [B, ncmax])."""
    gt_off, cand_off = parts["gt_off"][1], parts["cand_off"][1]
    args, ws, p = lp._chain_setup(None, int(parts["seg"][1][-1]), D, parts, plan_base, device)
    accept_ptr = result_d.data_ptr() + 8 * B
    _lib.ud.ud_gt_paste_select(p["gt"], gt_off.ctypes.data, p["gt_off"], p["cand"], p["cand_group"],
                               cand_off.ctypes.data, p["cand_off"], B, accept_ptr, ncmax, stream.cuda_stream)
    args += (p["pseg"], p["rm"], cand_off.ctypes.data, p["cand_off"], accept_ptr, ncmax)
    out, counts, accept = lp._two_pass(_lib.ud.ud_lidar_paste_count, _lib.ud.ud_lidar_paste_compact, args, result_d, ws,
                                       device, stream, out_compact)
    return out, counts, accept.reshape(B, ncmax).copy()


def _store_accept(pastes, accept):
    for b, p in enumerate(pastes):
        if p is not None:
            p["accept"] = accept[b, :len(p["cand_idx"])].astype(bool)


def lidar_paste_host_clouds(clouds, plans, device, compact=False):
    """lidar_prep_host_clouds for a batch in which at least one sample's lidar_aug record carries a ``paste`` record
    (GTSampling): selection, then the fused chain with point removal and the accepted objects' clouds ahead of each
    sample's scene (concatenate([obj_points, points])), BDA / range filter / padding as without paste.  One H2D copy
    (scene clouds + plan), four launches, one host wait.  Each paste record gets ``accept`` (bool per candidate).
    -> (points f32 [B, Nmax, D], or [sum(counts), D] with ``compact``; counts int64 [B]; accept uint8 [B, Ncmax])."""
    device = _lib.require_gpu_device(device)
    arrs, D = lp._host_clouds(clouds, plans)
    pastes = [None if a is None else a.get("paste") for a in plans]
    scenes = []
    for cs, aug in zip(arrs, plans):
        m, x, l, bda, rg = lp._plan_segments(cs, aug, D)
        scenes.append(([len(a) for a in cs], m, x, l, bda, rg))
    plan, parts, ncmax, rows = _paste_plan(scenes, pastes, D)
    B = len(arrs)
    pts_bytes = align16(rows * D * 4)
    result = []

    def fill(host, dev):                    # the plan holds addresses inside dev and result_d
        result.append(torch.empty(8 * B + B * ncmax, dtype=torch.uint8, device=dev.device))
        lp._stage_clouds(host, arrs)
        _resolve(plan, parts, dev.data_ptr(), result[0].data_ptr() + 8 * B)
        host[pts_bytes:] = plan

    def run(dev, s):
        return _paste_run(D, parts, dev.data_ptr() + pts_bytes, B, ncmax, result[0], dev.device, s, compact)

    out, counts, accept = staged_upload(device, pts_bytes + len(plan), fill, run)
    _store_accept(pastes, accept)
    return out, counts, accept


def gt_paste(points, seg, gt_boxes, database, cand_idx, cand_group, remove_extra_width=(0, 0, 0)):
    """The paste alone on device clouds: ``points`` f32 [rows, D], the samples' scenes back to back, ``seg`` their row
    offsets (B + 1 ints); per sample ``gt_boxes`` [M_b, >= 7], ``cand_idx`` database indices and ``cand_group`` their
    ascending group ids (a single array each for B == 1).  Candidates are selected by the DataBaseSampler rule, scene
    points inside an accepted candidate's box (enlarged by ``remove_extra_width``) are dropped, the accepted objects'
    clouds are placed ahead of their sample's scene.  No sweep transform, BDA or range filter.  Runs on the current
    stream; one host wait.  -> (points_out f32 [sum(counts), D], counts int64 numpy [B], accept uint8 numpy [B, Ncmax])."""
    seg = lp._check_points_seg(points, seg, 2)
    D = points.shape[1]
    B = len(seg) - 1
    if B == 1 and not isinstance(cand_idx, (list, tuple)):
        gt_boxes, cand_idx, cand_group = [gt_boxes], [cand_idx], [cand_group]
    if not (len(gt_boxes) == len(cand_idx) == len(cand_group) == B):
        raise ValueError("one gt_boxes / cand_idx / cand_group entry per sample")
    rew = tuple(float(v) for v in remove_extra_width)
    pastes, scenes = [], []
    for b in range(B):
        idx, grp = np.asarray(cand_idx[b], np.int64).reshape(-1), np.asarray(cand_group[b], np.int32).reshape(-1)
        if len(idx) != len(grp):
            raise ValueError(f"sample {b}: {len(idx)} candidates, {len(grp)} groups")
        pastes.append({"database": database, "cand_idx": idx, "cand_group": grp,
                       "gt_boxes": np.asarray(gt_boxes[b], np.float32),
                       "remove_extra_width": rew})
        scenes.append(([seg[b + 1] - seg[b]], [None], [False], [np.nan], None, None))
    plan, parts, ncmax, _ = _paste_plan(scenes, pastes, D)
    device = points.device
    stream = torch.cuda.current_stream(device)
    result_d = torch.empty(8 * B + B * ncmax, dtype=torch.uint8, device=device)
    _resolve(plan, parts, points.data_ptr(), result_d.data_ptr() + 8 * B)
    plan_d = torch.from_numpy(plan).to(device)
    return _paste_run(D, parts, plan_d.data_ptr(), B, ncmax, result_d, device, stream, True)


def append_pasted(data_dict):
    """After the readback: the sample's gt_boxes / gt_labels with the accepted candidates' boxes and labels appended,
    the boxes through the same BDA (bda_boxes, the parameters BevAffineTransformation left in lidar_aug["bda_params"])
    and boxes_in_range_mask the loader applied to the scene's boxes.  -> a shallow copy of data_dict (the input is not
    changed); the sample itself when it carries no paste record."""
    a = data_dict.get("lidar_aug")
    p = None if a is None else a.get("paste")
    if p is None:
        return data_dict
    if "accept" not in p:
        raise ValueError("the paste record has no accept bytes: run lidar_prep_host_clouds first")
    scene = np.asarray(data_dict["gt_boxes"])
    width = scene.shape[1] if scene.ndim == 2 else 7
    db = p["database"]
    if db.boxes.shape[1] < width:
        raise ValueError(f"the database's boxes have {db.boxes.shape[1]} columns, the scene's {width}")
    sel = np.nonzero(p["accept"])[0]
    boxes = db.boxes[np.asarray(p["cand_idx"], np.int64)[sel], :width].astype(np.float32)
    labels = np.asarray(p["cand_labels"])[sel] if "cand_labels" in p else db.class_ids[p["cand_idx"]][sel]
    if a.get("bda_mat") is not None:
        if a.get("bda_params") is None:
            raise ValueError("lidar_aug has a bda_mat but no bda_params (rotate, scale, flip_dx, flip_dy) for the boxes")
        rot, scale, fx, fy = a["bda_params"]
        boxes = lp.bda_boxes(boxes, np.asarray(a["bda_mat"], np.float64), rot, scale, fx, fy)
    if a.get("range") is not None and len(boxes):
        mask = lp.boxes_in_range_mask(boxes, a["range"])
        boxes, labels = boxes[mask], labels[mask]
    out = dict(data_dict)
    out["gt_boxes"] = np.concatenate([scene.reshape(-1, width), boxes]).astype(scene.dtype, copy=False)
    if data_dict.get("gt_labels", None) is not None:
        sl = np.asarray(data_dict["gt_labels"])
        out["gt_labels"] = np.concatenate([sl, labels.astype(sl.dtype)])
    return out
