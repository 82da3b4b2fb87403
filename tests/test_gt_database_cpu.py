"""CPU: the host side of the GT-database build (ops/gt_paste.py, csrc/gt_database.hip) -- the new
prototypes and their host validation (nothing is launched), the save / load round trip, the builder's argument checks --
and the float64 restatement's own check (tests/gt_database_reference.py): the committed seeds leave no row within
ROW_MARGIN of a box face."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gt_database_reference as dbref                                               # noqa: E402

from unidistill_amd.ops import gt_paste as gp                                       # noqa: E402
from unidistill_amd.ops import input_prep as ip                                     # noqa: E402

NEW = ("ud_points_in_boxes", "ud_gt_db_workspace_bytes", "ud_gt_db_count", "ud_gt_db_extract")
FAKE = 1 << 40                                                                      # never dereferenced
i64 = lambda v: np.ascontiguousarray(np.asarray(v, np.int64))


def test_reexported_from_input_prep():
    assert ip.points_in_boxes is gp.points_in_boxes and ip.ObjectDatabaseBuilder is gp.ObjectDatabaseBuilder


def test_symbols_are_declared_exported_and_typed(hip_lib):
    from unidistill_amd import _lib
    P, I, L, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    sigs = _lib.parse_header(open(_lib.HEADER_PATH).read())
    assert sigs["ud_points_in_boxes"] == (I, [P, L, I, L, P, P, P, I, L, P, P, I, P, P])
    assert sigs["ud_gt_db_workspace_bytes"] == (Z, [L, L])
    assert sigs["ud_gt_db_count"] == (I, [P, L, P, P, P, P, I, P, P, Z, P])
    assert sigs["ud_gt_db_extract"] == (I, [P, L, I, L, P, I, L, L, P, P, L, P, Z, P])
    for name in NEW:
        assert name in _lib.exported_symbols()
        assert list(getattr(hip_lib, name).argtypes) == sigs[name][1] and getattr(hip_lib, name).restype == sigs[name][0]


def _pib(lib, rows=10, D=5, ps=5, seg=(0, 10), W=7, bs=7, box_off=(0, 2), B=1):
    seg, box_off = i64(seg), i64(box_off)
    return lib.ud_points_in_boxes(FAKE, rows, D, ps, seg.ctypes.data, FAKE, FAKE, W, bs, box_off.ctypes.data, FAKE, B,
                                  FAKE, None)


def _count(lib, rows=10, seg=(0, 10), box_off=(0, 2), B=1):
    seg, box_off = i64(seg), i64(box_off)
    return lib.ud_gt_db_count(FAKE, rows, seg.ctypes.data, FAKE, box_off.ctypes.data, FAKE, B, FAKE, FAKE, 1 << 30, None)


def _extract(lib, rows=10, D=5, ps=5, W=7, bs=7, n_boxes=2, counts=(3, 4, 7), out_rows=7):
    counts = i64(counts)
    return lib.ud_gt_db_extract(FAKE, rows, D, ps, FAKE, W, bs, n_boxes, counts.ctypes.data, FAKE, out_rows, FAKE, 1 << 30,
                                None)


def test_invalid_arguments_are_refused_on_the_host(hip_lib):
    """Fake pointers, no GPU: every one of these returns UD_ERR_INVALID_ARG before anything is launched."""
    bad = -1
    assert _pib(hip_lib, rows=10, seg=(0, 12, 10), box_off=(0, 1, 2), B=2) == bad    # descending row offsets
    assert _pib(hip_lib, seg=(0, 4, 10), box_off=(0, 2, 1), B=2) == bad              # descending box offsets
    assert _pib(hip_lib, seg=(0, 9)) == bad                                          # the offsets do not span the rows
    assert _pib(hip_lib, D=2, ps=2) == bad
    assert _pib(hip_lib, W=6, bs=6) == bad
    assert _pib(hip_lib, ps=4) == bad and _pib(hip_lib, bs=6) == bad                 # a stride below the row
    assert _pib(hip_lib, B=-1) == bad and _pib(hip_lib, rows=1 << 31, seg=(0, 1 << 31)) == bad
    assert _count(hip_lib, seg=(0, 12, 10), box_off=(0, 1, 2), B=2) == bad
    assert _count(hip_lib, seg=(0, 4, 10), box_off=(0, 2, 1), B=2) == bad
    assert _count(hip_lib, seg=(1, 10)) == bad and _count(hip_lib, box_off=(1, 2)) == bad
    assert _count(hip_lib, box_off=(0, (1 << 18) + 1)) == bad                        # more boxes than the sort key holds
    assert _extract(hip_lib, D=2, ps=2) == bad
    assert _extract(hip_lib, W=6, bs=6) == bad
    assert _extract(hip_lib, out_rows=6) == bad                                      # out_rows below the counted total
    assert _extract(hip_lib, counts=(3, 4, 8), out_rows=8) == bad                    # the total is not the counts' sum
    assert _extract(hip_lib, counts=(-1, 8, 7)) == bad
    assert _extract(hip_lib, counts=(6, 6, 12), out_rows=12) == bad                  # more hits than rows
    assert hip_lib.ud_gt_db_workspace_bytes(-1, 2) == 0 and hip_lib.ud_gt_db_workspace_bytes(10, -1) == 0


def test_all_zero_sizes_are_ok(hip_lib):
    assert hip_lib.ud_points_in_boxes(None, 0, 5, 5, None, None, None, 7, 7, None, None, 0, None, None) == 0
    assert hip_lib.ud_gt_db_count(None, 0, None, None, None, None, 0, None, None, 0, None) == 0
    assert hip_lib.ud_gt_db_extract(None, 0, 5, 5, None, 7, 7, 0, None, None, 0, None, 0, None) == 0
    assert hip_lib.ud_gt_db_workspace_bytes(0, 0) == 0
    z = i64([0, 0])                                                                  # one sample, no rows, no boxes
    assert hip_lib.ud_points_in_boxes(None, 0, 5, 5, z.ctypes.data, None, None, 7, 7, z.ctypes.data, None, 1, None,
                                      None) == 0
    a, b = hip_lib.ud_gt_db_workspace_bytes(1000, 40), hip_lib.ud_gt_db_workspace_bytes(1000, 1000)
    assert 0 < a < b                                                                 # a second sort pass needs its buffers


def test_save_load_round_trip_is_bit_for_bit(tmp_path):
    rng = np.random.default_rng(3)
    rows = np.array([4, 0, 7, 1])
    pts = rng.normal(size=(rows.sum(), 5)).astype(np.float32)
    pts[2, 1], pts[5, 4] = np.nan, -0.0
    boxes = rng.normal(size=(4, 9)).astype(np.float32)
    db = gp.ObjectDatabase(pts, np.concatenate([[0], np.cumsum(rows)]), boxes, [2, 0, 0, 1], ["car", "truck", "bus"],
                           device="cpu")
    path = tmp_path / "db.npz"
    db.save(path)
    assert sorted(os.listdir(tmp_path)) == ["db.npz"]
    got = gp.ObjectDatabase.load(path, device="cpu", name="reloaded")
    assert got.name == "reloaded" and got.class_names == db.class_names and got.points.device.type == "cpu"
    np.testing.assert_array_equal(got.points.numpy().view(np.uint32), pts.view(np.uint32))
    np.testing.assert_array_equal(got.boxes.view(np.uint32), boxes.view(np.uint32))
    assert got.offsets.tolist() == db.offsets.tolist() and got.class_ids.tolist() == [2, 0, 0, 1]
    assert got.offsets.dtype == np.int64 and got.class_ids.dtype == np.int64 and got.boxes.dtype == np.float32
    with np.load(path) as z:
        assert sorted(z.files) == ["boxes", "class_ids", "class_names", "offsets", "points"]


def test_builder_argument_checks_come_before_any_device_work():
    b = gp.ObjectDatabaseBuilder(["car", "truck"])
    pts, boxes = np.zeros((4, 5), np.float32), np.zeros((2, 9), np.float32)
    with pytest.raises(ValueError, match="exactly one"):
        b.add_scene(pts, boxes)
    with pytest.raises(ValueError, match="exactly one"):
        b.add_scene(pts, boxes, gt_names=["car", "car"], gt_labels=[0, 0])
    with pytest.raises(ValueError, match="unknown label"):
        b.add_scene(pts, boxes, gt_labels=[0, 2])
    with pytest.raises(ValueError, match="unknown label"):
        b.add_scene(pts, boxes, gt_labels=[-1, 0])
    with pytest.raises(ValueError, match="2 boxes, 1 names"):
        b.add_scene(pts, boxes, gt_names=["car"])
    with pytest.raises(ValueError, match="W >= 7"):
        b.add_scene(pts, boxes[:, :6], gt_labels=[0, 0])
    with pytest.raises(ValueError, match="float32"):
        b.add_scene(pts.astype(np.float64), boxes, gt_labels=[0, 0])
    with pytest.raises(ValueError, match="4 columns, the scenes before 5"):      # D must match across scenes
        b.add_scenes([{"points": pts, "gt_boxes": boxes, "gt_labels": [0, 1]},
                      {"points": pts[:, :4], "gt_boxes": boxes, "gt_labels": [0, 1]}])
    assert b.D is None and b.scenes == 0                                           # nothing was taken in
    with pytest.raises(ValueError, match="no scene"):
        b.finish()
    with pytest.raises(RuntimeError, match="GPU only"):                            # valid arguments, but a CPU device
        gp.ObjectDatabaseBuilder(["car"], device="cpu").add_scene(pts, boxes, gt_labels=[0, 0])
    with pytest.raises(RuntimeError, match="GPU only"):
        gp.points_in_boxes(torch.zeros(4, 5), None, boxes)


def test_restatement_against_a_brute_force_loop():
    rng = np.random.default_rng(11)
    boxes = dbref.grid_boxes(rng, 3, nx=3)
    boxes[2] = boxes[0]
    boxes[2, :2] += 0.3                                                             # overlaps box 0: box 0 wins
    pts = dbref.scene_points(rng, 50, boxes, share_in=0.7, extra=dbref._centre_rows(rng, boxes[0], 8))
    pts[4, 0] = np.nan
    owner, near = dbref.owners(pts, [0, 50], boxes, [0, 3])
    assert near == 0
    inside, _ = dbref.inside_all(pts, boxes)
    assert (inside[:, 0] & inside[:, 2]).sum() >= 8 and set(owner.tolist()) == {-1, 0, 1, 2} and owner[4] == -1
    np.testing.assert_array_equal(owner, dbref.brute_owner(pts, boxes))
    clouds, counts = dbref.extract(pts, [0, 50], boxes, [0, 3], owner)
    assert counts.tolist() == [int((owner == i).sum()) for i in range(3)] and len(clouds) == counts.sum()
    first = pts[owner == 1][0]
    row = clouds[counts[0]]
    assert row[3] == first[3] and row[0] == np.float32(first[0] - boxes[1, 0]) and row[4] == first[4]


def test_committed_seeds_leave_no_row_near_a_face_and_hold_their_situations():
    pts, seg, boxes, off = dbref.owner_case()
    owner, near = dbref.owners(pts, seg, boxes, off)
    assert near == 0 and np.diff(seg).tolist() == [1000, 300] and np.diff(off).tolist() == [7, 3]
    assert pts.shape[1] == 5 and boxes.shape[1] == 9 and np.nanmax(np.abs(pts[:, :3])) < dbref.LIMIT
    inside, _ = dbref.inside_all(pts[:1000], np.where(np.isnan(boxes[:7]), 0.3, boxes[:7]))
    assert (inside[:, 1] & inside[:, 4]).sum() >= 20 and (owner[:1000] == 4).sum() > 0       # shared: box 1 wins
    assert not inside[:, 5].any() and inside[:, 6].sum() > 0 and not (owner[:1000] == 6).any()   # NaN yaw: owns nothing
    assert np.isnan(pts[:, :3]).any(axis=1).sum() == 3 and (owner[np.isnan(pts[:, :3]).any(axis=1)] == -1).all()
    assert 0.1 < (owner >= 0).mean() < 0.6
    pts, seg, boxes, off = dbref.chunk_case()
    owner, near = dbref.owners(pts, seg, boxes, off)
    inside, _ = dbref.inside_all(pts, boxes)
    assert near == 0 and len(pts) == 600 and len(boxes) == 130
    assert (inside[:, 10] & inside[:, 100]).sum() >= 15 and (owner == 100).sum() > 0 and owner.max() > 64
    pts, seg, boxes, off = dbref.empty_case()
    assert dbref.owners(pts, seg, boxes, off)[1] == 0 and np.diff(off).tolist() == [2, 0, 3]
    for p, b, names in dbref.builder_scenes():
        assert dbref.owners(p, [0, len(p)], b, [0, len(b)])[1] == 0 and len(names) == len(b)
    p, b = dbref.paste_scene()
    owner, near = dbref.owners(p, [0, 2000], b, [0, 6])
    assert near == 0 and all((owner == i).sum() > 0 for i in range(6))
