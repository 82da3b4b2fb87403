"""GPU: building the GT-sampling object database on the device (ops/gt_paste.py, csrc/gt_database.hip)
against the float64 restatement of tests/gt_database_reference.py.  The generators re-draw every row within ROW_MARGIN of
a box face, every test asserts that none is left, so owners, counts and clouds are compared exactly and in full."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gt_database_reference as dbref                                               # noqa: E402

pytestmark = pytest.mark.gpu

from unidistill_amd.ops import gt_paste as gp                                       # noqa: E402

DEV = "cuda:0"
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cases(hip_lib):
    """name -> (inputs, reference owner, reference clouds, reference counts); computed once, never changed."""
    out = {}
    for name, make in (("owner", dbref.owner_case), ("chunk", dbref.chunk_case), ("empty", dbref.empty_case)):
        pts, seg, boxes, off = make()
        owner, near = dbref.owners(pts, seg, boxes, off)
        assert near == 0, "a generated row lies within ROW_MARGIN of a box face"
        clouds, counts = dbref.extract(pts, seg, boxes, off, owner)
        out[name] = ((pts, seg, boxes, off), owner, clouds, counts)
    return out


def _owner(pts, seg, boxes, off):
    return gp.points_in_boxes(torch.from_numpy(pts).to(DEV), seg, boxes, off).cpu().numpy()


def test_owner_matches_the_restatement(cases):
    (pts, seg, boxes, off), want, _, _ = cases["owner"]
    got = _owner(pts, seg, boxes, off)
    assert got.dtype == np.int32 and got.shape == (1300,)
    np.testing.assert_array_equal(got, want)
    assert (want[:1000] == 4).any() and not (want[:1000] == 5).any() and not (want[:1000] == 6).any()
    # a row stride: the same rows as the first 5 of 8 columns
    wide = torch.zeros(1300, 8, device=DEV)
    wide[:, :5] = torch.from_numpy(pts).to(DEV)
    np.testing.assert_array_equal(gp.points_in_boxes(wide[:, :5], seg, boxes, off).cpu().numpy(), want)
    # a single scene without offsets; boxes as a device tensor
    one = gp.points_in_boxes(torch.from_numpy(pts[:1000]).to(DEV), None, torch.from_numpy(boxes[:7]).to(DEV))
    np.testing.assert_array_equal(one.cpu().numpy(), want[:1000])


def test_more_boxes_than_one_lds_chunk(cases):
    (pts, seg, boxes, off), want, _, _ = cases["chunk"]
    inside, _ = dbref.inside_all(pts, boxes)
    shared = inside[:, 10] & inside[:, 100]
    assert shared.sum() >= 15 and (want[shared] == 10).all() and (want == 100).any() and want.max() >= 128
    np.testing.assert_array_equal(_owner(pts, seg, boxes, off), want)


def test_empty_cases(cases):
    (pts, seg, boxes, off), want, _, _ = cases["empty"]
    np.testing.assert_array_equal(_owner(pts, seg, boxes, off), want)            # a sample with rows but no boxes
    assert (want[seg[1]:seg[2]] == -1).all() and (want[seg[2]:] >= 0).any()
    none = gp.points_in_boxes(torch.zeros(0, 5, device=DEV), [0, 0, 0], boxes[:3], [0, 1, 3])
    assert none.shape == (0,) and none.dtype == torch.int32                       # rows = 0
    got = gp.points_in_boxes(torch.from_numpy(pts).to(DEV), None, np.zeros((0, 7), np.float32))
    assert got.shape == (len(pts),) and (got == -1).all()                         # M = 0
    clouds, rows = gp._extract_objects(torch.from_numpy(pts).to(DEV), np.asarray([0, len(pts)], np.int64),
                                       torch.zeros(0, 7, device=DEV), np.asarray([0, 0], np.int64))
    assert clouds.shape == (0, 5) and len(rows) == 0


@pytest.mark.parametrize("name", ["owner", "chunk", "empty"])
def test_extract_matches_the_numpy_construction(cases, name):
    (pts, seg, boxes, off), _, clouds, counts = cases[name]
    got, rows = gp._extract_objects(torch.from_numpy(pts).to(DEV), seg, torch.from_numpy(boxes).to(DEV), off)
    np.testing.assert_array_equal(rows, counts)
    assert got.shape == clouds.shape
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(clouds))
    # the builder on the same scenes against ObjectDatabase.from_arrays of the construction
    labels = np.arange(len(boxes)) % 3
    b = gp.ObjectDatabaseBuilder(dbref.CLASSES, device=DEV)
    b.add_scenes([{"points": pts[seg[k]:seg[k + 1]], "gt_boxes": boxes[off[k]:off[k + 1]],
                   "gt_labels": labels[off[k]:off[k + 1]]} for k in range(len(seg) - 1)])
    db = b.finish()
    want = gp.ObjectDatabase.from_arrays(clouds, np.concatenate([[0], np.cumsum(counts)]), boxes, labels, dbref.CLASSES,
                                         device="cpu")
    assert db.points.is_cuda and db.boxes.shape == (len(boxes), 9)
    np.testing.assert_array_equal(bits(db.points.cpu().numpy()), bits(want.points.numpy()))
    np.testing.assert_array_equal(db.offsets, want.offsets)
    np.testing.assert_array_equal(bits(db.boxes), bits(want.boxes))
    np.testing.assert_array_equal(db.class_ids, want.class_ids)


def _build(scenes, one_by_one, **kw):
    b = gp.ObjectDatabaseBuilder(dbref.CLASSES, device=DEV, **kw)
    if one_by_one:
        for k, (p, bx, names) in enumerate(scenes):
            b.add_scene(torch.from_numpy(p).to(DEV) if k == 1 else p, bx, gt_names=names, sample_idx=f"s{k}")
    else:
        b.add_scenes([{"points": p, "gt_boxes": bx, "gt_names": names, "sample_idx": f"s{k}"}
                      for k, (p, bx, names) in enumerate(scenes)])
    return b


@pytest.fixture(scope="module")
def built(hip_lib):
    """The builder scenes, their reference (per scene: owner, clouds, counts) and the builder fed scene by scene."""
    scenes = dbref.builder_scenes()
    refs = []
    for p, bx, _ in scenes:
        owner, near = dbref.owners(p, [0, len(p)], bx, [0, len(bx)])
        assert near == 0
        refs.append((owner,) + dbref.extract(p, [0, len(p)], bx, [0, len(bx)], owner))
    return scenes, refs, _build(scenes, True, used_classes=["car", "bicycle"])


def test_builder_across_scenes(built):
    scenes, refs, b = built
    cfg = ["car:5"]
    db = b.finish(filter_by_min_points_cfg=cfg, name="built_one_by_one")
    both = _build(scenes, False, used_classes=["car", "bicycle"]).finish(filter_by_min_points_cfg=cfg)
    for a in ("offsets", "boxes", "class_ids"):
        np.testing.assert_array_equal(getattr(db, a), getattr(both, a))
    assert torch.equal(db.points.view(torch.int32), both.points.view(torch.int32))
    # the reference: ownership among ALL boxes, then the class filter, then the min-points filter
    names = np.concatenate([n for _, _, n in scenes])
    boxes = np.concatenate([bx for _, bx, _ in scenes])
    counts = np.concatenate([r[2] for r in refs])
    clouds = np.concatenate([r[1] for r in refs])
    offs = np.concatenate([[0], np.cumsum(counts)])
    used = np.nonzero(np.isin(names, ["car", "bicycle"]))[0]
    want = gp.ObjectDatabase.from_arrays(np.concatenate([clouds[offs[i]:offs[i + 1]] for i in used]),
                                         np.concatenate([[0], np.cumsum(counts[used])]), boxes[used],
                                         [dbref.CLASSES.index(n) for n in names[used]], dbref.CLASSES, device="cpu",
                                         filter_by_min_points_cfg=cfg)
    np.testing.assert_array_equal(bits(db.points.cpu().numpy()), bits(want.points.numpy()))
    np.testing.assert_array_equal(db.offsets, want.offsets)
    np.testing.assert_array_equal(bits(db.boxes), bits(want.boxes))
    np.testing.assert_array_equal(db.class_ids, want.class_ids)
    # scene 0: the unused truck (box 0) owns the points it shares with the car (box 1); the empty and the 3-point car go
    p0, b0, _ = scenes[0]
    inside, _ = dbref.inside_all(p0, b0)
    assert (inside[:, 0] & inside[:, 1]).sum() >= 15 and counts[1] == (inside[:, 1] & ~inside[:, 0]).sum() > 5
    assert counts[2] == 0 and 0 < counts[3] < 5
    cars = db.indices_of("car")
    assert len(db.indices_of("truck")) == 0 and (db.rows[cars] >= 5).all() and db.rows[0] == counts[1]
    assert "barrier" not in db.class_names and len(db) == len(want) < len(used)
    # infos(): OpenPCDet's layout, the class filter applied, the min-points filter not
    infos = b.infos()
    assert sorted(infos) == ["bicycle", "car"] and sum(len(v) for v in infos.values()) == len(used)
    flat = sorted((i for v in infos.values() for i in v), key=lambda i: (i["image_idx"], i["gt_idx"]))
    assert [set(i) for i in flat] == [{"name", "image_idx", "gt_idx", "box3d_lidar", "num_points_in_gt"}] * len(used)
    assert [i["num_points_in_gt"] for i in flat] == counts[used].tolist() and [i["name"] for i in flat] == list(names[used])
    assert flat[0]["image_idx"] == "s0" and flat[0]["gt_idx"] == 1 and flat[-1]["image_idx"] == "s2"
    np.testing.assert_array_equal(np.stack([i["box3d_lidar"] for i in flat]), boxes[used])
    kept = [i for i in flat if not (i["name"] == "car" and i["num_points_in_gt"] < 5)]
    assert [i["num_points_in_gt"] for i in kept] == db.rows.tolist()


def test_build_is_bitwise_reproducible(built):
    scenes, _, b = built
    again = _build(scenes, True, used_classes=["car", "bicycle"])
    x, y = b.finish(), again.finish()
    assert x.points.shape == y.points.shape and torch.equal(x.points.view(torch.int32), y.points.view(torch.int32))
    np.testing.assert_array_equal(x.offsets, y.offsets)


def test_round_trip_through_the_paste(hip_lib):
    p, boxes = dbref.paste_scene()
    owner, near = dbref.owners(p, [0, 2000], boxes, [0, 6])
    assert near == 0
    b = gp.ObjectDatabaseBuilder(["car"], device=DEV)
    b.add_scene(p, boxes, gt_labels=np.zeros(6, np.int64))
    db = b.finish(name="round_trip")
    assert db.rows.tolist() == [(owner == i).sum() for i in range(6)] and db.rows.min() > 0
    rng = np.random.default_rng(1)
    scene = np.zeros((100, 5), np.float32)                                         # a scene without objects, far above
    scene[:, :2], scene[:, 2], scene[:, 3] = rng.uniform(-40, 40, (100, 2)), 20.0, 5000 + np.arange(100)
    out, counts, accept = gp.gt_paste(torch.from_numpy(scene).to(DEV), [0, 100], np.zeros((0, 7), np.float32), db,
                                      np.arange(6), np.arange(6, dtype=np.int32))
    assert accept.reshape(-1)[:6].all() and counts.tolist() == [100 + int(db.rows.sum())]
    out = out.cpu().numpy()
    src = np.concatenate([p[owner == i] for i in range(6)])                       # the in-box rows, box by box, in order
    got = out[:len(src)]
    np.testing.assert_array_equal(bits(got[:, 3:]), bits(src[:, 3:]))
    err = np.abs(got[:, :3].astype(np.float64) - src[:, :3].astype(np.float64)).max()
    print("round trip: max |xyz - source| =", err, "m, bound 2^-17 =", 2.0 ** -17)
    assert err <= 2.0 ** -17
    np.testing.assert_array_equal(bits(out[len(src):]), bits(scene))              # the scene itself follows, untouched


def test_shim_fills_out_in_place(cases):
    from unidistill_amd import shims
    shims.install()
    fn = sys.modules["unidistill.utils.det3d_utils.roiaware_pool3d_cuda"].points_in_boxes_gpu
    (pts, seg, boxes, off), want, _, _ = cases["owner"]
    T = 8
    for k in range(2):
        bx = np.zeros((1, T, 7), np.float32)                                      # padded with zero-size boxes
        bx[0, :off[k + 1] - off[k]] = boxes[off[k]:off[k + 1], :7]
        xyz = torch.from_numpy(np.ascontiguousarray(pts[seg[k]:seg[k + 1], :3])).to(DEV)[None]
        out = torch.full((1, xyz.shape[1]), 77, dtype=torch.int32, device=DEV)
        assert fn(torch.from_numpy(bx).to(DEV), xyz, out) is None
        np.testing.assert_array_equal(out[0].cpu().numpy(), want[seg[k]:seg[k + 1]])
