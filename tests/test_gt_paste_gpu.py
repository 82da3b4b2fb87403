"""GPU: the GT-sampling paste -- ud_gt_paste_select and the fused chain with point removal and paste
(ud_lidar_paste_count / ud_lidar_paste_compact) through ops/gt_paste.py and collate_fn -- against the float64 restatement
tests/gt_paste_reference.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gt_paste_reference as ref                                                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 256                                                                         # csrc/lidar_prep.hip kTile


@pytest.fixture(scope="module")
def world(hip_lib):
    """The chain cases, the device database and the BDA, built once and left unchanged."""
    from unidistill_amd.ops import gt_paste as gp, input_prep as ip
    arrays, cases = ref.chain_cases()
    db = gp.ObjectDatabase.from_arrays(*arrays, ref.CLASSES, device=DEV, name="gt_paste_gpu_tests")
    margs, bpar = ref.bda_setup()
    return {"arrays": arrays, "cases": cases, "db": db, "bda_mat": ip.bev_transform_matrix(*margs), "bda_params": bpar}


def _selection(case):
    """ud_gt_paste_select on a list of (cand, group, gt) -> accept uint8 [B, ncmax]."""
    from unidistill_amd import _lib
    B = len(case)
    off = lambda ns: np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    cand_off, gt_off = off([len(c) for c, _, _ in case]), off([len(g) for _, _, g in case])
    ncmax = int(max(len(c) for c, _, _ in case))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    cand = dev(np.concatenate([c for c, _, _ in case]))
    grp = dev(np.concatenate([g for _, g, _ in case]).astype(np.int32))
    gt = dev(np.concatenate([g for _, _, g in case]))
    accept = torch.full((B, ncmax), 7, dtype=torch.uint8, device=DEV)
    _lib.ud.ud_gt_paste_select(gt, gt_off.ctypes.data, dev(gt_off), cand, grp, cand_off.ctypes.data, dev(cand_off), B,
                               accept, ncmax, _lib.stream_of(accept))
    return accept.cpu().numpy()


def test_selection_matches_the_reference(hip_lib):
    case = ref.selection_case()
    got = _selection(case)
    assert got.shape == (3, 63)
    pairs = near_pairs = 0
    for b, (cand, grp, gt) in enumerate(case):
        want, near = ref.select(cand, grp, gt)
        n = len(cand)
        pairs += n * len(gt) + n * (n - 1) // 2
        near_pairs += round(ref.near_pair_share(cand, gt) * (n * len(gt) + n * (n - 1) // 2))
        cmp = ~near
        np.testing.assert_array_equal(got[b, :n][cmp], want[cmp].astype(np.uint8))
        assert (got[b, n:] == 0).all()                                             # bytes past the candidates are cleared
    print("near-touching pairs", near_pairs, "of", pairs)
    assert near_pairs <= 0.02 * pairs
    again = _selection(case)
    np.testing.assert_array_equal(got, again)


def _plans(world, name, on):
    """Per sample (clouds, lidar_aug record with the paste record) of a chain case; ``on``: BDA + range filter."""
    clouds, plans = [], []
    for s in world["cases"][name]:
        aug = dict(s["aug"], bda_mat=world["bda_mat"] if on else None, bda_params=world["bda_params"] if on else None,
                   range=np.array(ref.PCR, np.float32) if on else None)
        if s["paste"] is not None:
            aug["paste"] = dict(s["paste"], database=world["db"])
        clouds.append(s["clouds"])
        plans.append(aug)
    return clouds, plans


def _reference(world, plans, clouds):
    pts, off, boxes, _ = world["arrays"]
    out = []
    for cs, aug in zip(clouds, plans):
        p = aug.get("paste")
        acc = ref.select(boxes[p["cand_idx"], :7], p["cand_group"], p["gt_boxes"])[0] if p is not None else np.zeros(0, bool)
        out.append((acc,) + ref.chain(cs, aug, pts, off, boxes, p, acc))
    return out


@pytest.mark.parametrize("compact", [False, True], ids=["padded", "compact"])
@pytest.mark.parametrize("on", [False, True], ids=["plain", "bda_range"])
@pytest.mark.parametrize("name", ["mixed", "extra_width", "all_rejected", "no_candidates"])
def test_chain_matches_the_reference(world, name, on, compact):
    from unidistill_amd.ops import gt_paste as gp
    clouds, plans = _plans(world, name, on)
    want = _reference(world, plans, clouds)
    out, counts, accept = gp.lidar_paste_host_clouds(clouds, plans, DEV, compact=compact)
    again = gp.lidar_paste_host_clouds(clouds, plans, DEV, compact=compact)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), again[0].view(torch.int32))          # two runs: bitwise equal
    np.testing.assert_array_equal(counts, again[1])
    got = out.cpu().numpy()
    near_rows = rows = 0
    start = 0
    for b, (acc, r, keep, near) in enumerate(want):
        np.testing.assert_array_equal(accept[b, :len(acc)], acc.astype(np.uint8))
        if plans[b].get("paste") is not None:
            np.testing.assert_array_equal(plans[b]["paste"]["accept"], acc)
        k = int(counts[b])
        if compact:
            mine = got[start:start + k]
            start += k
        else:
            mine = got[b, :k]
            assert (got[b, k:].view(np.uint32) == 0).all()                         # zero padding
        near_rows += ref.compare_sample(mine, r, keep, near)
        rows += len(r)
    assert (got.shape == (int(counts.sum()), 5)) if compact else (got.shape == (2, int(counts.max()), 5))
    print("near rows", near_rows, "of", rows)
    assert near_rows <= 0.01 * rows
    if name == "mixed":
        acc1, r1, keep1, _ = want[1]
        obj11 = (r1[:, 3] >= 100000 + 924)                                         # object 11's 300 rows (x = 200 m)
        assert acc1[1] and obj11.sum() == 300 and keep1[obj11].all() != on         # pasted, and gone with the range on
    if name == "all_rejected":
        assert not accept.any() and [int(c) for c in counts] == [256, 257]


def test_public_op_matches_the_reference(world):
    """gt_paste on device clouds: the paste alone (no sweep transform, BDA or range filter), compact output."""
    from unidistill_amd.ops import gt_paste as gp
    smps = world["cases"]["extra_width"]
    pts, off, boxes, _ = world["arrays"]
    scenes = [np.concatenate(s["clouds"]) for s in smps]
    x = torch.from_numpy(np.concatenate(scenes)).to(DEV)
    seg = np.cumsum([0] + [len(s) for s in scenes])
    out, counts, accept = gp.gt_paste(x, seg, [s["paste"]["gt_boxes"] for s in smps], world["db"],
                                      [s["paste"]["cand_idx"] for s in smps], [s["paste"]["cand_group"] for s in smps],
                                      remove_extra_width=(0.2, 0.2, 0.2))
    got = out.cpu().numpy()
    start = 0
    for b, s in enumerate(smps):
        acc = ref.select(boxes[s["paste"]["cand_idx"], :7], s["paste"]["cand_group"], s["paste"]["gt_boxes"])[0]
        np.testing.assert_array_equal(accept[b, :len(acc)], acc.astype(np.uint8))
        aug = {"sweep_mats": [], "time_lags": [], "bda_mat": None, "range": None}
        r, keep, near = ref.chain([scenes[b]], aug, pts, off, boxes, s["paste"], acc)
        r[len(r) - len(scenes[b]):, 4] = scenes[b][:, 4]                           # no time lag here: the column is kept
        ref.compare_sample(got[start:start + int(counts[b])], r, keep, near)
        start += int(counts[b])
    assert start == len(got)


def _samples(world, with_paste, seed=9):
    """Two synthetic loader samples through our loader-side transforms (GTSampling only ``with_paste``)."""
    from unidistill_amd.ops import gt_paste as gp, input_prep as ip
    rng = np.random.default_rng(seed)
    boxes = world["arrays"][2]
    sampler = gp.GTSampling(world["db"], ref.CLASSES, ["car:2", "truck:2", "bicycle:1"], remove_extra_width=(0.1, 0.1, 0.1),
                            seed=4)
    np.random.seed(12)
    bda = ip.BevAffineTransformation(rot_lim=(-45.0, 45.0), scale_lim=(0.9, 1.1), trans_lim=(0.5, 0.5, 0.5),
                                     flip_dx_ratio=0.5, flip_dy_ratio=0.5)
    out = []
    for k, n in enumerate((700, 900)):
        clouds, aug = ref.scene(rng, n)
        gt = np.concatenate([boxes[[3 * k]], boxes[[3 * k + 1]] + np.float32(40.0) * (np.arange(9) == 1)]).astype(np.float32)
        d = {"points": clouds[0], "sweep_points": clouds[1:], "gt_boxes": gt, "gt_labels": np.array([0, 1], np.int64),
             "lidar_aug": dict(aug)}
        if with_paste:
            d = sampler(d)
        d = ip.ObjectRangeFilter(ref.PCR)(bda(d))
        d["points_raw"] = [d.pop("points")] + list(d.pop("sweep_points"))
        out.append(d)
    return out


def test_collate_end_to_end_and_the_voxelizer_takes_the_batch(world):
    from unidistill_amd import synthetic as syn
    from unidistill_amd.ops import input_prep as ip
    from unidistill_amd.ops.voxelize import voxelize_batch
    pts, off, boxes, ids = world["arrays"]
    data = _samples(world, True)
    before = [(d["gt_boxes"].copy(), d["gt_labels"].copy()) for d in data]
    batch = ip.collate_fn(data, device=DEV)
    torch.cuda.synchronize()
    got_pts = batch["points"].cpu().numpy()
    lens = []
    for b, d in enumerate(data):
        a = d["lidar_aug"]
        p = a["paste"]
        assert len(p["cand_idx"]) == 5
        acc = ref.select(boxes[p["cand_idx"], :7], p["cand_group"], p["gt_boxes"])[0]
        np.testing.assert_array_equal(p["accept"], acc)
        assert not acc[boxes[p["cand_idx"], 0] == boxes[3 * b, 0]].any()            # the scene's own object is never pasted
        r, keep, near = ref.chain(d["points_raw"], a, pts, off, boxes, p, acc)
        k = int((np.abs(got_pts[b]).sum(axis=1) != 0).sum())
        ref.compare_sample(got_pts[b, :k], r, keep, near)
        sel = p["cand_idx"][acc]
        add = ip.bda_boxes(boxes[sel], a["bda_mat"], *a["bda_params"])
        mask = ip.boxes_in_range_mask(add, ref.PCR)
        want_boxes = np.concatenate([before[b][0], add[mask]])
        want_labels = np.concatenate([before[b][1], (ids[sel] % 3)[mask]])
        lens.append(len(want_boxes))
        np.testing.assert_array_equal(batch["gt_boxes"][b, :lens[-1]].cpu().numpy().view(np.uint32),
                                      want_boxes.view(np.uint32))
        np.testing.assert_array_equal(batch["gt_labels"][b, :lens[-1]].cpu().numpy(), want_labels.astype(np.float32))
        np.testing.assert_array_equal(d["gt_boxes"], before[b][0])                  # the samples are not changed
    assert batch["gt_boxes"].shape == (2, max(lens), 9) and max(lens) > 2
    _, coords, num, mean, _ = voxelize_batch(batch["points"], syn.VOXEL_SIZE, syn.POINT_CLOUD_RANGE, 10, 120000,
                                             want_voxels=False)
    torch.cuda.synchronize()
    assert coords.shape[0] > 0 and bool(torch.isfinite(mean).all())


def test_batch_without_a_paste_record_is_the_existing_path(world):
    """collate_fn on samples that never saw GTSampling: torch.equal to ud_lidar_prep_* driven directly (the existing
    route), and the boxes / labels are the samples' own."""
    from unidistill_amd.ops import input_prep as ip, lidar_prep as lp
    data = _samples(world, False)
    assert all("paste" not in d["lidar_aug"] for d in data)
    batch = ip.collate_fn(data, device=DEV)
    clouds, plans = [d["points_raw"] for d in data], [d["lidar_aug"] for d in data]
    D = 5
    rows, nseg, mats, xf, last, bdas, rgs = [], [], [], [], [], [], []
    for cs, a in zip(clouds, plans):
        m, x, l, bda, rg = lp._plan_segments(cs, a, D)
        rows += [len(c) for c in cs]
        nseg.append(len(cs))
        mats, xf, last = mats + m, xf + x, last + l
        bdas.append(bda)
        rgs.append(rg)
    buf, parts = lp._lidar_tables(rows, nseg, mats, xf, last, bdas, rgs)
    x = torch.from_numpy(np.concatenate([c for cs in clouds for c in cs])).to(DEV)
    plan = torch.from_numpy(buf).to(DEV)
    want, _ = lp._lidar_run(x, x.shape[0], D, parts, plan.data_ptr(), torch.device(DEV), torch.cuda.current_stream(),
                            False)
    torch.cuda.synchronize()
    assert torch.equal(batch["points"].view(torch.int32), want.view(torch.int32))
    for b, d in enumerate(data):
        n = len(d["gt_boxes"])
        assert torch.equal(batch["gt_boxes"][b, :n].cpu(), torch.from_numpy(d["gt_boxes"]))


def test_invalid_plans_are_refused_and_a_valid_call_follows(world):
    from unidistill_amd import _lib
    from unidistill_amd.ops import gt_paste as gp
    lib = _lib.load()
    i64 = lambda v: np.ascontiguousarray(np.asarray(v, np.int64))
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)                      # real device memory behind every pointer
    p = buf.data_ptr()
    assert lib.ud_gt_paste_select(p, i64([0, 0]).ctypes.data, p, p, p, i64([0, 64]).ctypes.data, p, 1, p, 64, None) == -1
    many = 65
    assert lib.ud_lidar_paste_count(None, 0, 5, i64(np.zeros(many + 1)).ctypes.data, i64([0, many]).ctypes.data, many, 1,
                                    p, p, p, p, p, p, i64([0, 0]).ctypes.data, p, p, 0, p, None, 0, None) == -1
    assert lib.ud_lidar_paste_count(None, 4, 5, i64([0, 4]).ctypes.data, i64([0, 1]).ctypes.data, 1, 1, p, p, p, p, p, p,
                                    i64([0, 64]).ctypes.data, p, p, 64, p, None, 0, None) == -1      # 64 removal boxes
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0                                                     # nothing was launched
    clouds, plans = _plans(world, "mixed", True)
    out, counts, accept = gp.lidar_paste_host_clouds(clouds, plans, DEV)
    torch.cuda.synchronize()
    assert accept[0, :4].tolist() == [1, 0, 1, 1] and out.shape[1] == int(counts.max())
