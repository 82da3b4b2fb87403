"""GPU: the box-fusion kernels (csrc/box_fusion.hip, ops/box_fusion.py) against the float64 reference of
tests/box_fusion_reference.py: counts, labels, membership and order exact, every float field within 4 eps32."""
import functools

import numpy as np
import pytest
import torch

import box_fusion_reference as R

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
K = 4.0                         # the kernel computes in double and rounds once (K of test_tta_merge_gpu.py)
IOU_TOL = 1e-4                  # what test_proposals.py allows ud_boxes_iou_bev against its oracle
MIN_MARGIN = 10 * IOU_TOL       # no same-label pair's IoU may lie closer to the threshold than this
B = 2
THR = 0.3

V16 = [(r, s, fx, fy) for r in (0.0, 6.0) for s in (1.0, 0.97) for fx, fy in ((0, 0), (0, 1), (1, 0), (1, 1))]
FLIPS3 = [(0, 0), (1, 0), (0, 1)]
DOUBLE_FLIP = [(0, 0), (0, 1), (1, 0), (1, 1)]

# name: (seed, S, R, box_dim, labels, views, weights); the seeds were chosen on the CPU so that the reference's smallest
# |IoU - THR| is at least MIN_MARGIN (asserted in every test)
CASES = {
    "s1_r5": (0, 1, 5, 7, 1, None, None),
    "s1_r70": (1, 1, 70, 9, 3, None, None),
    "s1_r150": (1, 1, 150, 7, 1, None, [2.5]),
    "s3_r70_flips": (1, 3, 70, 9, 3, FLIPS3, [1.0, 0.5, 2.0]),
    "s4_r150_double_flip": (3, 4, 150, 7, 1, DOUBLE_FLIP, None),
    "s4_r5_ensemble": (0, 4, 5, 9, 3, None, [1.0, 0.25, 0.5, 1.5]),
    "s16_r70_v16": (57, 16, 70, 9, 3, V16, [1.0 + 0.125 * (s % 5) for s in range(16)]),
}


def make_inputs(seed, S, Rr, box_dim, n_labels, views, equal_scores=False):
    """Per sample a lattice of objects (7 m cells); each source sees most of them, jittered in centre, size, yaw and score, some
    turned by pi, a few twice; plus distractors: lone boxes on free cells and neighbours that overlap an object partly.  Sample 1
    holds about half as many rows as sample 0.  Rows beyond num hold NaN."""
    rng = np.random.default_rng(seed)
    vg = R.general(views, S)
    rois = np.full((S * B, Rr, box_dim), np.nan, np.float32)
    scores = np.full((S * B, Rr), np.nan, np.float32)
    labels = np.full((S * B, Rr), -7, np.int64)
    num = np.zeros(S * B, np.int32)
    for b in range(B):
        n_obj = max(1, int(Rr * (0.85 if b == 0 else 0.4)))
        cells = rng.permutation(144)
        obj = np.zeros((n_obj, box_dim))
        c = cells[:n_obj]
        obj[:, 0] = (c % 12) * 7.0 - 38.5 + rng.uniform(-0.5, 0.5, n_obj)
        obj[:, 1] = (c // 12) * 7.0 - 38.5 + rng.uniform(-0.5, 0.5, n_obj)
        obj[:, 2] = rng.uniform(-2, 1, n_obj)
        obj[:, 3:6] = rng.uniform(1.0, 4.5, (n_obj, 3))
        obj[:, 6] = rng.uniform(-3.1, 3.1, n_obj)
        if box_dim == 9:
            obj[:, 7:9] = rng.uniform(-5, 5, (n_obj, 2))
        obj_label = rng.integers(1, n_labels + 1, n_obj)
        obj_score = rng.uniform(0.15, 0.9, n_obj)
        free = cells[n_obj:]
        for s in range(S):
            rows, sc, lb = [], [], []

            def seen(i, shift=0.0):
                o = obj[i].copy()
                o[0:2] += rng.uniform(-0.15, 0.15, 2) + shift
                o[2] += rng.uniform(-0.1, 0.1)
                o[3:6] *= rng.uniform(0.97, 1.03, 3)
                o[6] += rng.uniform(-0.03, 0.03) + (np.pi if rng.random() < 0.2 else 0.0)
                rows.append(o)
                sc.append(obj_score[i] * rng.uniform(0.9, 1.1))
                lb.append(obj_label[i])
            for i in range(n_obj):
                if rng.random() < 0.9:
                    seen(i)
                    if rng.random() < 0.1:
                        seen(i)                                         # twice in one source
                    if rng.random() < 0.1:
                        seen(i, shift=rng.uniform(0.8, 1.6))            # a neighbour that overlaps it partly
            for _ in range(max(1, Rr // 10)):                           # lone distractors
                cell = free[rng.integers(0, max(len(free), 1))] if len(free) else 0
                o = np.zeros(box_dim)
                o[0], o[1] = (cell % 12) * 7.0 - 38.5, (cell // 12) * 7.0 - 38.5
                o[0:2] += rng.uniform(-2, 2, 2)
                o[3:6] = rng.uniform(0.5, 3.0, 3)
                o[6] = rng.uniform(-3.1, 3.1)
                rows.append(o)
                sc.append(rng.uniform(0.05, 0.3))
                lb.append(rng.integers(1, n_labels + 1))
            order = rng.permutation(len(rows))[:Rr]
            n = len(order)
            row = s * B + b
            orig = np.array([rows[i] for i in order]).reshape(n, box_dim)
            orig[:, 6] = (orig[:, 6] + np.pi) % (2 * np.pi) - np.pi
            rois[row, :n] = R.make_views(orig, vg[s]).astype(np.float32)
            scores[row, :n] = 0.5 if equal_scores else np.array([sc[i] for i in order], np.float32)
            labels[row, :n] = np.array([lb[i] for i in order], np.int64)
            num[row] = n
    return rois, scores, labels, num


@functools.lru_cache(maxsize=None)
def case(name, equal_scores=False, max_out=500):
    seed, S, Rr, box_dim, n_labels, views, weights = CASES[name]
    inputs = make_inputs(seed, S, Rr, box_dim, n_labels, views, equal_scores)
    ref = R.fuse_reference(*inputs, S, views=views, weights=weights, iou_threshold=THR, max_out=max_out)
    for a in inputs:
        a.setflags(write=False)
    return inputs, ref


def run(inputs, S, **kw):
    from unidistill_amd.ops import box_fusion
    dev = torch.device("cuda:0")
    out = box_fusion.fuse_padded(*(torch.tensor(a).to(dev) for a in inputs), S,
                                 return_clusters=True, **kw)
    num = box_fusion.read_num(out[3])
    return [t.cpu().numpy() for t in out], num


def compare(got, num, ref, Rr=None):
    rois, scores, labels, out_num, anchor, members = got
    assert list(out_num) == num
    for b, want in enumerate(ref):
        n = len(want["rows"])
        assert num[b] == n, (b, num[b], n)
        assert np.array_equal(labels[b, :n], want["labels"])
        assert np.array_equal(anchor[b, :n], want["anchor"])                 # order and, with the counts, membership
        assert np.array_equal(members[b, :n], want["members"])
        g, w = rois[b, :n].astype(np.float64), want["rows"]
        bound = K * EPS32 * np.maximum(np.abs(w), 1.0)
        diff = np.abs(g - w)
        diff[:, 6] = np.abs((g[:, 6] - w[:, 6] + np.pi) % (2 * np.pi) - np.pi)
        assert (diff <= bound).all(), (b, float((diff / bound).max()))
        assert ((g[:, 6] >= -np.pi - 4 * EPS32) & (g[:, 6] <= np.pi + 4 * EPS32)).all()
        sb = K * EPS32 * np.maximum(np.abs(want["scores"]), 1.0)
        assert (np.abs(scores[b, :n].astype(np.float64) - want["scores"]) <= sb).all()
        assert not rois[b, n:].any() and not scores[b, n:].any() and not labels[b, n:].any()
        assert (anchor[b, n:] == -1).all() and not members[b, n:].any()


def assert_margin(ref):
    for want in ref:
        assert want["margin"] >= MIN_MARGIN, want["margin"]


@pytest.mark.parametrize("name", list(CASES))
def test_fusion_matches_reference(hip_lib, name):
    seed, S, Rr, box_dim, n_labels, views, weights = CASES[name]
    inputs, ref = case(name)
    assert_margin(ref)
    assert inputs[3][0] != inputs[3][1]                                       # unequal counts
    if Rr >= 70 and S == 1:                                                   # the boxes cross one / two mask words
        assert len(ref[0]["order"]) > (64 if Rr == 70 else 128)
    if S > 1 and Rr >= 70:
        assert max(w["members"].max() for w in ref) > S                       # two boxes of one source in one cluster
        assert any((w["members"] == 1).any() for w in ref)
    got, num = run(inputs, S, views=views, weights=weights, iou_threshold=THR)
    compare(got, num, ref)
    again, num2 = run(inputs, S, views=views, weights=weights, iou_threshold=THR)
    assert num2 == num and all(np.array_equal(a.view(np.uint8), c.view(np.uint8)) for a, c in zip(got, again))


@pytest.mark.parametrize("name", ["s3_r70_flips", "s4_r150_double_flip"])
def test_equal_scores_keep_the_tie_order(hip_lib, name):
    seed, S, Rr, box_dim, n_labels, views, weights = CASES[name]
    inputs, ref = case(name, equal_scores=True)
    assert_margin(ref)
    got, num = run(inputs, S, views=views, weights=weights, iou_threshold=THR)
    compare(got, num, ref)


def test_max_out_keeps_the_top_clusters(hip_lib):
    name = "s3_r70_flips"
    seed, S, Rr, box_dim, n_labels, views, weights = CASES[name]
    inputs, full = case(name)
    inputs, ref = case(name, max_out=7)
    assert all(w["clusters"] > 7 and len(w["rows"]) == 7 for w in ref)
    for w, f in zip(ref, full):
        assert np.array_equal(w["anchor"], f["anchor"][:7])
    got, num = run(inputs, S, views=views, weights=weights, iou_threshold=THR, max_out=7)
    assert got[0].shape == (B, 7, box_dim) and num == [7, 7]
    compare(got, num, ref)


def test_empty_and_single(hip_lib):
    """A sample with no valid box, all of num zero, and one valid box."""
    name = "s3_r70_flips"
    seed, S, Rr, box_dim, n_labels, views, weights = CASES[name]
    inputs, _ = case(name)
    rois, scores, labels, num = (a.copy() for a in inputs)
    num[1::B] = 0                                                             # sample 1 is empty in every source
    ref = R.fuse_reference(rois, scores, labels, num, S, views=views, weights=weights, iou_threshold=THR)
    assert len(ref[1]["rows"]) == 0 and len(ref[0]["rows"]) > 0
    got, n = run((rois, scores, labels, num), S, views=views, weights=weights, iou_threshold=THR)
    assert n[1] == 0
    compare(got, n, ref)
    num[:] = 0
    got, n = run((rois, scores, labels, num), S, views=views, weights=weights, iou_threshold=THR)
    assert n == [0, 0] and not got[0].any() and not got[1].any() and not got[2].any()
    num[2 * B + 0] = 1                                                        # one box, in source 2 of sample 0
    ref = R.fuse_reference(rois, scores, labels, num, S, views=views, weights=weights, iou_threshold=THR)
    got, n = run((rois, scores, labels, num), S, views=views, weights=weights, iou_threshold=THR)
    assert n == [1, 0] and got[4][0, 0] == 2 * Rr
    compare(got, n, ref)


def test_invalid_rows_are_dropped(hip_lib):
    """NaN or inf in a coordinate or the score, and scores at or below score_threshold: dropped, and they block nobody -- the
    result is that of the same inputs with those rows removed."""
    name = "s3_r70_flips"
    seed, S, Rr, box_dim, n_labels, views, weights = CASES[name]
    inputs, _ = case(name)
    rois, scores, labels, num = (a.copy() for a in inputs)
    rng = np.random.default_rng(5)
    thr = 0.2
    bad = np.zeros(scores.shape, bool)
    for row in range(S * B):
        pick = rng.permutation(int(num[row]))[:9]
        bad[row, pick] = True
        rois[row, pick[0], rng.integers(0, box_dim)] = np.nan
        rois[row, pick[1], rng.integers(0, box_dim)] = np.inf
        rois[row, pick[2], 6] = -np.inf
        scores[row, pick[3]] = np.nan
        scores[row, pick[4]] = np.inf
        scores[row, pick[5]] = thr                                            # at the threshold: dropped
        scores[row, pick[6]] = 0.01
        scores[row, pick[7]] = -0.5
        scores[row, pick[8]] = 0.99                                           # a strong box made invalid: it must block nobody
        rois[row, pick[8], 3] = np.nan
    thr32 = float(np.float32(thr))
    ref = R.fuse_reference(rois, scores, labels, num, S, views=views, weights=weights, iou_threshold=THR, score_threshold=thr32)
    assert_margin(ref)
    for b, want in enumerate(ref):
        assert len(want["order"]) > 0 and not any(bad[(a // Rr) * B + b, a % Rr] for a in want["order"])
    got, n = run((rois, scores, labels, num), S, views=views, weights=weights, iou_threshold=THR, score_threshold=thr32)
    compare(got, n, ref)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()            # and the NaN padding was never read into a result


def test_identity_is_bitwise(hip_lib):
    """S = 1, identity view, unit weight, NMS-clean input: boxes and scores come back bit for bit, reordered by score."""
    rng = np.random.default_rng(11)
    n, Rr = 90, 100
    rois = np.full((B, Rr, 9), np.nan, np.float32)
    scores = np.full((B, Rr), np.nan, np.float32)
    labels = np.zeros((B, Rr), np.int64)
    num = np.array([n, n - 37], np.int32)
    for b in range(B):
        c = rng.permutation(144)[:num[b]]
        k = int(num[b])
        rois[b, :k, 0] = (c % 12) * 7.0 - 38.5 + rng.uniform(-0.5, 0.5, k)
        rois[b, :k, 1] = (c // 12) * 7.0 - 38.5 + rng.uniform(-0.5, 0.5, k)
        rois[b, :k, 2] = rng.uniform(-2, 1, k)
        rois[b, :k, 3:6] = rng.uniform(0.5, 4.0, (k, 3))
        rois[b, :k, 6] = rng.uniform(-3.1, 3.1, k)
        rois[b, :k, 7:9] = rng.uniform(-5, 5, (k, 2))
        scores[b, :k] = rng.permutation(k).astype(np.float32) / 128 + 0.1     # distinct
        labels[b, :k] = rng.integers(1, 4, k)
    ref = R.fuse_reference(rois, scores, labels, num, 1, iou_threshold=THR)
    got, cnt = run((rois, scores, labels, num), 1, iou_threshold=THR)
    assert cnt == list(num)
    for b in range(B):
        k = int(num[b])
        assert ref[b]["clusters"] == k                                        # the input is NMS-clean
        order = np.argsort(-scores[b, :k], kind="stable")
        assert np.array_equal(got[0][b, :k].view(np.uint32), rois[b, order].view(np.uint32))
        assert np.array_equal(got[1][b, :k].view(np.uint32), scores[b, order].view(np.uint32))
        assert np.array_equal(got[2][b, :k], labels[b, order])


def test_bad_arguments_write_nothing(hip_lib):
    """box_dim = 8, S = 17 and iou_threshold = NaN: an error from the C entry, nothing launched, nothing written."""
    import ctypes
    from unidistill_amd import _lib
    from unidistill_amd.ops import box_fusion
    lib = _lib.load()
    dev = torch.device("cuda:0")

    def call(S, Rr, box_dim, thr):
        rois = torch.rand((S * B, Rr, box_dim), device=dev)
        scores = torch.rand((S * B, Rr), device=dev)
        labels = torch.ones((S * B, Rr), dtype=torch.int64, device=dev)
        num = torch.full((S * B,), Rr, dtype=torch.int32, device=dev)
        outs = [torch.full((B, 10, box_dim), -3.0, device=dev), torch.full((B, 10), -3.0, device=dev),
                torch.full((B, 10), -3, dtype=torch.int64, device=dev), torch.full((2, B), -3, dtype=torch.int32, device=dev)]
        ws = _lib.workspace(dev, 1 << 24, "box_fusion_test")
        views = (ctypes.c_double * (6 * S))(*([0.0, 1.0, 0.0, 0.0, 0.0, 1.0] * S))
        code = lib.ud_box_fusion(rois.data_ptr(), scores.data_ptr(), labels.data_ptr(), num.data_ptr(), B, S, Rr, box_dim, views,
                                 (ctypes.c_double * S)(*([1.0] * S)), thr, 0.0, 10, outs[0].data_ptr(), outs[1].data_ptr(),
                                 outs[2].data_ptr(), outs[3][0].data_ptr(), outs[3][1].data_ptr(), None, None, ws.data_ptr(),
                                 ws.numel(), None)
        torch.cuda.synchronize()
        return code, all(bool((o == -3).all()) for o in outs), (rois, scores, labels, num)
    ok, untouched, args = call(2, 6, 7, 0.3)
    assert ok == 0 and not untouched                                          # the same call with good arguments does run
    for S, box_dim, thr in ((2, 8, 0.3), (17, 7, 0.3), (2, 7, float("nan"))):
        code, untouched, args = call(S, 6, box_dim, thr)
        assert code != 0 and untouched, (S, box_dim, thr)
        with pytest.raises(ValueError):
            box_fusion.fuse_padded(*args, S, iou_threshold=thr)
    assert lib.ud_box_fusion_workspace_bytes(B, 17, 6) == 0


def test_fuse_pred_dicts(hip_lib):
    """The ensemble entry point pads and stacks pred_dicts and returns what fuse_padded gives."""
    from unidistill_amd.ops import box_fusion
    name = "s4_r5_ensemble"
    seed, S, Rr, box_dim, n_labels, views, weights = CASES[name]
    inputs, ref = case(name)
    dev = torch.device("cuda:0")
    rois, scores, labels, num = (torch.tensor(a).to(dev) for a in inputs)
    sources = [[{"pred_boxes": rois[s * B + b, :int(num[s * B + b])], "pred_scores": scores[s * B + b, :int(num[s * B + b])],
                 "pred_labels": labels[s * B + b, :int(num[s * B + b])]} for b in range(B)] for s in range(S)]
    pds = box_fusion.fuse(sources, weights=weights, iou_threshold=THR)
    want = box_fusion.fuse_padded(rois, scores, labels, num, S, weights=weights, iou_threshold=THR)
    for b, n in enumerate(box_fusion.read_num(want[3])):
        assert n == len(ref[b]["rows"]) and pds[b]["pred_boxes"].shape == (n, box_dim)
        assert torch.equal(pds[b]["pred_boxes"], want[0][b, :n]) and torch.equal(pds[b]["pred_scores"], want[1][b, :n])
        assert torch.equal(pds[b]["pred_labels"], want[2][b, :n])


def _dense_boxes(n):
    """n boxes of one label drawn so densely (four square metres of ground per box) that greedy NMS at THR drops about three in
    ten; the last one lies almost on the first."""
    rng = np.random.default_rng(100 + n)
    half = max(1.0, 0.5 * np.sqrt(4.0 * n))
    b = np.zeros((n, 7), np.float32)
    b[:, 0:2] = rng.uniform(-half, half, (n, 2))
    b[:, 2] = rng.uniform(-1, 1, n)
    b[:, 3:6] = rng.uniform(1.0, 4.5, (n, 3))
    b[:, 6] = rng.uniform(-3.1, 3.1, n)
    if n > 1:
        b[n - 1] = b[0]
        b[n - 1, 0] += 0.1
    return b


@pytest.mark.parametrize("n", [1, 64, 65, 4096, 4100])
def test_nms_keep_list_is_the_set_of_fusion_anchors(hip_lib, n):
    """The one-wave NMS scan (csrc/nms_scan.h) has an instantiation in ud_nms_rotated_bev and one in box fusion: on one label,
    strictly descending scores and one identity source both walk the same boxes in the same order, so the anchors of the fused
    clusters are the NMS keep list and every box is a member of exactly one cluster.  n crosses a mask word (64 / 65) and a
    lane's first word (4096 / 4100).  On the CPU, with the reference's IoU: box 0 is kept whatever follows, so every box that it
    overlaps by more than THR is suppressed -- the last one at least: neither set is empty."""
    from unidistill_amd.ops import nms
    boxes = _dense_boxes(n)
    scores = np.linspace(0.9, 0.1, n, dtype=np.float32)
    assert n == 1 or (np.diff(scores) < 0).all()
    first = [float(x) for x in boxes[0]]
    iou0 = np.array([R.iou_bev64(first, [float(x) for x in boxes[j]]) for j in range(1, n)])
    thr32 = float(np.float32(THR))
    assert (np.abs(iou0 - thr32) >= MIN_MARGIN).all()
    under_first = 1 + np.flatnonzero(iou0 > thr32)
    assert n == 1 or under_first[-1] == n - 1

    kept, count = nms._run(torch.from_numpy(boxes).cuda(), THR)
    keep = kept[:int(count.item())].cpu().numpy()
    assert keep[0] == 0 and not np.isin(under_first, keep).any()
    got, num = run((boxes[None], scores[None], np.ones((1, n), np.int64), np.array([n], np.int32)), 1, iou_threshold=THR,
                   max_out=n)
    anchor, members = got[4][0], got[5][0]
    assert num == [len(keep)]
    assert np.array_equal(np.sort(anchor[:num[0]]), keep)
    assert int(members.sum()) == n
