"""CPU: the float64 all-anchors restatement of target assignment (tests/assign_reference.py) against the
recorded output of the original project, against hand-computed cases, and as the yardstick of the two tensor-op
formulations of FCOSAssigner on the case matrix of tests/assign_cases.py."""
import numpy as np
import pytest
import torch

import assign_cases as C
from assign_reference import assign_reference, encoding_bound


# ---------------------------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------------------------
def test_reference_reproduces_the_recorded_targets(golden):
    """tests/golden/dense_head.npz holds head_gt and the targets the original module produced for it (32 x 32
    anchors, top-k 9, K = 200): integer targets exactly, encodings within the float32 bound."""
    g = golden("dense_head")
    gt = g["head_gt"]
    args = ((32, 32), 8, [-32.0, -32.0], [0.25, 0.25])
    ref, margin, _ = assign_reference(gt, C.TASKS, C.CLASS_MAP, *args, topk=9, K=200, default_box_dims=10)
    bound = encoding_bound(gt, ref, *args)
    assert margin > 0
    for t in range(3):
        for key in ("heatmap", "ind", "mask", "cat"):
            np.testing.assert_array_equal(ref[key][t], g[f"head_tgt{t}_{key}"], err_msg=f"{key}[{t}]")
        rec = g[f"head_tgt{t}_box_encoding"].astype(np.float64)
        want = ref["box_encoding"][t]
        assert rec.shape == want.shape
        fin = np.isfinite(want)
        assert np.isfinite(rec[fin]).all()
        assert (np.abs(rec - want)[fin] <= bound[t][fin]).all(), np.abs(rec - want)[fin].max()


def _tiny(rows, w=9, h=9, topk=1, K=12, cols=10, default_box_dims=10):
    """Cell 1 m (out_size_factor 1, voxel 1 m), range from (0, 0): a centre (x, y) is at anchor coordinates (x, y)."""
    gt = np.zeros((1, len(rows), cols), np.float32)
    for m, (x, y, cls) in enumerate(rows):
        if cls is not None:
            gt[0, m] = [x, y, 0.5, 2.0, 3.0, 4.0, 0.0, 0.25, -0.5, cls][:cols - 1] + [cls]
    return gt, assign_reference(gt, [["a"], ["b", "c"]], {"a": 1, "b": 2, "c": 3}, (w, h), 1, [0.0, 0.0], [1.0, 1.0],
                                topk, K, default_box_dims)


def test_reference_one_box_on_an_anchor_top1():
    gt, (ref, margin, _) = _tiny([(4.0, 6.0, 1)])
    assert ref["ind"][0][0, 0] == 6 * 9 + 4 and ref["mask"][0][0].tolist() == [True] + [False] * 11
    assert ref["cat"][0][0, 0] == 0 and ref["heatmap"][0].sum() == 1 and ref["heatmap"][0][0, 0, 6, 4] == 1
    np.testing.assert_allclose(ref["box_encoding"][0][0, 0],
                               [0, 0, 0.5, np.log(2.0), np.log(3.0), np.log(4.0), 0.0, 1.0, 0.25, -0.5], atol=1e-15)
    assert not ref["box_encoding"][0][0, 1:].any() and ref["row"][0][0].tolist() == [0] + [-1] * 11
    assert margin == 1.0                                   # nearest at distance 0, the next at 1: (1 - 0) / 1
    assert not ref["mask"][1].any() and not ref["heatmap"][1].any()


def test_reference_one_box_on_an_anchor_top5():
    """Centre, then the four neighbours at distance 1; the next four are at squared distance 2: margin 1 / 2."""
    gt, (ref, margin, _) = _tiny([(4.0, 6.0, 3)], topk=5)
    a = 6 * 9 + 4
    assert ref["ind"][1][0, :5].tolist() == [a - 9, a - 1, a, a + 1, a + 9] and ref["mask"][1][0].sum() == 5
    assert ref["cat"][1][0, :5].tolist() == [1] * 5 and ref["heatmap"][1][0, 1].sum() == 5
    assert not ref["heatmap"][1][0, 0].any() and not ref["mask"][0].any()
    np.testing.assert_allclose(ref["box_encoding"][1][0, :5, :2], [[0, 1], [1, 0], [0, 0], [-1, 0], [0, -1]], atol=0)
    assert margin == 0.5


def test_reference_two_boxes_equidistant_from_a_positive():
    """b (row 0, x = 4.25) and c (row 1, x = 3.75) around anchor x = 4, and a second b in row 2 on the other
    side at the same distance as row 0... task order is (class offset, row): rows 0, 2 (b), then row 1 (c)."""
    gt, (ref, margin, row_margin) = _tiny([(4.25, 2.0, 2), (3.75, 2.0, 3), (3.75, 2.0, 2)])
    assert ref["ind"][1][0, 0] == 2 * 9 + 4 and ref["mask"][1][0].sum() == 1
    assert ref["row"][1][0, 0] == 0 and ref["cat"][1][0, 0] == 0          # first in task order among three equals
    assert ref["box_encoding"][1][0, 0, 0] == 0.25
    assert margin == 0.0 and (row_margin[0] == 0).all()
    # without row 0 the two remaining tie, and class b (row 2) is ahead of class c (row 1)
    gt, (ref, margin, _) = _tiny([(4.25, 2.0, None), (3.75, 2.0, 3), (3.75, 2.0, 2)])
    assert ref["row"][1][0, 0] == 2 and ref["cat"][1][0, 0] == 0


def test_reference_zero_row_before_the_last_valid_one_and_trailing_rows():
    """Row 1 is all zero but precedes a valid row: it stays in the sample, with class id 0, which no task lists.
    Rows after the last non-zero one are dropped even when they carry a class id."""
    gt, (ref, _, _) = _tiny([(2.0, 2.0, 1), (0.0, 0.0, None), (6.0, 5.0, 1), (0.0, 0.0, None)])
    assert ref["ind"][0][0, :2].tolist() == [2 * 9 + 2, 5 * 9 + 6] and ref["row"][0][0, :2].tolist() == [0, 2]
    gt = gt.copy()
    gt[0, 3, -1] = 1.0                                      # zero box after the last valid row: not a member
    ref2 = assign_reference(gt, [["a"], ["b", "c"]], {"a": 1, "b": 2, "c": 3}, (9, 9), 1, [0.0, 0.0], [1.0, 1.0], 1, 12, 10)[0]
    assert ref2["mask"][0][0].sum() == 2
    gt[0, 1, -1] = 1.0                                      # zero box before it: a member, centred on anchor 0
    ref3 = assign_reference(gt, [["a"], ["b", "c"]], {"a": 1, "b": 2, "c": 3}, (9, 9), 1, [0.0, 0.0], [1.0, 1.0], 1, 12, 10)[0]
    assert ref3["ind"][0][0, :3].tolist() == [0, 2 * 9 + 2, 5 * 9 + 6] and ref3["row"][0][0, :3].tolist() == [1, 0, 2]
    assert np.isneginf(ref3["box_encoding"][0][0, 0, 3:6]).all()


def test_reference_slots_overflow_and_lower_index_first():
    """top-k 3 on an anchor: the centre and the two lower-index neighbours of the four at distance 1.  K = 2 keeps
    the first two in anchor order; the heat map keeps all three."""
    gt, (ref, margin, _) = _tiny([(4.0, 6.0, 1)], topk=3, K=2)
    a = 6 * 9 + 4
    assert ref["ind"][0][0].tolist() == [a - 9, a - 1] and ref["mask"][0][0].all()
    assert np.flatnonzero(ref["heatmap"][0][0, 0]).tolist() == [a - 9, a - 1, a] and margin == 0.0


# ---------------------------------------------------------------------------------------------
# the tensor-op formulations against the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", C.RANDOM_IDS)
def test_redraws_stay_within_one_percent(cid):
    cfg = C.case(cid)
    assert cfg.margin >= C.MARGIN
    assert cfg.n_redrawn <= 0.01 * cfg.n_boxes, (cfg.n_redrawn, cfg.n_boxes)


@pytest.mark.parametrize("windowed", [False, True], ids=["dense", "windowed"])
@pytest.mark.parametrize("cid", C.RANDOM_IDS)
def test_tensor_formulation_equals_reference(cid, windowed):
    cfg = C.case(cid)
    asg = C.make_assigner(cfg)
    asg.windowed = windowed
    got = asg.assign_targets(torch.from_numpy(cfg.gt.copy()))
    C.check(got, cfg, f"{cid}/{'windowed' if windowed else 'dense'}")
    print("worst |error| / bound per encoding column so far:", {k: round(v, 3) for k, v in sorted(C.worst_ratio.items())})
