"""CPU: invariants of the float64 box-fusion reference (tests/box_fusion_reference.py) and the host-side checks of
train.ValidationStep's tta_level keyword."""
import numpy as np
import pytest
import torch

import box_fusion_reference as R


def _scene(rng, n, box_dim=9, spread=40.0):
    """n well separated boxes (centres on a jittered 8 m lattice, sizes below 5 m): NMS-clean at any threshold."""
    cells = rng.permutation(100)[:n]
    b = np.zeros((n, box_dim))
    b[:, 0] = (cells % 10) * 8.0 - spread + rng.uniform(-1, 1, n)
    b[:, 1] = (cells // 10) * 8.0 - spread + rng.uniform(-1, 1, n)
    b[:, 2] = rng.uniform(-2, 1, n)
    b[:, 3:6] = rng.uniform(0.5, 4.5, (n, 3))
    b[:, 6] = rng.uniform(-3.1, 3.1, n)
    if box_dim == 9:
        b[:, 7:9] = rng.uniform(-5, 5, (n, 2))
    return b


def test_clean_single_source_comes_back_unchanged():
    rng = np.random.default_rng(0)
    n = 17
    boxes = _scene(rng, n).astype(np.float32)
    scores = rng.uniform(0.1, 0.9, n).astype(np.float32)
    labels = rng.integers(1, 4, n)
    ref = R.fuse_reference(boxes[None], scores[None], labels[None], [n], 1, iou_threshold=0.1)[0]
    assert ref["clusters"] == n and (ref["members"] == 1).all()
    by_score = np.argsort(-scores, kind="stable")
    assert np.array_equal(ref["anchor"], by_score)
    assert np.array_equal(ref["rows"][:, :6], boxes[by_score, :6].astype(np.float64))
    assert np.array_equal(ref["rows"][:, 7:], boxes[by_score, 7:].astype(np.float64))
    assert np.abs(ref["rows"][:, 6] - boxes[by_score, 6]).max() <= 1e-15            # the wrap into [-pi, pi) is one rounding
    assert np.array_equal(ref["scores"], scores[by_score].astype(np.float64))
    assert np.array_equal(ref["labels"], labels[by_score])


def test_own_views_fuse_back_to_the_scene():
    """A scene with its flipped, rotated and scaled copies (float64 views, exact un-view): one cluster per object, the object's
    own box within 1e-12 and its own score."""
    rng = np.random.default_rng(1)
    n = 12
    boxes = _scene(rng, n)
    scores = rng.uniform(0.2, 0.9, n)
    labels = rng.integers(1, 3, n)
    views = [(0.0, 1.0, 0, 0), (0.0, 1.0, 1, 0), (0.0, 1.0, 0, 1), (7.5, 0.95, 1, 1), (-11.0, 1.05, 0, 1), (90.0, 1.0, 1, 0)]
    S = len(views)
    rois = np.stack([R.make_views(boxes, v) for v in views])
    ref = R.fuse_reference(rois, np.tile(scores, (S, 1)), np.tile(labels, (S, 1)), [n] * S, S, views=views,
                           iou_threshold=0.5, dtype=np.float64)[0]
    assert ref["clusters"] == n and (ref["members"] == S).all()
    by_score = np.argsort(-scores, kind="stable")
    got, want = ref["rows"], boxes[by_score]
    dyaw = (got[:, 6] - want[:, 6] + np.pi) % (2 * np.pi) - np.pi
    assert np.abs(np.delete(got - want, 6, 1)).max() <= 1e-12 and np.abs(dyaw).max() <= 1e-12
    assert np.abs(ref["scores"] - scores[by_score]).max() <= 1e-15
    assert np.array_equal(ref["labels"], labels[by_score])


def test_score_scales_with_the_share_of_sources():
    """A cluster present in k of S unit-weight sources: mean score * k / S."""
    S, k = 5, 3
    box = np.array([1.0, 2.0, 0.0, 4.0, 2.0, 1.5, 0.3], np.float32)
    rois = np.tile(box, (S, 1, 1))
    scores = np.array([[0.9], [0.5], [0.7], [0.0], [0.0]], np.float32)
    num = [1, 1, 1, 0, 0]
    ref = R.fuse_reference(rois, scores, np.ones((S, 1), np.int64), num, S, iou_threshold=0.5)[0]
    assert ref["clusters"] == 1 and ref["members"][0] == k
    mean = (float(np.float32(0.9)) + 0.5 + float(np.float32(0.7))) / 3
    assert abs(ref["scores"][0] - mean * k / S) <= 1e-15
    # present in every source: the plain mean
    full = R.fuse_reference(rois[:k], scores[:k], np.ones((k, 1), np.int64), [1] * k, k, iou_threshold=0.5)[0]
    assert abs(full["scores"][0] - mean) <= 1e-15
    # two boxes of one source in a cluster: sum of member weights exceeds the sources' and takes over
    two = R.fuse_reference(np.tile(box, (1, 2, 1)), np.array([[0.8, 0.4]], np.float32), np.ones((1, 2), np.int64), [2], 1,
                           iou_threshold=0.5)[0]
    assert two["members"][0] == 2 and abs(two["scores"][0] - (float(np.float32(0.8)) + float(np.float32(0.4))) / 2) <= 1e-15


def test_chain_does_not_merge_through_a_suppressed_box():
    """A ~ B, B ~ C, A !~ C with descending scores: {A, B} and {C}: a suppressed box suppresses nobody."""
    def box(x):
        return [x, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0]
    rois = np.array([[box(0.0), box(1.0), box(2.0)]], np.float32)       # IoU 0.6 for a shift of 1, 1/3 for 2
    scores = np.array([[0.9, 0.8, 0.7]], np.float32)
    assert abs(R.iou_bev64(rois[0, 0], rois[0, 1]) - 0.6) < 1e-12 and abs(R.iou_bev64(rois[0, 0], rois[0, 2]) - 1 / 3) < 1e-12
    ref = R.fuse_reference(rois, scores, np.ones((1, 3), np.int64), [3], 1, iou_threshold=0.5)[0]
    assert ref["anchor_of"] == [0, 0, 2] and list(ref["members"]) == [2, 1]
    assert list(ref["anchor"]) == [0, 2]
    # other labels never meet
    ref = R.fuse_reference(rois, scores, np.array([[1, 2, 1]]), [3], 1, iou_threshold=0.5)[0]
    assert ref["clusters"] == 3


def test_yaw_folds_half_turns():
    """A member turned by pi has the same footprint: it pulls the fused yaw nowhere."""
    a = [0.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.2]
    b = [0.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.2 + np.pi - 0.02]
    ref = R.fuse_reference(np.array([[a, b]]), np.array([[0.8, 0.8]]), np.ones((1, 2), np.int64), [2], 1, iou_threshold=0.5,
                           dtype=np.float64)[0]
    assert ref["clusters"] == 1 and abs(ref["rows"][0, 6] - 0.19) <= 1e-12


class _Model(torch.nn.Module):
    pass


def test_validation_step_checks_tta_level():
    from unidistill_amd import train
    with pytest.raises(ValueError, match="tta_level"):
        train.ValidationStep(_Model(), None, tta_level="bogus")
    with pytest.raises(ValueError, match="tta is None"):
        train.ValidationStep(_Model(), None, tta_level="boxes")
    step = train.ValidationStep(_Model(), None)
    assert step.tta_level == "maps" and step.ensemble == []
    step = train.ValidationStep(_Model(), None, tta="double_flip", tta_level="boxes")
    assert step.tta_level == "boxes" and len(step.tta_views) == 4
    with pytest.raises(ValueError, match="weights"):
        train.ValidationStep(_Model(), None, ensemble=[(_Model(), 0.0)])


def test_head_defaults_to_map_merging():
    from unidistill_amd.layers.center_head import CenterHead
    assert CenterHead.tta_level == "maps" and CenterHead.tta_views is None
