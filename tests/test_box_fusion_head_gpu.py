"""GPU: box-level fusion wired through the head (CenterHead.tta_level = "boxes") and train.ValidationStep(tta_level=...,
ensemble=...)."""
import copy

import numpy as np
import pytest
import torch

import box_fusion_reference as R
import tta_reference as TR
from test_box_fusion_gpu import EPS32, K, MIN_MARGIN
from test_tta_head_gpu import B, H, W, _Collect, _peak_pattern

pytestmark = pytest.mark.gpu


def _small_head(dev):
    from unidistill_amd import config as C
    from unidistill_amd.models import DetHead
    torch.manual_seed(0)
    cfg = C.model_cfg(lidar=True, camera=False)["det_head"]
    return DetHead(cfg).dense_head.to(dev).eval(), cfg


def _shape_maps(head, views, dev):
    """The hook of test_tta_head_gpu.py: heat maps +-0.01 logits around the flipped images of one peak pattern per view, iou
    scaled by 1e-3, dim zeroed (size 1); here reg is also pulled to 0.5 +- 0.01 cells, so that the views' boxes of one peak
    coincide within centimetres after the un-view and clusters are far from the IoU threshold (asserted by the margin)."""
    rng = np.random.default_rng(0)
    pattern = [torch.from_numpy(p["hm"]).to(dev)
               for p in TR.make_views([{"hm": hm} for hm in _peak_pattern(rng, head.num_classes)], views)]

    def shape(out, t):
        out["hm"].mul_(0.01).add_(pattern[t])
        out["iou"].mul_(1e-3)
        out["dim"].zero_()
        out["reg"].mul_(0.01).add_(0.5)
        return out
    return head.tasks.register_forward_hook(lambda mod, inp, out: [shape(d, t) for t, d in enumerate(out)])


def test_head_fuses_the_views_boxes(hip_lib, lenient):
    """CenterHeadIouAware (project configuration, 32 x 32 map) on 4 * B feature rows with tta_views = DOUBLE_FLIP and tta_level =
    "boxes": the B pred_dicts are the reference's fusion of the proposal layer's own V * B padded outputs -- counts, labels and
    order exact, floats within 4 eps32."""
    from unidistill_amd.ops import tta
    dev = torch.device("cuda:0")
    head, cfg = _small_head(dev)
    prop = head.proposal_layer
    # boxes carry metric coordinates: the 32 x 32 map must span a range symmetric about 0 for a flipped view's peaks to land,
    # un-viewed, on view 0's (the project's range belongs to the 180 x 180 map)
    prop.pc_range = [-0.5 * W * prop.out_size_factor * prop.voxel_size[0], -0.5 * H * prop.out_size_factor * prop.voxel_size[1]]
    views = tta.DOUBLE_FLIP
    V = len(views)
    hook = _shape_maps(head, views, dev)
    x = torch.randn(V * B, cfg["input_channels"], H, W, device=dev)
    with torch.no_grad():
        plain = head(x)                                       # the V * B samples one by one: the fusion's inputs
        head.tta_views, head.tta_level = views, "boxes"
        got = head(x)
        head.tta_views, head.tta_level = None, "maps"
    hook.remove()
    num = [pd["pred_boxes"].shape[0] for pd in plain["pred_dicts"]]
    assert len(num) == V * B and min(num) >= 30
    thr = prop.nms_iou_threshold_test
    ref = R.fuse_reference(plain["rois"].cpu().numpy(), plain["roi_scores"].cpu().numpy(), plain["roi_labels"].cpu().numpy(),
                           num, V, views=views, iou_threshold=thr)
    assert len(got["pred_dicts"]) == B and got["rois"].shape == (B, 500, 9)
    for b, want in enumerate(ref):
        assert want["margin"] >= MIN_MARGIN, want["margin"]
        assert want["members"].max() == V and want["clusters"] < sum(num[b::B])         # the views were fused, not stacked
        pd = got["pred_dicts"][b]
        n = len(want["rows"])
        assert pd["pred_boxes"].shape == (n, 9) and pd["pred_scores"].shape == (n,)
        assert np.array_equal(pd["pred_labels"].cpu().numpy(), want["labels"])
        g, w = pd["pred_boxes"].cpu().numpy().astype(np.float64), want["rows"]
        diff = np.abs(g - w)
        diff[:, 6] = np.abs((g[:, 6] - w[:, 6] + np.pi) % (2 * np.pi) - np.pi)
        assert (diff <= K * EPS32 * np.maximum(np.abs(w), 1.0)).all()
        assert (np.abs(pd["pred_scores"].cpu().numpy() - want["scores"]) <= K * EPS32).all()
        assert torch.equal(got["rois"][b, :n], pd["pred_boxes"]) and not bool(got["rois"][b, n:].any())


def test_default_paths_are_untouched(hip_lib, lenient):
    """tta_level = "maps" with views, and tta_views = None whatever the level: bit-identical to a head whose tta_level was never
    touched."""
    from unidistill_amd.ops import tta
    dev = torch.device("cuda:0")
    head, cfg = _small_head(dev)
    views = tta.DOUBLE_FLIP
    hook = _shape_maps(head, views, dev)
    pristine = copy.deepcopy(head)                            # carries the hook; its tta_level stays the class attribute
    assert "tta_level" not in vars(pristine) and type(head).tta_level == "maps"
    x = torch.randn(len(views) * B, cfg["input_channels"], H, W, device=dev)
    with torch.no_grad():
        want_plain = pristine(x)["pred_dicts"]
        pristine.tta_views = views
        want_maps = pristine(x)["pred_dicts"]
        head.tta_level = "boxes"                              # ignored without views
        got_plain = head(x)["pred_dicts"]
        head.tta_views, head.tta_level = views, "maps"
        got_maps = head(x)["pred_dicts"]
    hook.remove()
    assert "tta_level" not in vars(pristine)
    assert len(got_plain) == len(views) * B and len(got_maps) == B
    for got, want in ((got_plain, want_plain), (got_maps, want_maps)):
        for a, c in zip(got, want):
            assert a["pred_boxes"].shape[0] >= 30
            for k in ("pred_boxes", "pred_scores", "pred_labels"):
                assert torch.equal(a[k], c[k]), k


def test_validation_step_fuses_an_ensemble(hip_lib):
    """ValidationStep(ensemble=[(model2, 0.5)]) hands the evaluator fuse([...]) of the two models' pred_dicts; tta_level="boxes"
    runs through the whole model and restores the head."""
    from unidistill_amd import train
    from unidistill_amd.ops import box_fusion
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = train.build_model("lidar").to(dev)
    torch.manual_seed(1)
    model2 = train.build_model("lidar").to(dev)
    head = model.det_head.dense_head
    batch = train.synthetic_batch(dev, 1, with_imgs=False)
    one = train.ValidationStep(model, _Collect())(batch, [3], None)
    two = train.ValidationStep(model2, _Collect())(batch, [3], None)
    assert one[0]["pred_boxes"].shape[0] > 0 and two[0]["pred_boxes"].shape[0] > 0
    seen = _Collect()
    got = train.ValidationStep(model, seen, ensemble=[(model2, 0.5)])(batch, [3], None)
    want = box_fusion.fuse([one, two], weights=[1.0, 0.5], iou_threshold=head.proposal_layer.nms_iou_threshold_test)
    assert len(seen.calls) == 1 and seen.calls[0][0] == [3] and seen.calls[0][1] is got
    assert model.training and model2.training
    assert len(got) == 1 and 0 < got[0]["pred_boxes"].shape[0] <= one[0]["pred_boxes"].shape[0] + two[0]["pred_boxes"].shape[0]
    for k in ("pred_boxes", "pred_scores", "pred_labels"):
        assert torch.equal(got[0][k], want[0][k]), k
    # the views' boxes fused through the whole model, on a range that need not be symmetric for it
    rng_before = head.point_cloud_range
    head.point_cloud_range = [rng_before[0] + 1.0] + list(rng_before[1:])
    try:
        boxes = train.ValidationStep(model, _Collect(), tta="double_flip", tta_level="boxes")(batch, [3], None)
    finally:
        head.point_cloud_range = rng_before
    assert head.tta_views is None and head.tta_level == "maps" and model.training
    assert len(boxes) == 1 and boxes[0]["pred_boxes"].shape[1] == 9 and boxes[0]["pred_boxes"].shape[0] > 0
    assert boxes[0]["pred_labels"].min() >= 1 and boxes[0]["pred_labels"].max() <= 10
