"""GPU: flip test-time augmentation wired through the head (CenterHead.tta_views) and train.ValidationStep(tta=...)."""
import numpy as np
import pytest
import torch

import tta_reference as R

pytestmark = pytest.mark.gpu

B, H, W = 2, 32, 32
THR = 0.1                      # the proposal layer's score threshold (config.DET_HEAD)


def _peak_pattern(rng, ncs):
    """Per task a base heat map [B, nc, H, W]: -8 everywhere (score 3e-4) and, per sample and class, ten peaks on distinct
    pixels of a 3-cell lattice; the 10 * nc peaks of a sample and task have logits -1.5 .. 1.5 in equal steps (0.3 / nc:
    scores 0.18 .. 0.8, at least 0.02 apart)."""
    out = []
    for nc in ncs:
        hm = np.full((B, nc, H, W), -8.0, np.float32)
        for b in range(B):
            slots = rng.permutation(100)[:10 * nc]
            for j, s in enumerate(slots):
                hm[b, j // 10, 1 + 3 * (s // 10), 1 + 3 * (s % 10)] = -1.5 + 0.3 / nc * j
        out.append(hm)
    return out


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
def test_head_merges_views_before_the_proposal_layer(hip_lib, lenient, packed):
    """CenterHeadIouAware (project configuration, 32 x 32 BEV map) on 4 * B random feature rows: with tta_views = DOUBLE_FLIP the
    B pred_dicts equal the unchanged proposal layer run on merge32 of the maps the same head returns without a proposal layer
    -- same counts, same labels, bitwise boxes.

    How the comparison is made exact.  The two paths read identical bits of reg, height, rot, vel and iou (linear heads:
    bitwise merge32), so a box can only differ through hm (ranking, threshold) and dim (device logf against libm).  A forward
    hook on the head's conv stacks therefore (a) scales the random heat map to +-0.01 logits around a fixed pattern -- the
    flipped images of one base pattern per view, -8 off the peaks, peaks >= 0.15 logits apart -- so that merged scores of the
    candidates differ by >= 0.02 and stay clear of the score threshold, (b) scales the iou map by 1e-3, so that the NMS score
    score^0.35 * iou^0.65 keeps the order and a spacing >= 1e-3 (both asserted below on the merged maps), and (c) zeroes dim:
    exp(0) = 1 and log(1) = 0 are exact in every libm, so both paths decode the size 1.  dim's own merge is tested in
    test_tta_merge_gpu.py.  An ulp of hm then cannot move a candidate across the spacing, and boxes, which do not hold the
    score, are bitwise equal."""
    from unidistill_amd import config as C
    from unidistill_amd.models import DetHead
    from unidistill_amd.layers.center_head import CenterHeadIouAware
    from unidistill_amd.ops import tta
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = C.model_cfg(lidar=True, camera=False)["det_head"]
    det = DetHead(cfg)
    head = det.dense_head
    if not packed:
        head = CenterHeadIouAware(
            dataset_name="nuscenes", tasks=cfg["tasks"], target_assigner=head.target_assigner, proposal_layer=head.proposal_layer,
            out_size_factor=cfg["out_size_factor"], input_channels=cfg["input_channels"], grid_size=cfg["grid_size"],
            point_cloud_range=cfg["point_cloud_range"], code_weights=cfg["code_weights"], loc_weight=cfg["loc_weight"],
            iou_weight=cfg["iou_weight"], share_conv_channel=cfg["share_conv_channel"], common_heads=cfg["common_heads"],
            init_bias=cfg["init_bias"], voxel_size_xy=cfg["voxel_size"][0:2], packed_heads=False)
    head = head.to(dev).eval()
    prop = head.proposal_layer
    ncs = head.num_classes
    views = tta.DOUBLE_FLIP
    V = len(views)
    rng = np.random.default_rng(0)
    pattern = [torch.from_numpy(p["hm"]).to(dev) for p in R.make_views([{"hm": hm} for hm in _peak_pattern(rng, ncs)], views)]

    seen = []                                       # the shaped maps of every forward, task by task

    def shape(out, t):
        out["hm"].mul_(0.01).add_(pattern[t])
        out["iou"].mul_(1e-3)
        out["dim"].zero_()
        seen.append({k: v.float().cpu().numpy() for k, v in out.items()})
        return out
    if packed:                                      # one module returns the list over tasks
        hooks = [head.tasks.register_forward_hook(lambda mod, inp, out: [shape(d, t) for t, d in enumerate(out)])]
    else:                                           # a ModuleList of SepHeads: the same edit after each task's stack
        hooks = [task.register_forward_hook(lambda mod, inp, out, t=t: shape(out, t)) for t, task in enumerate(head.tasks)]
    x = torch.randn(V * B, cfg["input_channels"], H, W, device=dev)
    T = len(ncs)
    with torch.no_grad():
        assert head.tta_views is None
        plain = head(x)["pred_dicts"]               # before the attribute is ever set: the parent commit's path
        assert len(plain) == V * B
        head.proposal_layer = None
        maps = head(x)["multi_head_features"]
        head.proposal_layer = prop
        returned = [{k: v.float().cpu().numpy() for k, v in m.items()} for m in maps]
        head.tta_views = views
        got = head(x)["pred_dicts"]
        head.tta_views = None
        plain_again = head(x)["pred_dicts"]
    for h in hooks:
        h.remove()
    assert len(seen) == 4 * T
    # The maps the merge read.  The hand-written kernels of the packed head are bitwise reproducible, so these are the maps the
    # head returns without a proposal layer (asserted); the unpacked head's library convolutions differ between two calls by
    # their own rounding (1e-6 observed), so there the maps of the very forward that was merged are the ones compared.
    host = seen[2 * T:3 * T]
    if packed:
        for a, c in zip(returned, host):
            assert set(a) == set(c) and all(np.array_equal(a[k], c[k]) for k in a)
    assert len(got) == B
    merged = R.merge32(host, views, prop.no_log)
    # the premise: candidates' NMS scores >= 1e-3 apart per sample and task, none near the score threshold
    for t, m in enumerate(merged):
        s = R.sigmoid64(m["hm"])
        q = np.clip(m["iou"].astype(np.float64) / 2 + 0.5, 0, 1)
        nms = s ** 0.35 * q ** 0.65
        assert not ((s > THR / 2) & (s < 1.5 * THR)).any()
        for b in range(B):
            cand = np.sort(nms[b][s[b] > THR])
            assert len(cand) == 10 * ncs[t] and np.diff(cand).min() >= 1e-3, (t, b, np.diff(cand).min())
        assert np.array_equal(m["dim"], np.zeros_like(m["dim"]))
    with torch.no_grad():
        want = prop.generate_predicted_boxes(
            {"multi_head_features": [{k: torch.from_numpy(v).to(dev) for k, v in m.items()} for m in merged]}, {})["pred_dicts"]
    assert len(want) == B
    for b in range(B):
        n = want[b]["pred_boxes"].shape[0]
        assert n >= 30 and got[b]["pred_boxes"].shape == (n, 9)
        assert torch.equal(got[b]["pred_labels"], want[b]["pred_labels"])
        assert torch.equal(got[b]["pred_boxes"], want[b]["pred_boxes"])
        assert torch.allclose(got[b]["pred_scores"], want[b]["pred_scores"], rtol=1e-5, atol=0)
    # the views really differ, so the merge was needed: view 0 alone decodes other boxes
    assert not all(plain[b]["pred_boxes"].shape == got[b]["pred_boxes"].shape and torch.equal(plain[b]["pred_boxes"], got[b]["pred_boxes"])
                   for b in range(B))
    # and with the attribute back at None the plain path is what it was: bit for bit on the reproducible kernels
    assert len(plain_again) == V * B
    for a, c in zip(plain, plain_again):
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert a[k].shape == c[k].shape and (not packed or torch.equal(a[k], c[k])), k


class _Collect:
    def __init__(self):
        self.calls = []

    def add_batch(self, ids, preds, l2g):
        self.calls.append((list(ids), preds))


def test_validation_step_with_double_flip(hip_lib):
    """The LiDAR model of the project's configuration on one synthetic sample: four views in one forward, B pred_dicts out."""
    from unidistill_amd import train
    from unidistill_amd.ops import tta
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = train.build_model("lidar").to(dev)
    head = model.det_head.dense_head
    batch = train.synthetic_batch(dev, 1, with_imgs=False)
    seen = _Collect()
    plain_before = train.ValidationStep(model, _Collect())(batch, [7], None)
    step = train.ValidationStep(model, seen, tta="double_flip")
    assert step.tta_views == tta.DOUBLE_FLIP
    pds = step(batch, [7], None)
    assert model.training and head.tta_views is None
    assert len(pds) == 1 and len(seen.calls) == 1 and seen.calls[0][0] == [7] and seen.calls[0][1] is pds
    lo, hi = (torch.tensor(head.proposal_layer.post_center_limit_range[i:i + 3], device=dev) for i in (0, 3))
    boxes = pds[0]["pred_boxes"]
    assert boxes.shape[1] == 9 and boxes.shape[0] > 0
    assert bool((boxes[:, :3] >= lo).all()) and bool((boxes[:, :3] <= hi).all())
    assert pds[0]["pred_labels"].min() >= 1 and pds[0]["pred_labels"].max() <= 10
    # a plain step afterwards is the plain step: the head is back as it was
    plain = train.ValidationStep(model, _Collect())(batch, [7], None)
    for k in ("pred_boxes", "pred_scores", "pred_labels"):
        assert torch.equal(plain[0][k], plain_before[0][k]), k
    # an exception inside the forward leaves nothing behind
    fwd = model.forward

    def boom(*a, **kw):
        assert head.tta_views == tta.DOUBLE_FLIP
        raise RuntimeError("boom")
    model.forward = boom
    try:
        with pytest.raises(RuntimeError, match="boom"):
            step(batch, [7], None)
    finally:
        model.forward = fwd
    assert head.tta_views is None and model.training and len(seen.calls) == 1
    # an asymmetric range is refused before anything runs
    rng_before = head.point_cloud_range
    head.point_cloud_range = [0.0, -54.0, -5.0, 108.0, 54.0, 3.0]
    try:
        with pytest.raises(ValueError, match="x axis"):
            step(batch, [7], None)
    finally:
        head.point_cloud_range = rng_before
    assert head.tta_views is None
    with pytest.raises(ValueError):
        train.ValidationStep(model, seen, tta=[(0, 0)] * 5)


def test_validation_step_tta_with_depth_metric(hip_lib):
    """tta together with depth_metric measures view 0 alone: exactly the B samples' labelled pixels are added, with the figures of
    the plain step; a view list that does not start unflipped is refused."""
    from unidistill_amd import _lib, evaluation, train
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = train.build_model("camera").to(dev)
    enc = model.camera_encoder.backbone
    batch = train.synthetic_batch(dev, 1, ncam=1)
    m_tta, m_plain = (evaluation.DepthMetric(enc.d_bound, ncam=1, device=dev) for _ in range(2))
    # the camera model's eval-mode image BatchNorm on NCHW activations has no hand-written kernel: library path allowed
    with _lib.strict(False):
        pds = train.ValidationStep(model, _Collect(), depth_metric=m_tta, tta="double_flip")(batch, [0], None)
        train.ValidationStep(model, _Collect(), depth_metric=m_plain)(batch, [0], None)
        with pytest.raises(ValueError, match="view 0"):
            train.ValidationStep(model, _Collect(), depth_metric=m_tta, tta=[(1, 0), (0, 0)])(batch, [0], None)
    assert len(pds) == 1 and model.det_head.dense_head.tta_views is None
    a, b = m_tta.compute(), m_plain.compute()
    assert a["n"] == b["n"] > 20
    # view 0's images and matrices are the batch's own: the same logits up to the batch size's effect on the kernels' sums
    assert abs(a["abs_rel"] - b["abs_rel"]) <= 1e-3 * b["abs_rel"]
