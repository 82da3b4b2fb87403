"""GPU: the whole chain at small size -- `pred_dicts` through `NuScenesDetectionEval.add_batch`, `compute()`,
`NuScenesTracker.track` and `NuScenesTrackingEval.compute` -- against tests/track_metric_reference.py run on the evaluator's own
rows and the tracker's ids.  The detection summary and the track ids are unchanged by the metric."""
import json
import math

import numpy as np
import pytest
import torch

import track_metric_reference as R
from test_tracking_eval_gpu import _chain, _evaluator


@pytest.mark.gpu
def test_detection_to_tracking_summary():
    from unidistill_amd.evaluation import (CLASS_NAMES, TRACKING_NAMES, TRACKING_NIPS_2019, NuScenesTracker,
                                           NuScenesTrackingEval)
    assert R.CLASS_NAMES == CLASS_NAMES and sorted(R.TRACKING_CLASSES) == TRACKING_NAMES
    assert TRACKING_NIPS_2019["metric_worst"] == R.METRIC_WORST and TRACKING_NIPS_2019["class_range"] == R.CLASS_RANGE
    dev = torch.device("cuda", 0)
    scene, ts, l2g, pds, gt = _chain()
    ev = _evaluator(dev, l2g, pds, gt)
    G = len(gt["cls"])
    objects = G // len(scene)
    instance = np.array([(s % 2) * 1000 + o for s in range(len(scene)) for o in range(objects)], np.int64)   # per scene, object
    num_pts = np.full(G, 5)
    num_pts[3] = 0
    keep = np.ones(G, bool)
    keep[7] = False
    tev = NuScenesTrackingEval(class_names=CLASS_NAMES, cfg=TRACKING_NIPS_2019, device=dev)
    tev.add_ground_truth(gt["translation"], gt["cls"], instance, num_pts, gt["sample"], l2g[:, :3, 3], scene, ts, keep=keep)
    tr = NuScenesTracker()
    with pytest.raises(RuntimeError, match="track"):
        tr.last_tracks()
    strip = lambda s: json.dumps({k: v for k, v in s.items() if k != "eval_time"}, sort_keys=True)
    before = strip(ev.compute())
    ids = tr.track(ev, scene, ts)["track_id"].clone()
    summary = tev.compute(tr)
    assert strip(ev.compute()) == before and torch.equal(tr.track(ev, scene, ts)["track_id"], ids)
    pred, layout, tids, tscene = tr.last_tracks()
    assert tids.is_cuda and np.array_equal(tscene, scene)

    tracked, rng = R.default_config(CLASS_NAMES)
    order = tev.gt_order
    off = tev.gt["off"]
    ref = R.evaluate_reference(pred["rec"].cpu().numpy(), pred["cls"].cpu().numpy(), tids.cpu().numpy(), layout["start"],
                               layout["count"], gt["translation"][order], gt["cls"][order], instance[order], num_pts[order],
                               keep[order], off, l2g[:, :3, 3], scene, ts, tracked=tracked, class_range=rng,
                               recall=R.recall_thresholds())
    curves = tev.last_curves()
    names = [n for n, t in zip(CLASS_NAMES, tracked) if t]
    assert curves["classes"] == names and np.array_equal(curves["counts"], ref["counts"])
    assert curves["thresholds"].tobytes() == ref["thresholds"].tobytes() and ref["counts"][:, 0, 2].sum() > 10
    want = R.summarize_reference(ref, names, R.recall_thresholds())
    assert set(summary) == set(want) | {"eval_time", "cfg"} and summary["cfg"] == TRACKING_NIPS_2019
    for m in R.METRIC_WORST:
        for got, exp in [(summary[m], want[m])] + [(summary["label_metrics"][m][n], want["label_metrics"][m][n]) for n in names]:
            assert (math.isnan(got) and math.isnan(exp)) or abs(got - exp) <= 1e-12 * max(1.0, abs(exp)), (m, got, exp)
    assert summary["tp"] > 10
