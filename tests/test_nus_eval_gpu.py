"""GPU: the nuScenes detection metric on the device (csrc/nus_eval.hip via unidistill_amd.evaluation) against the numpy
restatement of the devkit (tests/nus_eval_reference.py): the hand-worked CPU cases, a full-size synthetic val set, the
eval forward end to end, the rejection paths, the submission JSON and two ranks gathering to rank 0."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nus_eval_reference as R
import test_nus_eval_cpu as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= TOL


def assert_summary(got, ref):
    for k in ("label_aps", "mean_dist_aps", "mean_ap", "label_tp_errors", "tp_errors", "tp_scores", "nd_score"):
        assert _same(got[k], ref[k]), (k, got[k], ref[k])


def _rows_to_pred_dicts(p, S, dev):
    """Case prediction rows (global frame) as pred_dicts under identity LiDAR->global matrices."""
    pds = []
    for s in range(S):
        rows = [r for r in p if r[0] == s]
        bx = []
        for r in rows:
            ex = r[-1] if isinstance(r[-1], dict) else {}
            w, l, h = ex.get("size", [2.0, 4.0, 1.5])
            v = ex.get("vel", [0.0, 0.0])
            bx.append([r[2], r[3], 0.5, l, w, h, ex.get("yaw", 0.0), v[0], v[1]])
        pds.append({"pred_boxes": torch.tensor(bx, dtype=torch.float32).reshape(-1, 9).to(dev),
                    "pred_scores": torch.tensor([r[4] for r in rows], dtype=torch.float32).to(dev),
                    "pred_labels": torch.tensor([r[1] + 1 for r in rows], dtype=torch.int64).to(dev)})
    return pds


def _host(pds):
    return [{k: v.cpu().numpy() for k, v in pd.items()} for pd in pds]


def _make_eval(gt, ego, dev, **kw):
    from unidistill_amd import evaluation as E
    ev = E.NuScenesDetectionEval(device=dev, **kw)
    ev.add_ground_truth(gt["translation"], gt["size"], gt["yaw"], gt["velocity"], gt["cls"], gt["attr"], gt["num_pts"],
                        gt["sample"], ego, keep=gt.get("keep"))
    return ev


def _check_detail(ev, ref_detail):
    out, _, layout = ev.compute_curves()
    counts = out["counts"].cpu().numpy()
    order = out["order"].cpu().numpy()
    tp = out["tp"].cpu().numpy()
    match = out["match_gt"].cpu().numpy()
    base = 0
    for c, name in enumerate(ev.class_names):
        n = int(counts[0, c])
        d = ref_detail[name]
        assert n == len(d["order"]) and int(counts[1, c]) == d["npos"], name
        q = order[base:base + n]
        np.testing.assert_array_equal(q, d["order"], err_msg=name)
        np.testing.assert_array_equal(tp[:, q], d["tp"], err_msg=name)
        m = match[q]
        m = np.where(m >= 0, ev.gt_order[np.maximum(m, 0)], -1)
        np.testing.assert_array_equal(m, d["match_gt"], err_msg=name)
        base += n


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_cpu_cases_on_device(hip_lib, name):
    dev = torch.device("cuda:0")
    g, p, S = cases.CASES[name]()
    gt = cases.boxes(g)
    pds = _rows_to_pred_dicts(p, S, dev)
    l2g = np.tile(np.eye(4), (S, 1, 1))
    pred = R.preds_from_dicts(_host(pds), range(S), l2g)
    ref, detail, _ = R.evaluate(gt, pred, cases.ego(S))
    ev = _make_eval(gt, cases.ego(S), dev)
    ev.add_batch(list(range(S)), pds, torch.from_numpy(l2g).to(dev))
    assert_summary(ev.compute(), ref)
    _check_detail(ev, detail)


# ---- full-size synthetic val set ------------------------------------------------------------------------------------
CLASS_P = np.array([0.43, 0.08, 0.015, 0.015, 0.02, 0.13, 0.01, 0.01, 0.19, 0.10])
SIZES = np.array([[1.9, 4.6, 1.7], [2.5, 6.9, 2.8], [2.8, 6.4, 3.2], [2.9, 11.0, 3.5], [2.9, 12.3, 3.9],
                  [2.5, 0.5, 1.0], [0.8, 2.1, 1.5], [0.6, 1.7, 1.3], [0.7, 0.7, 1.8], [0.4, 0.4, 1.1]])


def _rot(yaw, tilt):
    c, s = math.cos(yaw), math.sin(yaw)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    ct, st = math.cos(tilt), math.sin(tilt)
    Rx = np.array([[1, 0, 0], [0, ct, -st], [0, st, ct]])
    return Rz @ Rx


def synthetic_val(S=6019, seed=0, max_pred=500):
    """GT ~40 per sample with the val split's rough class mix, NaN velocities and '' attributes; per sample up to
    max_pred predictions (jittered GT + clutter) with scores on a 0.01 grid (exact ties)."""
    rng = np.random.default_rng(seed)
    ego = np.stack([rng.uniform(200, 2000, S), rng.uniform(200, 2000, S), np.zeros(S)], 1)
    l2g = np.zeros((S, 4, 4))
    for s in range(S):
        l2g[s, :3, :3] = _rot(rng.uniform(-math.pi, math.pi), rng.normal(0, 0.01))
        l2g[s, :3, 3] = ego[s] + [0.9, 0.0, 1.8]
        l2g[s, 3, 3] = 1.0
    ng = rng.poisson(40, S)
    G = int(ng.sum())
    gs = np.repeat(np.arange(S), ng)
    gc = rng.choice(10, G, p=CLASS_P)
    local = np.stack([rng.uniform(-60, 60, G), rng.uniform(-60, 60, G), rng.normal(-1, 0.5, G)], 1)
    size_l = SIZES[gc][:, [1, 0, 2]] * rng.uniform(0.8, 1.2, (G, 3))                # dx dy dz
    rot = rng.uniform(-math.pi, math.pi, G)
    vel_l = rng.normal(0, 2, (G, 2)) * (rng.random((G, 1)) < 0.5)
    gt_l = np.concatenate([local, size_l, rot[:, None], vel_l], 1).astype(np.float32)
    gt = R.preds_from_arrays(gt_l, np.zeros(G, np.float32), gc + 1, gs, l2g)
    gt["velocity"][rng.random(G) < 0.1] = np.nan
    gt["attr"] = np.where(rng.random(G) < 0.2, -1, rng.integers(0, 8, G))
    gt["num_pts"] = np.where(rng.random(G) < 0.05, 0, rng.integers(1, 500, G))
    gt["keep"] = rng.random(G) > 0.01
    del gt["score"]
    np_ = np.minimum(rng.integers(0, max_pred + 1, S), max_pred)
    P = int(np_.sum())
    ps = np.repeat(np.arange(S), np_)
    goff = np.r_[0, np.cumsum(ng)]
    # 40 % jittered copies of a GT of the sample, the rest clutter
    from_gt = (rng.random(P) < 0.4) & (ng[ps] > 0)
    pick = goff[ps] + (rng.random(P) * np.maximum(ng[ps], 1)).astype(np.int64)
    pick = np.minimum(pick, G - 1)
    pc = np.where(from_gt & (rng.random(P) < 0.9), gc[pick], rng.choice(10, P, p=CLASS_P))
    base = np.where(from_gt[:, None], gt_l[pick], np.concatenate(
        [rng.uniform(-60, 60, (P, 2)), rng.normal(-1, 0.5, (P, 1)), SIZES[pc][:, [1, 0, 2]], rng.uniform(-3, 3, (P, 1)),
         rng.normal(0, 2, (P, 2))], 1))
    jit = np.concatenate([rng.normal(0, 0.8, (P, 2)) * rng.choice([0.3, 1, 3], (P, 1)), rng.normal(0, 0.2, (P, 1)),
                          rng.uniform(0.9, 1.1, (P, 3)), rng.normal(0, 0.3, (P, 1)), rng.normal(0, 0.5, (P, 2))], 1)
    pb = base.copy()
    pb[:, :3] += jit[:, :3]
    pb[:, 3:6] *= jit[:, 3:6]
    pb[:, 6:] += jit[:, 6:]
    pb = pb.astype(np.float32)
    score = np.round(np.where(from_gt, rng.uniform(0.3, 1.0, P), rng.uniform(0.0, 0.6, P)), 2).astype(np.float32)
    return {"gt": gt, "ego": ego, "l2g": l2g, "pred_boxes": pb, "pred_scores": score, "pred_labels": pc + 1,
            "pred_count": np_}


def _batches(data, B):
    off = np.r_[0, np.cumsum(data["pred_count"])]
    S = len(data["pred_count"])
    for s0 in range(0, S, B):
        ids = list(range(s0, min(S, s0 + B)))
        yield ids, [{"pred_boxes": data["pred_boxes"][off[s]:off[s + 1]], "pred_scores": data["pred_scores"][off[s]:off[s + 1]],
                     "pred_labels": data["pred_labels"][off[s]:off[s + 1]]} for s in ids]


def _add_all(ev, data, dev, B=8, order=None):
    for ids, pds in _batches(data, B):
        if order is not None and not order(ids):
            continue
        dpd = [{k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in pd.items()} for pd in pds]
        ev.add_batch(ids, dpd, torch.from_numpy(data["l2g"][ids]).to(dev))


def _oracle_preds(data):
    S = len(data["pred_count"])
    return R.preds_from_arrays(data["pred_boxes"], data["pred_scores"], data["pred_labels"],
                               np.repeat(np.arange(S), data["pred_count"]), data["l2g"])


def test_full_size_synthetic_val(hip_lib):
    dev = torch.device("cuda:0")
    data = synthetic_val()
    assert data["pred_count"].max() <= 500 and len(np.unique(data["pred_scores"])) <= 101
    ref, detail, _ = R.evaluate(data["gt"], _oracle_preds(data), data["ego"])
    ev = _make_eval(data["gt"], data["ego"], dev)
    _add_all(ev, data, dev)
    assert_summary(ev.compute(), ref)
    _check_detail(ev, detail)
    assert 0.0 < ref["mean_ap"] < 1.0 and 0.0 < ref["nd_score"] < 1.0


def test_eval_forward_end_to_end(hip_lib):
    """ValidationStep (eval forward -> add_batch) on synthetic batches for a LiDAR and a camera model, against the
    reference-format prediction dicts fed to the oracle."""
    from unidistill_amd import _lib, evaluation as E, train
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    for modality in ("lidar", "camera"):
        torch.manual_seed(0)
        model = train.build_model(modality).to(dev)
        batch = train.synthetic_batch(dev, 2, with_imgs=modality == "camera", with_points=modality == "lidar")
        l2g = np.stack([np.eye(4)] * 2)
        for s in range(2):
            l2g[s, :3, :3] = _rot(rng.uniform(-3, 3), 0.01)
            l2g[s, :3, 3] = [500.0 + s, 800.0, 1.8]
        gtb = batch["gt_boxes"].cpu().numpy()
        gtl = batch["gt_labels"].cpu().numpy()
        ego = l2g[:, :3, 3].copy()
        gt_rows = [(s, i) for s in range(2) for i in range(gtb.shape[1]) if gtl[s, i] >= 0 and gtb[s, i, 3] > 0]
        gt = R.preds_from_arrays(np.stack([gtb[s, i, :9] for s, i in gt_rows]), np.zeros(len(gt_rows), np.float32),
                                 np.array([gtl[s, i] + 1 for s, i in gt_rows]), np.array([s for s, _ in gt_rows]), l2g)
        gt["num_pts"] = np.ones(len(gt_rows), np.int64)
        del gt["score"]
        ev = _make_eval(gt, ego, dev, cfg=dict(E.DETECTION_CVPR_2019, max_boxes_per_sample=600))
        step = train.ValidationStep(model, ev)
        # the camera model's eval-mode image BatchNorm on NCHW activations has no hand-written kernel: library path allowed
        with _lib.strict(modality == "lidar"):
            pds = step(batch, [0, 1], torch.from_numpy(l2g).to(dev))
        assert model.training                     # the step restores the mode it found
        pred = R.preds_from_dicts(_host(pds), [0, 1], l2g)
        ref, _, _ = R.evaluate(gt, pred, ego)
        assert_summary(ev.compute(), ref)


def test_rejections(hip_lib):
    from unidistill_amd import evaluation as E
    dev = torch.device("cuda:0")
    g, p, S = cases.case_all_fp()
    gt = cases.boxes(g)
    pds = _rows_to_pred_dicts(p, S, dev)
    eye = torch.eye(4, dtype=torch.float64, device=dev).repeat(S, 1, 1)
    ev = _make_eval(gt, cases.ego(S), dev)
    big = {"pred_boxes": torch.zeros((501, 9), device=dev), "pred_scores": torch.zeros(501, device=dev),
           "pred_labels": torch.ones(501, dtype=torch.int64, device=dev)}
    with pytest.raises(ValueError, match="max_boxes_per_sample"):
        ev.add_batch([0], [big], eye[:1])
    ev.add_batch([0], pds[:1], eye[:1])                      # sample 1 never arrives
    with pytest.raises(ValueError, match="not in the predictions"):
        ev.compute()
    ev.reset()
    ev.add_batch([0, 5], pds, eye)
    with pytest.raises(ValueError, match="outside"):
        ev.compute()
    ev.reset()
    bad = [dict(pds[0], pred_labels=pds[0]["pred_labels"] + 10), pds[1]]
    ev.add_batch([0, 1], bad, eye)
    with pytest.raises(ValueError, match="class id"):
        ev.compute()
    ev.reset()                                               # a matched pair with a zero size
    zero = dict(pds[0], pred_boxes=torch.tensor([[0.1, 0.0, 0.5, 4, 0, 1.5, 0, 0, 0]], device=dev))
    g2 = cases.boxes([(0, 0, 0.0, 0.0), (1, 8, 5.0, 5.0)])
    ev2 = _make_eval(g2, cases.ego(S), dev)
    ev2.add_batch([0, 1], [zero, pds[1]], eye)
    with pytest.raises(ValueError, match="size"):
        ev2.compute()
    with pytest.raises(RuntimeError, match="GPU only"):
        ev.add_batch([0, 1], [{k: v.cpu() for k, v in pd.items()} for pd in pds], eye)
    with pytest.raises(ValueError, match="float64"):
        ev.add_batch([0, 1], pds, eye.float())
    with pytest.raises(ValueError, match="ground-truth class"):
        ev.add_ground_truth(gt["translation"], gt["size"], gt["yaw"], gt["velocity"], gt["cls"] + 20, gt["attr"],
                            gt["num_pts"], gt["sample"], cases.ego(S))
    assert E.NuScenesDetectionEval(device=dev).gt is None


def test_submission_json(hip_lib, tmp_path):
    dev = torch.device("cuda:0")
    data = synthetic_val(S=12, seed=4, max_pred=60)
    ev = _make_eval(data["gt"], data["ego"], dev)
    _add_all(ev, data, dev, B=5)
    tokens = [f"tok{s:03d}" for s in range(12)]
    path = tmp_path / "results_nusc.json"
    with pytest.raises(RuntimeError, match="compute"):
        ev.write_submission(str(path), tokens)            # it writes what compute() evaluated
    ev.compute()
    ev.write_submission(str(path), tokens)
    check_submission(json.loads(path.read_text()), data, tokens)
    ev.reset()
    with pytest.raises(RuntimeError, match="compute"):
        ev.write_submission(str(path), tokens)


def check_submission(sub, data, tokens):
    """The results JSON against the oracle's conversion of the same predictions."""
    assert sub["meta"] == {"use_camera": True, "use_lidar": True, "use_radar": False, "use_map": False,
                           "use_external": False}
    ref = _oracle_preds(data)
    assert list(sub["results"]) == list(tokens)
    k = 0
    for s, tok in enumerate(tokens):
        for box in sub["results"][tok]:
            assert box["sample_token"] == tok
            np.testing.assert_allclose(box["translation"], ref["translation"][k], rtol=0, atol=1e-9)
            assert box["size"] == ref["size"][k].tolist()
            np.testing.assert_allclose(box["velocity"], ref["velocity"][k], rtol=0, atol=1e-12)
            q = box["rotation"]
            assert abs(math.remainder(2 * math.atan2(q[3], q[0]) - ref["yaw"][k], 2 * math.pi)) < 1e-12
            assert box["detection_name"] == R.CLASS_NAMES[ref["cls"][k]]
            assert box["detection_score"] == ref["score"][k]
            assert box["attribute_name"] == (R.ATTRIBUTE_NAMES[ref["attr"][k]] if ref["attr"][k] >= 0 else "")
            k += 1
    assert k == len(ref["cls"])


_TWO_RANKS = r'''
import datetime, os, sys, json, numpy as np, torch, torch.distributed as dist
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=60))   # an unpaired collective fails, not hangs
import test_nus_eval_gpu as T
dev = torch.device("cuda", 0)
data = T.synthetic_val(S=40, seed=7, max_pred=120)
ev = T._make_eval(data["gt"], data["ego"], dev)
# rank r takes the batches with (first id // 4) % 2 == r; both take batch 0 again, as DistributedSampler padding would
T._add_all(ev, data, dev, B=4, order=lambda ids: (ids[0] // 4) % world == rank or ids[0] == 0)
got = ev.compute()
tokens = ["tok%03d" % s for s in range(40)]
if rank == 0:
    ref, _, _ = T.R.evaluate(data["gt"], T._oracle_preds(data), data["ego"])
    T.assert_summary(got, ref)
    # rank 0 alone, as in INTEGRATION: no collective may run inside, or the barrier below pairs with it
    sub = ev.write_submission({json_path!r}, tokens)
    T.check_submission(json.load(open({json_path!r})), data, tokens)
else:
    assert got is None
    assert ev.write_submission({json_path!r} + ".rank1", tokens) is None
    assert not os.path.exists({json_path!r} + ".rank1")
dist.barrier()
flag = torch.tensor([rank + 1])
dist.all_reduce(flag)                                    # the next collective after the epoch still pairs up
assert int(flag) == 3
ev.reset()
if rank == 0:
    print("TWO_RANKS_OK", json.dumps(got["nd_score"]))
dist.destroy_process_group()
'''


def test_two_ranks_gather_to_rank0(hip_lib, tmp_path):
    script = tmp_path / "two_ranks.py"
    script.write_text(_TWO_RANKS.format(root=ROOT, pkg=os.path.join(ROOT, "cvpr2023-unidistill_amd"),
                                        tests=os.path.join(ROOT, "tests"), json_path=str(tmp_path / "results.json")))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29557", str(script)]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "TWO_RANKS_OK" in res.stdout
