"""CPU: the depth metric's host side.  The float64 restatement the GPU tests compare against (tests/depth_metric_ref.py) against
a hand expansion; evaluation.DepthMetric.compute() from hand-filled states, alone and over two gloo ranks; and
train.ValidationStep's new keyword, whose default must leave the step as it was."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import depth_metric_ref as R
from unidistill_amd import evaluation, train
from unidistill_amd.ops import depth_metric as op

KEYS = ("n", "abs_rel", "sq_rel", "rmse", "rmse_log", "mae", "d1", "d2", "d3", "bin_acc", "bin_acc1", "nll")


def test_op_refuses_cpu_tensors():
    state = torch.zeros(1, 1, 12, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU only"):
        op.depth_metric_accumulate(torch.zeros(1, 3, 2, 2), torch.zeros(1, 2, 2), state, [2.0, 5.0, 1.0], [2.0, 5.0])
    assert float(state.abs().max()) == 0.0
    assert op.depth_bins([2.0, 58.0, 0.5]) == (2.0, 0.5, 112) and len(op.TERMS) == R.T == 12


def test_restatement_matches_hand_expansion():
    """D = 3 bins [2, 3), [3, 4), [4, 5) with centres 2.5, 3.5, 4.5.  Pixel 0: logits (0.3, -1.2, 2.0), d = 3.25 (bin 1).
    Pixel 1: logits (1, 1, -0.5), a tie that goes to bin 0, d = 4.75 (bin 2).  Pixel 2 has no return, pixel 3 lies beyond the
    last bin.  Ranges [2, 4), [4, 5): one pixel each."""
    x = np.array([[0.3, -1.2, 2.0], [1.0, 1.0, -0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]).T.reshape(1, 3, 1, 4)
    dmin = np.array([3.25, 4.75, np.inf, 5.0], np.float32).reshape(1, 1, 4)
    state = R.depth_metric_state(x, dmin, 2.0, 1.0, [2.0, 4.0, 5.0], 1)
    assert state.shape == (1, 2, 12)

    def hand(logits, d, b):
        ex = [math.exp(v - max(logits)) for v in logits]
        p = [v / sum(ex) for v in ex]
        dhat = p[0] * 2.5 + p[1] * 3.5 + p[2] * 4.5
        e = dhat - d
        q = max(dhat / d, d / dhat)
        a = logits.index(max(logits))
        return [1.0, abs(e), abs(e) / d, e * e / d, e * e, (math.log(dhat) - math.log(d)) ** 2, float(q < 1.25),
                float(q < 1.5625), float(q < 1.953125), float(a == b), float(abs(a - b) <= 1), -math.log(p[b])]
    want0, want1 = hand([0.3, -1.2, 2.0], 3.25, 1), hand([1.0, 1.0, -0.5], 4.75, 2)
    # pixel 0: dhat = 4.13..., q = 1.27: outside 1.25, inside 1.25^2; arg-max 2, one off the label.  pixel 1: dhat = 3.09...,
    # q = 1.53; arg-max 0 by the tie rule, two off
    assert want0[6:11] == [0.0, 1.0, 1.0, 0.0, 1.0] and want1[6:11] == [0.0, 1.0, 1.0, 0.0, 0.0]
    np.testing.assert_allclose(state[0, 0], want0, rtol=1e-14, atol=0)
    np.testing.assert_allclose(state[0, 1], want1, rtol=1e-14, atol=0)
    # two groups: image n goes to group n mod 2; a pixel outside every bucket is counted nowhere
    x2 = np.concatenate([x, x, x], 0)
    d2 = np.concatenate([dmin, dmin, dmin], 0)
    s2 = R.depth_metric_state(x2, d2, 2.0, 1.0, [2.0, 4.0], 2)
    np.testing.assert_allclose(s2[0, 0], 2 * np.array(want0), rtol=1e-14)
    np.testing.assert_allclose(s2[1, 0], want0, rtol=1e-14)
    # the plain-PyTorch float32 evaluation of the same expression agrees to float32 accuracy
    s32 = R.torch_fp32_state(torch.from_numpy(x2), torch.from_numpy(d2), 2.0, 1.0, [2.0, 4.0, 5.0], 2)
    np.testing.assert_allclose(s32, R.depth_metric_state(x2, d2, 2.0, 1.0, [2.0, 4.0, 5.0], 2), rtol=1e-5, atol=1e-6)


def _filled_state(rank):
    """[2 cameras, 3 ranges, 12]: range 1 of camera 0 and all of range 2 are empty."""
    g = np.random.default_rng(40 + rank)
    s = np.zeros((2, 3, 12))
    for cam, r, n in ((0, 0, 7 + rank), (1, 0, 5), (1, 1, 11 + 2 * rank)):
        s[cam, r] = g.uniform(0.5, 4.0, 12) * n
        s[cam, r, 0] = n
        s[cam, r, 6:11] = g.integers(0, n + 1, 5)
    return s


def _want(t):
    n = t[0]
    return {"n": int(n), "abs_rel": t[2] / n, "sq_rel": t[3] / n, "rmse": math.sqrt(t[4] / n), "rmse_log": math.sqrt(t[5] / n),
            "mae": t[1] / n, "d1": t[6] / n, "d2": t[7] / n, "d3": t[8] / n, "bin_acc": t[9] / n, "bin_acc1": t[10] / n,
            "nll": t[11] / n}


def _check_figures(out, s):
    assert set(KEYS) <= set(out)
    for got, t in [(out, s.sum((0, 1)))] + [(out["ranges"][r], s[:, r].sum(0)) for r in range(2)] + \
                  [(out["cameras"][c], s[c].sum(0)) for c in range(2)]:
        want = _want(t)
        assert got["n"] == want["n"]
        for k in KEYS[1:]:
            assert abs(got[k] - want[k]) <= 1e-15 * abs(want[k]), k
    empty = out["ranges"][2]
    assert empty["n"] == 0 and all(math.isnan(empty[k]) for k in KEYS[1:])
    assert [(r["lo"], r["hi"]) for r in out["ranges"]] == [(2.0, 20.0), (20.0, 40.0), (40.0, 58.0)]


def test_compute_from_a_hand_filled_state():
    m = evaluation.DepthMetric([2.0, 58.0, 0.5], ncam=2, range_edges=[2.0, 20.0, 40.0, 58.0], per_camera=True, device="cpu")
    assert tuple(m.state.shape) == (2, 3, 12) and m.state.dtype == torch.float64 and float(m.state.abs().max()) == 0.0
    s = _filled_state(0)
    m.state.copy_(torch.from_numpy(s))
    out = m.compute()
    _check_figures(out, s)
    # overall is formed from the summed terms: with 12 and 5 + 11 pixels it is not the mean of the buckets' figures
    assert abs(out["abs_rel"] - np.mean([r["abs_rel"] for r in out["ranges"][:2]])) > 1e-6
    assert torch.equal(m.state, torch.from_numpy(s))                     # compute() leaves the state alone
    m.reset()
    out = m.compute()
    assert out["n"] == 0 and math.isnan(out["rmse"]) and float(m.state.abs().max()) == 0.0
    # the default: one bucket over the bins, no breakdown
    m1 = evaluation.DepthMetric([2.0, 58.0, 0.5], ncam=6, device="cpu")
    assert tuple(m1.state.shape) == (1, 1, 12) and m1.range_edges == [2.0, 58.0]
    assert "ranges" not in m1.compute() and "cameras" not in m1.compute()
    with pytest.raises(RuntimeError, match="GPU only"):                  # the accumulation itself has no CPU path
        m1.add_batch(torch.zeros(6, 112, 2, 2), torch.zeros(1, 6, 2, 2))
    for bad in ([2.0], [2.0, 2.0], [3.0, 2.0], list(range(10))):
        with pytest.raises(ValueError):
            evaluation.DepthMetric([2.0, 58.0, 0.5], range_edges=bad, device="cpu")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = evaluation.DepthMetric([2.0, 58.0, 0.5], ncam=2, range_edges=[2.0, 20.0, 40.0, 58.0], per_camera=True, device="cpu")
    m.state.copy_(torch.from_numpy(_filled_state(rank)))
    out[rank] = m.compute()
    out[f"state{rank}"] = m.state.clone()
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_reduce_sums_the_states():
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    total = _filled_state(0) + _filled_state(1)
    for rank in range(2):
        _check_figures(out[rank], total)                                 # every rank gets the figures of the sum
        assert torch.equal(out[f"state{rank}"], torch.from_numpy(_filled_state(rank)))   # its own state is not overwritten


class _StubBackbone:
    def __init__(self):
        self.calls = 0

    def lidar_depth_labels(self, points, mats_dict):
        self.calls += 1
        raise AssertionError("the default ValidationStep must not build depth labels")


class _StubEncoder:
    def __init__(self):
        self.backbone = _StubBackbone()


class _StubModel(torch.nn.Module):
    def __init__(self, camera=True):
        super().__init__()
        self.camera_encoder = _StubEncoder() if camera else None
        self.seen = []

    def forward(self, *args, **kwargs):
        self.seen.append((args, kwargs))
        return {"pred_dicts": [{"pred_boxes": torch.zeros(0, 9)}]}


class _StubEvaluator:
    def __init__(self):
        self.batches = []

    def add_batch(self, *a):
        self.batches.append(a)


def test_validation_step_default_path_is_unchanged():
    model, ev = _StubModel(), _StubEvaluator()
    step = train.ValidationStep(model, ev, weights=None, depth_metric=None)
    assert step.depth_metric is None
    batch = {"points": torch.zeros(1, 4, 5), "imgs": torch.zeros(1), "mats_dict": {"x": 1}}
    model.train()
    preds = step(batch, [3], None)
    (args, kwargs), = model.seen
    assert kwargs == {} and len(args) == 4 and args[3] is None and args[2] == {"x": 1}      # today's call, no new keyword
    assert isinstance(args[0], list) and len(args[0]) == 1
    assert model.camera_encoder.backbone.calls == 0 and model.training
    assert preds is ev.batches[0][1] and ev.batches[0][0] == [3]
    assert train.ValidationStep(model, ev).depth_metric is None                              # the keyword defaults to None


def test_validation_step_with_metric_needs_camera_and_points():
    m = evaluation.DepthMetric([2.0, 58.0, 0.5], device="cpu")
    batch = {"points": torch.zeros(1, 4, 5), "imgs": torch.zeros(1), "mats_dict": {"x": 1}}
    lidar_only = _StubModel(camera=False)
    with pytest.raises(ValueError, match="camera encoder"):
        train.ValidationStep(lidar_only, _StubEvaluator(), depth_metric=m)(batch, [0], None)
    model = _StubModel()
    for missing in ("points", "mats_dict"):
        with pytest.raises(ValueError, match="points"):
            train.ValidationStep(model, _StubEvaluator(), depth_metric=m)({k: v for k, v in batch.items() if k != missing},
                                                                          [0], None)
    assert lidar_only.seen == [] and model.seen == []                                        # refused before any forward
