"""CPU: the float64 yardstick of the rotated 3-D IoU (tests/rot_iou_reference.py) is itself pinned -- closed forms, autograd against
central differences -- and the random draw the GPU tests share is checked for how many of its pairs sit next to a decision."""
import math

import pytest
import torch

import rot_iou_reference as R

F64 = torch.float64
N_RANDOM = 256


def _boxes(rows):
    return torch.tensor(rows, dtype=F64)


def _iou(a, b):
    return R.iou3d_pairs(_boxes(a), _boxes(b))[0]


def test_axis_aligned_pairs_equal_the_product_formula():
    g = torch.Generator().manual_seed(3)
    a = torch.cat([torch.rand(32, 3, generator=g, dtype=F64) * 4 - 2, torch.rand(32, 3, generator=g, dtype=F64) * 4 + 0.5,
                   torch.zeros(32, 1, dtype=F64)], 1)
    b = torch.cat([torch.rand(32, 3, generator=g, dtype=F64) * 4 - 2, torch.rand(32, 3, generator=g, dtype=F64) * 4 + 0.5,
                   torch.zeros(32, 1, dtype=F64)], 1)
    ov = torch.clamp(torch.minimum(a[:, :3] + a[:, 3:6] / 2, b[:, :3] + b[:, 3:6] / 2)
                     - torch.maximum(a[:, :3] - a[:, 3:6] / 2, b[:, :3] - b[:, 3:6] / 2), min=0).prod(1)
    want = ov / (a[:, 3:6].prod(1) + b[:, 3:6].prod(1) - ov)
    assert (want > 0).sum() >= 16
    torch.testing.assert_close(R.iou3d_pairs(a, b)[0], want, rtol=0, atol=1e-13)


def test_closed_forms():
    r2 = math.sqrt(2.0)
    # a unit square turned by 45 degrees fits exactly into a sqrt(2) square: inter = 1, union = 2
    torch.testing.assert_close(_iou([[1, 2, 0, 1, 1, 3, math.pi / 4]], [[1, 2, 0, r2, r2, 3, 0]]), _boxes([0.5]), rtol=0, atol=1e-12)
    box = [3.0, -2.0, 0.5, 4.0, 1.5, 2.0, 0.7]
    same = _iou([box, box[:6] + [0.7 + math.pi]], [box, box])                      # itself, and turned by half a turn
    torch.testing.assert_close(same, _boxes([1.0, 1.0]), rtol=0, atol=1e-12)
    sq = [3.0, -2.0, 0.5, 2.5, 2.5, 2.0, 0.7]
    torch.testing.assert_close(_iou([sq[:6] + [0.7 + math.pi / 2]], [sq]), _boxes([1.0]), rtol=0, atol=1e-12)
    # touching along an edge (binary-exact coordinates), and overlapping in BEV with disjoint z
    assert float(_iou([[0, 0, 0, 2, 2, 2, 0]], [[2, 0, 0, 2, 2, 2, 0]])) == 0.0
    assert float(_iou([[0, 0, 0, 2, 2, 1, 0.3]], [[0.5, 0, 1.5, 2, 2, 1, 0.1]])) == 0.0
    # half-overlapping unit cubes: 0.5 / 1.5
    torch.testing.assert_close(_iou([[0, 0, 0, 1, 1, 1, 0]], [[0.5, 0, 0, 1, 1, 1, 0]]), _boxes([1 / 3]), rtol=0, atol=1e-13)


def test_margin_reports_the_nearest_decision():
    # the corner (1, y) of a is 0.25 inside b's edge x = 1.25 and nothing else is closer: margin 0.25
    _, m = R.iou3d_pairs(_boxes([[0, 0, 0, 2, 2, 2, 0]]), _boxes([[0.75, 1.5, 0.5, 1, 4, 4, 0]]))
    assert abs(float(m) - 0.25) < 1e-12
    _, m = R.iou3d_pairs(_boxes([[0, 0, 0, 2, 2, 2, 0]]), _boxes([[2, 0, 0, 2, 2, 2, 0]]))      # touching: on the decision
    assert float(m) == 0.0


@pytest.fixture(scope="module")
def drawn():
    a, b = R.random_pairs(N_RANDOM)
    a, b = a.float().double(), b.float().double()          # what the GPU tests feed the kernel
    iou, grad, margin = R.iou3d_and_grad(a, b, F64)
    return a, b, iou, grad, margin


def test_random_draw_keeps_at_least_nine_pairs_in_ten(drawn):
    a, b, iou, grad, margin = drawn
    rejected = int((margin < R.MARGIN).sum())
    print(f"rejected {rejected} of {N_RANDOM} pairs (margin < {R.MARGIN}); {int((iou > 0).sum())} pairs overlap")
    assert rejected <= N_RANDOM // 10
    assert int((iou > 0.05).sum()) >= N_RANDOM // 2           # the draw is about overlapping boxes
    assert bool((iou >= 0).all()) and bool((iou <= 1).all())


def test_autograd_matches_central_differences(drawn):
    a, b, iou, grad, margin = drawn
    pick = torch.nonzero(margin >= R.MARGIN)[::4, 0]          # every fourth accepted pair: 14 evaluations each
    assert pick.numel() >= 56
    h = 1e-6
    a, b, grad = a[pick], b[pick], grad[pick]
    with torch.no_grad():
        for j in range(7):
            step = torch.zeros(7, dtype=F64)
            step[j] = h
            fd = (R.iou3d_pairs(a + step, b)[0] - R.iou3d_pairs(a - step, b)[0]) / (2 * h)
            # second-order error h^2 f''' ~ 1e-12, rounding 1e-16 / h = 1e-10
            torch.testing.assert_close(grad[:, j], fd, rtol=0, atol=2e-9, msg=lambda m: f"d/d box[{j}]: {m}")


def test_reg_terms_restatement_on_a_hand_expanded_slot():
    """One positive slot: the composition with the head decode gives the numbers worked out by hand."""
    sx, sy = 0.5, 0.25
    # prediction: unit cube at the anchor, heading from a non-unit (sin, cos); target: the same cube moved by 0.5 m in x
    g = torch.zeros(1, 1, 1, 11, dtype=F64)
    g[..., 6], g[..., 7], g[..., 10] = 0.0, 1.7, 0.25
    tgt = torch.zeros(1, 1, 1, 10, dtype=F64)
    tgt[..., 0], tgt[..., 7] = 0.5 / sx, 1.0
    mask = torch.ones(1, 1, 1, dtype=torch.bool)
    box, iou_loss, aware, margin = R.reg_terms_ref(g.requires_grad_(True), tgt, mask, torch.tensor([1.0], dtype=F64), sx, sy, 10)
    torch.testing.assert_close(iou_loss, _boxes([1 - 1 / 3]), rtol=0, atol=1e-13)
    torch.testing.assert_close(aware, _boxes([abs(0.25 - 2 * (1 / 3 - 0.5)) / 1.0001]), rtol=0, atol=1e-13)
    torch.testing.assert_close(box[0, 0], _boxes([1.0 / 1.0001])[0], rtol=0, atol=1e-13)
    torch.testing.assert_close(box[0, 7], _boxes([0.7 / 1.0001])[0], rtol=0, atol=1e-13)
    iou_loss.sum().backward()
    # inter = 1 - (0.5 - x), union = 1 + (0.5 - x): d IoU / d x = 2 / (1.5)^2, times sx for the head value
    torch.testing.assert_close(g.grad[0, 0, 0, 0], _boxes([-(2 / 2.25) * sx])[0], rtol=0, atol=1e-12)
    assert float(g.grad[0, 0, 0, 10]) == 0.0                 # the IoU-aware target is detached


def test_pairwise_op_and_modes_refuse_the_cpu(hip_lib):
    from unidistill_amd.ops import det_loss
    for name in ("ud_det_reg_fwd_rot", "ud_det_reg_bwd_rot", "ud_rot_iou3d_pairs"):
        assert hasattr(hip_lib, name)
    with pytest.raises(RuntimeError, match="GPU only"):
        det_loss.rotated_iou3d(torch.zeros(2, 7), torch.zeros(2, 7))
    with pytest.raises(ValueError, match="iou_mode"):
        det_loss.check_iou_mode("aligned")
    assert det_loss.IOU_MODES == ("reference", "rotated3d")
