"""GPU: ops.det_loss.rotated_iou3d (csrc/rot_iou3d.h, ud_rot_iou3d_pairs) against the float64 restatement of tests/rot_iou_reference.py.

The yardstick for "close enough" is what single precision costs the restatement itself: its float32 evaluation on the CPU is compared
with its float64 one on the very same (float32-representable) inputs, and the kernel may deviate by 4x that maximum (the factor covers
a different order of operations), never less than 1e-6.  Derivatives are compared on the pairs at least rot_iou_reference.MARGIN away
from every decision (tests/test_rot_iou_cpu.py caps how many the draw may lose)."""
import functools
import math

import pytest
import torch

import rot_iou_reference as R

pytestmark = pytest.mark.gpu
N = 256


@functools.lru_cache(maxsize=None)
def _reference():
    a, b = R.random_pairs(N)
    a, b = a.float(), b.float()
    iou64, grad64, margin = R.iou3d_and_grad(a.double(), b.double(), torch.float64)
    iou32, grad32, _ = R.iou3d_and_grad(a, b, torch.float32)
    ok = margin >= R.MARGIN
    tol_v = max(4 * float((iou32 - iou64).abs().max()), 1e-6)
    tol_g = max(4 * float((grad32 - grad64)[ok].abs().max()), 1e-6)
    print(f"float32 restatement against float64: value {float((iou32 - iou64).abs().max()):.3e}, derivative "
          f"{float((grad32 - grad64)[ok].abs().max()):.3e} on {int(ok.sum())} of {N} pairs")
    return a, b, iou64, grad64, ok, tol_v, tol_g


def _run(a, b, grad=True):
    from unidistill_amd.ops import det_loss
    x = a.cuda().requires_grad_(grad)
    iou = det_loss.rotated_iou3d(x, b.cuda())
    if not grad:
        return iou.cpu()
    g, = torch.autograd.grad(iou.sum(), x)
    return iou.detach().cpu(), g.cpu()


def test_values_and_derivatives_match_float64(hip_lib):
    a, b, iou64, grad64, ok, tol_v, tol_g = _reference()
    iou, grad = _run(a, b)
    dev_v = float((iou.double() - iou64).abs().max())
    dev_g = float((grad.double() - grad64)[ok].abs().max())
    print(f"value: kernel {dev_v:.3e} allowed {tol_v:.3e} | derivative: kernel {dev_g:.3e} allowed {tol_g:.3e} "
          f"on {int(ok.sum())} of {N} pairs")
    assert dev_v <= tol_v
    assert dev_g <= tol_g
    assert torch.isfinite(grad).all()
    # the value does not depend on whether the derivative is asked for, and a second run is bitwise the same
    assert torch.equal(_run(a, b, grad=False), iou)
    iou2, grad2 = _run(a, b)
    assert torch.equal(iou2, iou) and torch.equal(grad2, grad)


def test_upstream_gradient_scales_the_rows(hip_lib):
    from unidistill_amd.ops import det_loss
    a, b, _, grad64, ok, _, tol_g = _reference()
    w = torch.linspace(-2, 2, N)
    x = a.cuda().requires_grad_(True)
    (det_loss.rotated_iou3d(x, b.cuda()) * w.cuda()).sum().backward()
    assert float((x.grad.cpu().double() - grad64 * w[:, None].double())[ok].abs().max()) <= 2 * tol_g


def test_closed_forms(hip_lib):
    r2 = math.sqrt(2.0)
    box = [3.0, -2.0, 0.5, 4.0, 1.5, 2.0, 0.7]
    sq = [3.0, -2.0, 0.5, 2.5, 2.5, 2.0, 0.7]
    a = torch.tensor([[1, 2, 0, 1, 1, 3, math.pi / 4], box, box[:6] + [0.7 + math.pi], sq[:6] + [0.7 + math.pi / 2],
                      [0, 0, 0, 2, 2, 2, 0], [0, 0, 0, 2, 2, 1, 0.3], [0, 0, 0, 1, 1, 1, 0], [0, 0, 0, 2, 3, 4, 0]])
    b = torch.tensor([[1, 2, 0, r2, r2, 3, 0], box, box, sq,
                      [2, 0, 0, 2, 2, 2, 0], [0.5, 0, 1.5, 2, 2, 1, 0.1], [0.5, 0, 0, 1, 1, 1, 0], [1, 1, 1, 2, 3, 4, 0]])
    want = torch.tensor([0.5, 1.0, 1.0, 1.0, 0.0, 0.0, 1 / 3, 1 * 2 * 3 / (48 - 6)])
    iou, grad = _run(a, b)
    # a handful of float32 roundings of O(1) quantities
    torch.testing.assert_close(iou, want, rtol=0, atol=2e-6)
    assert float(iou[4]) == 0.0 and float(iou[5]) == 0.0
    assert torch.isfinite(grad).all()


def test_degenerate_pairs(hip_lib):
    nan = float("nan")
    a = torch.tensor([[0, 0, 0, 2, 1, 1, 0.3],                  # identical boxes
                      [0, 0, 0, 1e-3, 1e-3, 1e-3, 0],           # the clamped 1e-3 extents: union 1e-9 below the 1e-8 floor
                      [0, 0, 0, 2, 1, 1, 0.0],                  # heading atan2(0, 0) = 0
                      [0, 0, 0, 2, 1, 1, 0.3],                  # NaN target row
                      [nan, 0, 0, 2, 1, 1, 0.3],                # NaN in the prediction
                      [0, 0, 0, 2, 1, nan, 0.3],
                      [40, 40, 0, 2, 1, 1, 0.3]])               # far apart
    b = torch.tensor([[0, 0, 0, 2, 1, 1, 0.3],
                      [0, 0, 0, 1e-3, 1e-3, 1e-3, 0],
                      [0.5, 0, 0, 2, 1, 1, 0.0],
                      [nan] * 7,
                      [0, 0, 0, 2, 1, 1, 0.3],
                      [0, 0, 0, 2, 1, 1, 0.3],
                      [0, 0, 0, 2, 1, 1, 0.3]])
    iou, grad = _run(a, b)
    assert abs(float(iou[0]) - 1.0) <= 1e-6
    assert abs(float(iou[1]) - 0.1) <= 1e-6                     # 1e-9 / max(1e-9, 1e-8)
    assert abs(float(iou[2]) - 1.5 / 2.5) <= 1e-6
    assert torch.isnan(iou[3:6]).all()                          # a NaN flows through to the value ...
    assert float(iou[6]) == 0.0
    assert torch.isfinite(grad).all()                           # ... and its derivative is reported as 0
    assert float(grad[3:7].abs().max()) == 0.0


def test_argument_checks(hip_lib):
    from unidistill_amd.ops import det_loss
    a = torch.zeros(4, 7, device="cuda")
    with pytest.raises(RuntimeError, match="GPU only"):
        det_loss.rotated_iou3d(a, torch.zeros(4, 7))
    with pytest.raises(TypeError):
        det_loss.rotated_iou3d(a.double(), a.double())
    with pytest.raises(ValueError):
        det_loss.rotated_iou3d(a, a[:3])
    assert det_loss.rotated_iou3d(a[:0], a[:0]).shape == (0,)


def test_shim_binds_the_pairwise_op(hip_lib):
    """The stand-in for the reference's missing iou3d_nms_cuda extension carries the op as boxes_iou3d_pairs."""
    import sys
    from unidistill_amd import shims
    before = dict(sys.modules)
    try:
        shims.install()
        stub = sys.modules["unidistill.layers.head.det3d.generate_proposals.iou3d_nms_cuda"]
        box = torch.tensor([[0, 0, 0, 1, 1, 1, 0.0]], device="cuda")
        assert abs(float(stub.boxes_iou3d_pairs(box, box)) - 1.0) <= 1e-6
    finally:                                # leave no stub modules behind for the tests that follow
        for k in list(sys.modules):
            if k not in before:
                del sys.modules[k]
