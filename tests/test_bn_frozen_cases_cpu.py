"""CPU half of tests/test_bn_frozen_gpu.py: every seeded case keeps its float64 pre-activations (on the running statistics) at
least bn_reference.MARGIN away from the ReLU threshold, and the float64 restatement used there agrees with torch's eval-mode
BatchNorm under autograd in float64."""
import torch
import torch.nn.functional as F

import bn_reference as R
import test_bn_frozen_gpu as T


def test_every_case_is_off_the_relu_threshold():
    n = 0
    for shape, dtype, residual, relu in T.cases():
        case = T.draw(shape, dtype, residual, relu)
        assert case["x"].dtype == dtype and tuple(case["x"].shape) == T._pc(shape)
        if relu:
            assert case["zmin"] >= R.MARGIN, (shape, dtype, residual, case["zmin"])
            n += 1
    assert n == len(T.SHAPES) * 2 * 2


def test_the_float64_restatement_equals_torch_eval_batchnorm():
    for shape in [(2, 64, 9, 13), (5, 48), (1, 16, 1, 1)]:
        for residual, relu in T.VARIANTS:
            case = T.draw(shape, torch.float32, residual, relu)
            ref = T.reference(case, relu)
            x = case["x"].double().requires_grad_(True)
            g = case["gamma"].double().requires_grad_(True)
            b = case["beta"].double().requires_grad_(True)
            r = case["r"].double().requires_grad_(True) if residual else None
            y = F.batch_norm(x, case["rm"].double(), case["rv"].double(), g, b, False, 0.0, T.EPS)
            y = y + r if residual else y
            y = F.relu(y) if relu else y
            y.backward(case["dy"].double())
            pairs = [(y, ref["y"]), (x.grad, ref["dx"]), (g.grad, ref["dgamma"]), (b.grad, ref["dbeta"])]
            if residual:
                pairs.append((r.grad, ref["dres"]))
            for got, want in pairs:
                assert torch.allclose(got.detach(), want, rtol=1e-12, atol=1e-12)
