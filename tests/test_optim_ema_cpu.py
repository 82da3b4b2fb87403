"""CPU: the float64 EMA reference (tests/ema_reference.py) agrees with torch's AveragedModel and with the closed form of
the recurrence, skipped steps and gradient-less tensors included; the EMA arguments are validated; the new entry points are
declared, exported and reject bad arguments without a GPU."""
import math

import numpy as np
import pytest
import torch

from ema_reference import ClipAdamWEmaReference, EmaReference

EMA_SYMBOLS = ("ud_optim_clip_adamw_ema", "ud_optim_swap")


def test_argument_validation():
    """ValueError before anything touches a device (the parameters here are CPU tensors)."""
    from unidistill_amd.ops.optim import ClipAdamW
    p = [torch.zeros(4, requires_grad=True)]
    for decay in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            ClipAdamW(p, lr=1e-3, ema_decay=decay)
    for ramp in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="ema_ramp"):
            ClipAdamW(p, lr=1e-3, ema_decay=0.9, ema_ramp=ramp)
    with pytest.raises(ValueError, match="ema_ramp needs ema_decay"):
        ClipAdamW(p, lr=1e-3, ema_ramp=4.0)
    with pytest.raises(RuntimeError, match="GPU only"):           # valid EMA arguments: the usual refusal of CPU tensors
        ClipAdamW(p, lr=1e-3, ema_decay=0.9, ema_ramp=4.0)


def test_trainer_refuses_an_ema_without_the_hip_optimizer():
    from unidistill_amd import train
    lin = lambda: train.DetectStep(model=torch.nn.Linear(4, 4))
    with pytest.raises(ValueError, match="optimizer='hip'"):
        train.Trainer(lin(), device=torch.device("cpu"), optimizer="torch", ema_decay=0.9)
    with pytest.raises(ValueError, match="optimizer='hip'"):
        train.Trainer(lin(), device=torch.device("cpu"), optimizer="torch", ema_ramp=4.0)


def test_reference_agrees_with_averaged_model_in_float64():
    """Constant mode against AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay)) around clip_grad_norm_ + AdamW in float64
    on the CPU, 6 steps, to 1e-12 relative.  The average starts from the initial weights (the first update_parameters call
    of an AveragedModel copies); one tensor never gets a gradient."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    rng = np.random.default_rng(0)
    shapes = [(1,), (5,), (7, 9), (16, 8, 3, 3), (1000,), (11,)]
    n_live = len(shapes) - 1
    lr, betas, eps, wd, max_norm = 2e-4, (0.9, 0.999), 1e-8, 1e-7, 0.1
    for decay in (0.999, 0.9):
        init = [rng.standard_normal(s) for s in shapes]
        model = torch.nn.ParameterList([torch.nn.Parameter(torch.tensor(a, dtype=torch.float64)) for a in init])
        params = list(model)
        avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))
        avg.update_parameters(model)                 # n_averaged 0 -> 1: a copy of the initial weights
        opt = torch.optim.AdamW(params, lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=True)
        ref = ClipAdamWEmaReference(init, lr, betas, eps, wd, max_norm, ema_decay=decay)
        for norm in (0.5, 0.03, 2.0, 0.05, 0.2, 0.08):
            grads = [rng.standard_normal(s) for s in shapes[:n_live]]
            scale = norm / np.sqrt(sum((g * g).sum() for g in grads))
            grads = [g * scale for g in grads]
            for p, g in zip(params, grads):
                p.grad = torch.tensor(g, dtype=torch.float64)
            torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=True)
            opt.step()
            avg.update_parameters(model)
            ref.step(grads + [None])
            for got, want in zip(avg.module.parameters(), ref.ema.e):
                assert np.abs(got.detach().numpy() - want).max() <= 1e-12 * np.abs(want).max()
        assert ref.ema.n == 6
        assert np.array_equal(ref.p[-1], init[-1])                       # the gradient-less tensor never moved,
        assert np.abs(ref.ema.e[-1] - init[-1]).max() <= 1e-15           # so its average stayed on it
        assert np.abs(ref.ema.e[0] - ref.p[0]).max() > 0.0               # while a stepped tensor's average lags


def test_reference_closed_form_constant_and_ramp():
    """A constant target c and a start e0: e_n = c + (e0 - c) * prod_k (1 - w_k)."""
    c, e0 = np.array([2.0, -1.0, 0.5]), np.array([0.0, 3.0, 0.5])
    for decay, ramp in ((0.9, None), (0.999, None), (0.9, 4.0), (0.999, 4.0), (0.5, 0.25)):
        ref = EmaReference([e0], decay, ramp)
        keep = 1.0
        for n in range(1, 8):
            ref.update([c])
            d = decay if ramp is None else decay * (1.0 - math.exp(-n / ramp))
            assert ref.weight(n) == 1.0 - d
            keep *= d
            assert np.abs(ref.e[0] - (c + (e0 - c) * keep)).max() <= 1e-14
        assert ref.n == 7
    # the ramp starts near "copy the weights" and ends at the constant decay
    ramped = EmaReference([e0], 0.999, 4.0)
    assert ramped.weight(1) > 0.75 and abs(ramped.weight(10 ** 6) - 0.001) < 1e-12
    assert all(ramped.weight(n) > ramped.weight(n + 1) for n in range(1, 40))


def test_reference_skipped_steps_do_not_advance_the_ramp():
    """Steps 2 and 3 of 5 carry a non-finite gradient: the average is bitwise unchanged across them and what follows uses
    n = 2, 3 -- equal to a run that never saw them."""
    rng = np.random.default_rng(1)
    init = [rng.standard_normal(6), rng.standard_normal(3)]
    good = [[rng.standard_normal(6), rng.standard_normal(3)] for _ in range(3)]
    bad = [np.array([1.0, np.inf, 0, 0, 0, 0]), np.ones(3)], [np.full(6, np.nan), np.ones(3)]
    for ramp in (None, 4.0):
        a = ClipAdamWEmaReference(init, 1e-2, max_norm=0.1, ema_decay=0.9, ema_ramp=ramp)
        b = ClipAdamWEmaReference(init, 1e-2, max_norm=0.1, ema_decay=0.9, ema_ramp=ramp)
        a.step(good[0])
        b.step(good[0])
        before = [e.copy() for e in a.ema.e]
        for g in bad:
            a.step(list(g))
            assert all(np.array_equal(x, y) for x, y in zip(before, a.ema.e))
        assert a.skipped == 2 and a.step_count == 1 and a.ema.n == 1
        for g in good[1:]:
            a.step(g)
            b.step(g)
        assert a.ema.n == b.ema.n == 3
        assert all(np.array_equal(x, y) for x, y in zip(a.ema.e, b.ema.e))
    # and counting the skipped steps would have given something else in ramp mode
    assert EmaReference(init, 0.9, 4.0).weight(2) != EmaReference(init, 0.9, 4.0).weight(4)


def test_reference_gradient_less_tensor_converges_to_its_value():
    """A tensor that stops getting gradients: its parameter stands still and its average closes in on it geometrically."""
    rng = np.random.default_rng(2)
    init = [rng.standard_normal(5), rng.standard_normal(4)]
    ref = ClipAdamWEmaReference(init, 1e-1, max_norm=None, ema_decay=0.5)
    for _ in range(3):
        ref.step([rng.standard_normal(5), rng.standard_normal(4)])
    p1 = ref.p[1].copy()
    gap = np.abs(ref.ema.e[1] - p1).max()
    assert gap > 0.0
    for k in range(1, 6):
        ref.step([rng.standard_normal(5), None])
        assert np.array_equal(ref.p[1], p1)
        assert np.abs(ref.ema.e[1] - p1).max() <= gap * 0.5 ** k * (1 + 1e-12)
    assert ref.step_count == 8 and ref.ema.n == 8


def test_ema_symbols_declared_and_exported(hip_lib):
    from unidistill_amd import _lib
    declared = _lib.exported_symbols()      # the prototypes parsed from unidistill_hip.h (test_abi.py counts them independently)
    for n in EMA_SYMBOLS:
        assert n in declared, f"{n} not declared in unidistill_hip.h"
        assert hasattr(hip_lib, n), f"{n} declared in unidistill_hip.h but not exported"


def test_ema_launchers_reject_bad_arguments_without_a_gpu(hip_lib):
    ema = hip_lib.ud_optim_clip_adamw_ema
    nulls = [None] * 7
    assert ema(None, 1, *nulls, 0.9, 0.999, 1e-8, 0.0, 0.1, 1, 0.999, 0.0, None) == -1        # null tables
    one = 1                                                                                        # never dereferenced:
    assert ema(None, 0, *nulls[:6], one, 0.9, 0.999, 1e-8, 0.0, 0.1, 1, 0.999, 0.0, None) == 0   # no chunks, nothing to do
    for decay in (0.0, 1.0, float("nan")):
        assert ema(None, 0, *nulls[:6], one, 0.9, 0.999, 1e-8, 0.0, 0.1, 1, decay, 0.0, None) == -1
    assert ema(None, 0, *nulls[:6], one, 0.9, 0.999, 1e-8, 0.0, 0.1, 1, 0.9, float("nan"), None) == -1
    assert hip_lib.ud_optim_swap(None, 1, None, None, None) == -1
    assert hip_lib.ud_optim_swap(None, -1, None, None, None) == -1
    assert hip_lib.ud_optim_swap(None, 0, None, None, None) == 0
