"""GPU: the weight EMA of ops.optim.ClipAdamW (csrc/optim.hip: k_optim_clip_adamw<EMA>, k_optim_swap) against the float64
reference of tests/ema_reference.py, and what train.Trainer / train.ValidationStep build on it.

The parity bound follows tests/test_optim_gpu.py and is measured, not chosen: torch._foreach_lerp_ runs in fp32 on the same
device over the same parameter trajectory (the fp32 parameters ClipAdamW produced, step by step) with the same weights, its
maximum error against the float64 reference over that trajectory is taken, and the fused EMA must stay within 2 x that error
plus one fp32 ulp of the value, element by element, after every step.

Measured on an MI355X (6 steps, the tensor set below), max |error| of torch._foreach_lerp_ / of the fused average: constant
0.999 5.20e-07 / 5.20e-07, constant 0.9 4.59e-07 / 4.15e-07, ramp 0.999 3.14e-07 / 3.14e-07, ramp 0.9 2.90e-07 / 2.90e-07
(DESIGN.md, section 2.13)."""
import copy

import numpy as np
import pytest
import torch

from ema_reference import EmaReference

pytestmark = pytest.mark.gpu

LR, BETAS, EPS, WD, MAX_NORM = 2e-4, (0.9, 0.999), 1e-8, 1e-7, 0.1
NORMS = (0.5, 0.03, 2.0, 0.05, 0.2, 0.08)         # total gradient norm per step: on both sides of MAX_NORM
RAMP = 4.0                                        # six steps cross 1 - exp(-6 / 4) = 78 % of the ramp
MODES = {"const-0.999": (0.999, None), "const-0.9": (0.9, None), "ramp-0.999": (0.999, RAMP), "ramp-0.9": (0.9, RAMP)}
I_TWO_CHUNKS, I_VIEW, I_EMPTY, I_NOGRAD = 5, 6, 7, 8


def _dev():
    return torch.device("cuda:0")


def _chunk():
    from unidistill_amd.ops import optim
    return optim.chunk_elems()


def _make_params(seed=0):
    """1, 3, 4, 7 and 1030 elements (below, at and past one float4 group, a tail after whole groups); chunk + 5 (two chunks, the
    last short and odd); a view at a 12-byte offset (the 4-byte path); an empty tensor; one whose gradient stays None.
    -> (params, number of leading tensors that get gradients)."""
    g = torch.Generator().manual_seed(seed)
    dev = _dev()
    params = [torch.randn(n, generator=g).to(dev) for n in (1, 3, 4, 7, 1030, _chunk() + 5)]
    buf = torch.randn(1024 + 8, generator=g).to(dev)
    params.append(buf[3:3 + 1001])
    assert params[I_VIEW].data_ptr() % 16 == 12
    params.append(torch.randn(0, generator=g).to(dev))
    n_live = len(params)
    params.append(torch.randn(41, generator=g).to(dev))
    for p in params:
        p.requires_grad_(True)
    return params, n_live


def _make_grads(params, n_live, norms=NORMS, seed=1):
    g = torch.Generator().manual_seed(seed)
    out = []
    for norm in norms:
        gs = [torch.randn(p.shape, generator=g).to(p.device) for p in params[:n_live]]
        total = float(torch.sqrt(sum((x.double() ** 2).sum() for x in gs)))
        out.append([x * (norm / total) for x in gs])
    return out


def _set_grads(params, n_live, grads):
    for p, g in zip(params[:n_live], grads):
        p.grad = g.clone()
    for p in params[n_live:]:
        p.grad = None


def _f64(t):
    return t.detach().double().cpu().numpy().ravel()


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _optimizer(params, decay=None, ramp=None, order=None, **kw):
    from unidistill_amd.ops.optim import ClipAdamW
    reg = params if order is None else [params[i] for i in order]
    return ClipAdamW(reg, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_norm=MAX_NORM, ema_decay=decay, ema_ramp=ramp, **kw)


def _ema_of(opt, params):
    """The average per tensor of ``params`` (whatever the registration order), cloned."""
    by_id = {id(p): e for p, e in zip(opt.param_groups[0]["params"], opt.ema_params())}
    return [by_id[id(p)].detach().clone() for p in params]


def _run(params, n_live, grads, decay, ramp, order=None, opt=None, before_steps=None):
    """-> (optimizer, per step the parameters, per step the averages), all cloned, in the order of ``params``."""
    if opt is None:
        opt = _optimizer(params, decay, ramp, order)
    if before_steps is not None:
        before_steps(opt)
    traj, emas = [], []
    for gs in grads:
        _set_grads(params, n_live, gs)
        opt.step()
        traj.append([p.detach().clone() for p in params])
        emas.append(_ema_of(opt, params))
    return opt, traj, emas


def _reference_and_torch(start, traj, decay, ramp, applied=None):
    """The float64 recurrence and torch._foreach_lerp_ (fp32, this device) over the trajectory ``traj``, both started at
    ``start``.  -> (per step the reference averages, torch's maximum error against them over all steps and tensors)."""
    ref = EmaReference([_f64(e) for e in start], decay, ramp)
    t_ema = [e.detach().clone() for e in start]
    refs, e_torch = [], 0.0
    for s, ps in enumerate(traj):
        ok = applied is None or applied[s]
        ref.update([_f64(p) for p in ps], applied=ok)
        if ok:
            torch._foreach_lerp_(t_ema, ps, ref.weight(ref.n))
        refs.append([e.copy() for e in ref.e])
        e_torch = max([e_torch] + [float(np.abs(_f64(t) - r).max()) for t, r in zip(t_ema, ref.e) if r.size])
    return refs, e_torch


def _assert_within(emas, refs, e_torch, what):
    worst = 0.0
    for s, (es, rs) in enumerate(zip(emas, refs)):
        for i, (e, r) in enumerate(zip(es, rs)):
            if not r.size:
                continue
            err = np.abs(_f64(e) - r)
            worst = max(worst, float(err.max()))
            excess = err - (2.0 * e_torch + _ulp(r))
            assert excess.max() <= 0.0, f"{what}: EMA of tensor {i} after step {s + 1} misses the parity bound by {excess.max():.3e}"
    return worst


@pytest.fixture(scope="module")
def base(hip_lib):
    """Initial parameters, the six gradient sets and the run WITHOUT an EMA that everything else is compared with."""
    params, n_live = _make_params()
    init = [p.detach().clone() for p in params]
    grads = _make_grads(params, n_live)

    def fresh():
        ps, _ = _make_params()
        for a, b in zip(ps, init):
            assert torch.equal(a, b)
        return ps
    plain_opt = _optimizer(params)
    traj, scalars = [], []
    for gs in grads:
        _set_grads(params, n_live, gs)
        plain_opt.step()
        traj.append([p.detach().clone() for p in params])
        scalars.append((plain_opt.last_norm.clone(), plain_opt.last_coef.clone(), plain_opt.steps_done.clone()))
    torch.cuda.synchronize()
    coefs = [float(c) for _, c, _ in scalars]
    assert [c < 1.0 for c in coefs] == [True, False, True, False, True, False]
    return dict(fresh=fresh, n_live=n_live, init=init, grads=grads, plain_opt=plain_opt, plain_params=params, plain_traj=traj,
                plain_scalars=scalars)


@pytest.fixture(scope="module")
def runs(base):
    """One six-step run per mode; none is modified later."""
    out = {}
    for name, (decay, ramp) in MODES.items():
        ps = base["fresh"]()
        opt, traj, emas = _run(ps, base["n_live"], base["grads"], decay, ramp)
        out[name] = dict(params=ps, opt=opt, traj=traj, emas=emas)
    torch.cuda.synchronize()
    return out


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_parity_with_float64_reference(base, runs, mode):
    decay, ramp = MODES[mode]
    R = runs[mode]
    refs, e_torch = _reference_and_torch(base["init"], R["traj"], decay, ramp)
    worst = _assert_within(R["emas"], refs, e_torch, mode)
    print("\n%s: max |EMA - float64| over 6 steps   torch._foreach_lerp_ %.3e / fused %.3e" % (mode, e_torch, worst))
    assert float(R["opt"].steps_done) == 6 and float(R["opt"].skipped) == 0
    # the average did move, and lags the weights
    assert not torch.equal(R["emas"][-1][4], base["init"][4]) and not torch.equal(R["emas"][-1][4], R["traj"][-1][4])
    if ramp is not None:                             # the first steps of the ramp take torch's other lerp branch (w >= 0.5)
        w = [EmaReference([], decay, ramp).weight(n) for n in range(1, 7)]
        assert w[0] >= 0.5 > w[-1]
    views = R["opt"].ema_params()
    assert [(tuple(v.shape), v.stride()) for v in views] == [(tuple(p.shape), p.stride()) for p in R["params"]]


# ---- 2. the EMA changes nothing else -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["const-0.9", "ramp-0.999"])
def test_ema_changes_nothing_else(base, runs, mode):
    R = runs[mode]
    for s, (a, b) in enumerate(zip(R["traj"], base["plain_traj"])):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), f"parameters differ after step {s + 1}"
    sd, sd0 = R["opt"].state_dict(), base["plain_opt"].state_dict()
    assert sd["param_groups"] == sd0["param_groups"] and sorted(sd["state"]) == sorted(sd0["state"])
    for k, st in sd["state"].items():
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        for name in st:
            assert torch.equal(st[name], sd0["state"][k][name]), (k, name)
    norm, coef, steps = base["plain_scalars"][-1]
    assert torch.equal(R["opt"].last_norm, norm) and torch.equal(R["opt"].last_coef, coef)
    assert torch.equal(R["opt"].steps_done, steps) and float(steps) == 6


def test_without_ema_nothing_is_allocated_or_exposed(base):
    opt = base["plain_opt"]
    assert opt.ema_decay is None and opt._flat.shape[0] == 2 and opt._ptrs_dev.shape[0] == 4
    for call in (opt.ema_params, opt.swap_ema, opt.ema_state_dict, opt.reset_ema):
        with pytest.raises(RuntimeError, match="no EMA"):
            call()
    assert not any("ema" in k for k in opt.state_dict()["param_groups"][0])


# ---- 3. the guard ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ramp-0.9", "const-0.9"])
def test_guard_freezes_the_average_and_the_ramp(base, mode):
    decay, ramp = MODES[mode]
    n_live = base["n_live"]
    grads = [[g.clone() for g in gs] for gs in base["grads"]]
    grads[2][I_TWO_CHUNKS][_chunk() + 1] = float("inf")            # step 3, second chunk of the two-chunk tensor
    ps = base["fresh"]()
    opt, traj, emas = _run(ps, n_live, grads, decay, ramp)
    assert float(opt.skipped) == 1 and float(opt.steps_done) == 5
    for a, b in zip(emas[1], emas[2]):                              # bitwise unchanged across the skipped step
        assert torch.equal(a, b)
    for a, b in zip(traj[1], traj[2]):
        assert torch.equal(a, b)
    applied = [True, True, False, True, True, True]
    refs, e_torch = _reference_and_torch(base["init"], traj, decay, ramp, applied)
    _assert_within(emas, refs, e_torch, mode + " with step 3 skipped")      # step 4 is held to n = 3
    if ramp is not None:
        # what an average that counts calls would have done at step 4 (n = 4) lies outside the bound: the test can tell
        w4 = EmaReference([], decay, ramp).weight(4)
        wrong = refs[2][4] + w4 * (_f64(traj[3][4]) - refs[2][4])
        assert (np.abs(wrong - refs[3][4]) - (2.0 * e_torch + _ulp(refs[3][4]))).max() > 0.0


# ---- 4. a tensor without a gradient ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["const-0.9", "ramp-0.999"])
def test_gradient_less_tensor_is_averaged_but_not_stepped(base, mode):
    """Its average is moved off it before the first step (an average that starts ON a constant stays there whatever the
    kernel does), then has to follow the lerp towards the constant; parameter and moments stay untouched."""
    decay, ramp = MODES[mode]
    ps = base["fresh"]()
    start = [p.detach().clone() for p in base["init"]]
    start[I_NOGRAD] += 0.5

    def push(opt):
        with torch.no_grad():
            opt.ema_params()[I_NOGRAD].add_(0.5)
    opt, traj, emas = _run(ps, base["n_live"], base["grads"], decay, ramp, before_steps=push)
    refs, e_torch = _reference_and_torch(start, traj, decay, ramp)
    _assert_within(emas, refs, e_torch, mode)
    gaps = [float((e[I_NOGRAD] - base["init"][I_NOGRAD]).abs().max()) for e in emas]
    assert all(a > b for a, b in zip([0.5 + 1e-6] + gaps, gaps)) and gaps[-1] > 0.0
    assert torch.equal(ps[I_NOGRAD], base["init"][I_NOGRAD])
    sd = opt.state_dict()["state"][I_NOGRAD]
    assert not sd["exp_avg"].any() and not sd["exp_avg_sq"].any()


# ---- 5. reproducibility ---------------------------------------------------------------------------------------------------
def test_bitwise_reproducible_and_independent_of_registration_order(base, runs):
    decay, ramp = MODES["ramp-0.9"]
    want = runs["ramp-0.9"]["emas"]
    again = base["fresh"]()
    _, _, emas2 = _run(again, base["n_live"], base["grads"], decay, ramp)
    rev = base["fresh"]()
    _, _, emas3 = _run(rev, base["n_live"], base["grads"], decay, ramp, order=list(range(len(rev)))[::-1])
    for s in range(len(want)):
        for i, (a, b, c) in enumerate(zip(want[s], emas2[s], emas3[s])):
            assert torch.equal(a, b), f"second run: tensor {i} after step {s + 1}"
            assert torch.equal(a, c), f"reversed registration: tensor {i} after step {s + 1}"


# ---- 6. swap -------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_swap_is_an_exact_exchange(base):
    decay, ramp = MODES["const-0.9"]
    ps = base["fresh"]()
    opt, _, _ = _run(ps, base["n_live"], base["grads"][:2], decay, ramp)
    with torch.no_grad():                            # bit patterns arithmetic would not keep: -0.0, inf, a NaN with a payload
        special = torch.tensor([-0.0, float("inf"), float("nan")], device=_dev())
        special.view(torch.int32)[2] = 0x7FC12345
        opt.ema_params()[1].copy_(special)
        ps[3][:3].copy_(special.flip(0))
    p0 = [_bits(p).clone() for p in ps]
    e0 = [_bits(e).clone() for e in opt.ema_params()]
    assert any(not torch.equal(a, b) for a, b in zip(p0, e0))
    opt.swap_ema()
    assert opt.ema_swapped
    assert all(torch.equal(_bits(p), e) for p, e in zip(ps, e0))
    assert all(torch.equal(_bits(e), p) for e, p in zip(opt.ema_params(), p0))
    opt.swap_ema()
    assert not opt.ema_swapped
    assert all(torch.equal(_bits(p), a) for p, a in zip(ps, p0))
    assert all(torch.equal(_bits(e), a) for e, a in zip(opt.ema_params(), e0))
    with opt.ema_weights():
        assert opt.ema_swapped
        assert all(torch.equal(_bits(p), e) for p, e in zip(ps, e0))
        _set_grads(ps, base["n_live"], base["grads"][2])
        with pytest.raises(RuntimeError, match="swapped"):
            opt.step()
        with pytest.raises(RuntimeError, match="swapped"):
            opt.state_dict()
        with pytest.raises(RuntimeError, match="swapped"):
            opt.ema_state_dict()
    assert not opt.ema_swapped
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("inside")
    assert not opt.ema_swapped
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(p), a) for p, a in zip(ps, p0))
    assert all(torch.equal(_bits(e), a) for e, a in zip(opt.ema_params(), e0))
    assert float(opt.steps_done) == 2                 # the refused step() launched nothing


# ---- 7. checkpoints ----------------------------------------------------------------------------------------------------------
class _TinyStep(torch.nn.Module):
    """Elementwise only (no GEMM, no convolution): what is under test is the trainer around the optimizer."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.a = torch.nn.Parameter(torch.randn(1030, generator=g))
        self.b = torch.nn.Parameter(torch.randn(7, generator=g))
        self.unused = torch.nn.Parameter(torch.randn(5, generator=g))

    def forward(self, batch):
        return {"loss": ((self.a * batch["x"]) ** 2).mean() + (self.b * batch["y"]).sum()}


def _tiny_trainer(**kw):
    from unidistill_amd import train
    return train.Trainer(_TinyStep(), device=_dev(), optimizer="hip", lr=1e-2, **kw)


def test_trainer_checkpoint_round_trip_is_bitwise(hip_lib):
    dev = _dev()
    g = torch.Generator().manual_seed(4)
    batches = [{"x": torch.randn(1030, generator=g).to(dev), "y": torch.randn(7, generator=g).to(dev)} for _ in range(4)]
    tr = _tiny_trainer(ema_decay=0.9, ema_ramp=RAMP)
    for b in batches[:2]:
        tr.step(b)
    state = copy.deepcopy(tr.state_dict())
    model_state = copy.deepcopy(tr.module.state_dict())
    assert set(state) == {"optimizer", "epoch", "scheduler", "ema"}
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in state["optimizer"]["state"].values())
    for b in batches[2:]:
        tr.step(b)
    want = [e.clone() for e in tr.opt.ema_params()]
    tr2 = _tiny_trainer(ema_decay=0.9, ema_ramp=RAMP)
    tr2.module.load_state_dict(model_state)
    tr2.load_state_dict(state)
    assert float(tr2.opt.steps_done) == 2
    for b in batches[2:]:
        tr2.step(b)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(tr2.opt.ema_params(), want))
    assert all(torch.equal(a, b) for a, b in zip(tr2.params, tr.params))
    assert any(not torch.equal(e, p) for e, p in zip(want, tr.params))
    # the optimizer part is still torch.optim.AdamW's
    topt = torch.optim.AdamW(tr2.params, lr=1e-2, weight_decay=1e-7, fused=True)
    topt.load_state_dict(state["optimizer"])
    assert topt.param_groups[0]["fused"] is True and float(topt.state[tr2.params[0]]["step"]) == 2.0
    # a checkpoint from before the EMA: the average restarts at the loaded weights
    old = {k: v for k, v in state.items() if k != "ema"}
    tr3 = _tiny_trainer(ema_decay=0.9)
    tr3.step(batches[0])                              # so that the average and the weights differ before the load
    tr3.module.load_state_dict(model_state)
    tr3.load_state_dict(old)
    assert all(torch.equal(e, p) for e, p in zip(tr3.opt.ema_params(), tr3.params))
    assert all(torch.equal(p, model_state[k]) for k, p in tr3.module.state_dict().items())
    # and a trainer without an EMA carries no "ema" entry and ignores one
    tr4 = _tiny_trainer()
    assert "ema" not in tr4.state_dict()
    tr4.load_state_dict(state)
    with pytest.raises(RuntimeError, match="no EMA"):
        with tr4.ema_weights():
            pass


# ---- 8. Trainer + ValidationStep ------------------------------------------------------------------------------------------
class _Collect:
    def __init__(self):
        self.calls = []

    def add_batch(self, sample_ids, pred_dicts, lidar_to_global):
        self.calls.append((sample_ids, pred_dicts))


def _same_predictions(a, b):
    return len(a) == len(b) and all(set(x) == set(y) and all(torch.equal(x[k], y[k]) for k in x) for x, y in zip(a, b))


def test_validation_step_runs_on_the_averaged_weights(hip_lib):
    from unidistill_amd import ops, train
    dev = _dev()
    torch.manual_seed(0)
    tr = train.Trainer(train.DetectStep("lidar"), device=dev, optimizer="hip", lr=2e-4, ema_decay=0.9)
    batch = train.synthetic_batch(dev, batch_size=1, with_imgs=False)
    for _ in range(3):
        out = tr.step(batch)
    assert torch.isfinite(out["loss"]) and float(tr.opt.skipped) == 0
    model = tr.module.model
    before = [p.detach().clone() for p in tr.params]
    l2g = torch.eye(4, dtype=torch.float64, device=dev)[None]
    live = train.ValidationStep(model, _Collect())(batch, [0], l2g)           # fills the frozen-weight caches from the live weights
    seen = _Collect()
    got = train.ValidationStep(model, seen, weights=tr.ema_weights)(batch, [0], l2g)
    assert len(seen.calls) == 1 and not tr.opt.ema_swapped and model.training
    assert all(torch.equal(a, b) for a, b in zip(tr.params, before))           # the training weights are back, bitwise
    live_again = train.ValidationStep(model, _Collect())(batch, [0], l2g)     # and nothing cached from the average survives
    assert _same_predictions(live, live_again)
    # the same forward on a copy whose parameters were overwritten with the average by plain copy_
    twin = copy.deepcopy(model)
    ops.invalidate_caches(twin)
    twin_params = [p for p in twin.parameters() if p.requires_grad]
    assert len(twin_params) == len(tr.params)
    with torch.no_grad():
        for p, e in zip(twin_params, tr.opt.ema_params()):
            p.copy_(e)
    want = train.ValidationStep(twin, _Collect())(batch, [0], l2g)
    torch.cuda.synchronize()
    assert _same_predictions(got, want)
    assert sum(len(d["pred_scores"]) for d in got) > 0 and not _same_predictions(got, live)     # the comparison is not vacuous
    assert any(not torch.equal(e, p) for e, p in zip(tr.opt.ema_params(), tr.params))


# ---- 9. cannot run -----------------------------------------------------------------------------------------------------------
def test_ema_needs_the_hip_optimizer(hip_lib):
    from unidistill_amd import train
    with pytest.raises(ValueError, match="optimizer='hip'"):
        train.Trainer(train.DetectStep(model=torch.nn.Linear(4, 4)), device=_dev(), optimizer="torch", ema_decay=0.9)


# ---- 10. graph capture -------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_equal_eager_steps(base, runs):
    decay, ramp = MODES["ramp-0.9"]
    n_live, grads = base["n_live"], base["grads"]
    R = runs["ramp-0.9"]                              # the eager steps
    ps = base["fresh"]()
    opt = _optimizer(ps, decay, ramp)
    for p, g in zip(ps[:n_live], grads[0]):
        p.grad = g.clone()                            # static gradient buffers from here on
    opt.step()                                        # eager: the pointer table reaches the device
    uploads, builds = opt.grad_uploads, opt.table_builds
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                     # two kernels on one stream: a straight chain
        opt.step()
    assert (opt.grad_uploads, opt.table_builds) == (uploads, builds)
    for gs in grads[1:4]:
        for p, g in zip(ps[:n_live], gs):
            p.grad.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert float(opt.steps_done) == 4
    assert all(torch.equal(a, b) for a, b in zip(ps, R["traj"][3]))
    assert all(torch.equal(a, b) for a, b in zip(_ema_of(opt, ps), R["emas"][3]))
    assert torch.equal(opt.last_norm, base["plain_scalars"][3][0])
