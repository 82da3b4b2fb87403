"""GPU: ops.optim.ClipAdamW (csrc/optim.hip) against the float64 reference of tests/optim_reference.py.

The parity bound is measured, not chosen: PyTorch's own path (clip_grad_norm_(foreach=True) + AdamW(fused=True)) runs on the
same inputs, its maximum error against the float64 reference is taken per quantity (p, exp_avg, exp_avg_sq, total_norm),
and the new path must stay within 2x that error plus one fp32 ulp of the value (the factor 2 allows for a different but
equally valid summation / FMA order).

Measured on an MI355X (5 steps, the tensor set below), max |error| of the torch path / of ClipAdamW: p 7.94e-07 / 7.94e-07,
exp_avg 1.54e-11 / 1.89e-11, exp_avg_sq 1.78e-16 / 2.18e-16, total_norm 1.84e-08 / 1.14e-08."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
from optim_reference import ClipAdamWReference

pytestmark = pytest.mark.gpu

LR, BETAS, EPS, WD, MAX_NORM = 2e-4, (0.9, 0.999), 1e-8, 1e-7, 0.1
NORMS = (0.5, 0.03, 2.0, 0.05, 0.2)               # total gradient norm per step: clipped, not, clipped, not, clipped
QUANTITIES = ("p", "exp_avg", "exp_avg_sq", "total_norm")


def _dev():
    return torch.device("cuda:0")


def _chunk():
    from unidistill_amd.ops import optim
    return optim.chunk_elems()


def _make_params(seed=0):
    """Sizes on every edge of the chunking and of the 16-byte path; -> (params, names of those that get gradients)."""
    c = _chunk()
    g = torch.Generator().manual_seed(seed)
    dev = _dev()
    params = [torch.randn(n, generator=g).to(dev) for n in (1, 3, 4, 5, 63, 64, 65, c - 1, c, c + 1, 2 * c + 3)]
    params.append(torch.randn(16, 8, 3, 3, generator=g).to(dev).contiguous(memory_format=torch.channels_last))
    params.append(torch.randn(8, 4, 1, 1, generator=g).to(dev))
    buf = torch.randn(1024 + 8, generator=g).to(dev)
    params.append(buf[3:3 + 1001])                 # storage offset 12 bytes: 4-byte but not 16-byte aligned
    assert params[-1].data_ptr() % 16 == 12
    n_live = len(params)
    params.append(torch.randn(37, generator=g).to(dev))           # requires_grad=False
    params.append(torch.randn(41, generator=g).to(dev))           # requires_grad=True, grad stays None
    for i, p in enumerate(params):
        p.requires_grad_(i != n_live)
    return params, n_live


def _make_grads(params, n_live, steps=len(NORMS), seed=1, norms=NORMS):
    """Per step a list of gradients (same layout as the parameter), scaled to the step's total norm."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in range(steps):
        gs = [torch.randn(p.shape, generator=g).to(p.device) for p in params[:n_live]]
        gs = [x.contiguous(memory_format=torch.channels_last) if p.dim() == 4 and p.stride() != x.stride() else x
              for x, p in zip(gs, params)]
        total = float(torch.sqrt(sum((x.double() ** 2).sum() for x in gs)))
        out.append([x * (norms[s] / total) for x in gs])
    return out


def _flat(t):
    """Elements in storage order as float64 numpy (elementwise comparisons only need one consistent order)."""
    if t.dim() == 4 and not t.is_contiguous():
        t = t.permute(0, 2, 3, 1)
    return t.detach().double().cpu().numpy().ravel()


def _set_grads(params, n_live, grads):
    for p, g in zip(params[:n_live], grads):
        p.grad = g.clone()
    for p in params[n_live:]:
        p.grad = None


def _run_new(params, n_live, grads, milestones=None, order=None, skip_nonfinite=True, opt=None, max_norm=MAX_NORM):
    from unidistill_amd.ops.optim import ClipAdamW
    reg = params if order is None else [params[i] for i in order]
    if opt is None:
        opt = ClipAdamW(reg, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_norm=max_norm, skip_nonfinite=skip_nonfinite)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, list(milestones), gamma=0.1) if milestones else None
    norms = []
    for gs in grads:
        _set_grads(params, n_live, gs)
        opt.step()
        norms.append(opt.last_norm.clone())
        if sched is not None:
            sched.step()
    return opt, [float(n) for n in norms]


def _run_torch(params, n_live, grads, milestones=None, opt=None):
    if opt is None:
        opt = torch.optim.AdamW(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, fused=True)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, list(milestones), gamma=0.1) if milestones else None
    norms = []
    for gs in grads:
        _set_grads(params, n_live, gs)
        norms.append(torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True))
        opt.step()
        if sched is not None:
            sched.step()
    return opt, [float(n) for n in norms]


def _run_ref(params, n_live, grads, milestones=None, skip_nonfinite=True):
    ref = ClipAdamWReference([_flat(p) for p in params], LR, BETAS, EPS, WD, MAX_NORM, skip_nonfinite)
    norms, lr = [], LR
    for s, gs in enumerate(grads):
        ref.lr = lr
        ref.step([_flat(g) for g in gs] + [None] * (len(params) - n_live))
        norms.append(ref.total_norm)
        if milestones and (s + 1) in milestones:
            lr *= 0.1
    return ref, norms


def _state_of(opt, params, n_live):
    """(p, exp_avg, exp_avg_sq) per live parameter as float64 storage-order arrays, through the public state_dict()."""
    sd = opt.state_dict()
    index = {id(p): k for k, p in zip(sd["param_groups"][0]["params"], opt.param_groups[0]["params"])}
    out = []
    for p in params[:n_live]:
        st = sd["state"][index[id(p)]]
        out.append((_flat(p), _flat(st["exp_avg"]), _flat(st["exp_avg_sq"])))
    return out


def _errors(state, norms, ref, ref_norms):
    """max |x - ref| per quantity."""
    e = dict.fromkeys(QUANTITIES, 0.0)
    for i, (p, m, v) in enumerate(state):
        e["p"] = max(e["p"], float(np.abs(p - ref.p[i]).max()))
        e["exp_avg"] = max(e["exp_avg"], float(np.abs(m - ref.m[i]).max()))
        e["exp_avg_sq"] = max(e["exp_avg_sq"], float(np.abs(v - ref.v[i]).max()))
    e["total_norm"] = max(abs(a - b) for a, b in zip(norms, ref_norms))
    return e


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _assert_within(state, norms, ref, ref_norms, e_torch, what):
    """|new - ref| <= 2 x (torch's max error for that quantity) + one fp32 ulp of the value, element by element."""
    for i, (p, m, v) in enumerate(state):
        for name, got, want in (("p", p, ref.p[i]), ("exp_avg", m, ref.m[i]), ("exp_avg_sq", v, ref.v[i])):
            excess = np.abs(got - want) - (2.0 * e_torch[name] + _ulp(want))
            assert excess.max() <= 0.0, f"{what}: {name} of tensor {i} misses the parity bound by {excess.max():.3e}"
    for s, (a, b) in enumerate(zip(norms, ref_norms)):
        assert abs(a - b) <= 2.0 * e_torch["total_norm"] + float(_ulp(b)), f"{what}: total_norm of step {s + 1}: {a!r} vs {b!r}"


@pytest.fixture(scope="module")
def parity(hip_lib):
    """The shared 5-step runs: float64 reference, PyTorch's fused path (the bound) and ClipAdamW; none is modified later."""
    params, n_live = _make_params()
    grads = _make_grads(params, n_live)
    init = [p.detach().clone() for p in params]

    def fresh():
        ps, _ = _make_params()
        for a, b in zip(ps, init):
            assert torch.equal(a, b)
        return ps
    ref, ref_norms = _run_ref(params, n_live, grads)
    pt = fresh()
    topt, t_norms = _run_torch(pt, n_live, grads)
    t_state = [(_flat(p), _flat(topt.state[p]["exp_avg"]), _flat(topt.state[p]["exp_avg_sq"])) for p in pt[:n_live]]
    e_torch = _errors(t_state, t_norms, ref, ref_norms)
    pn = fresh()
    nopt, n_norms = _run_new(pn, n_live, grads)
    n_state = _state_of(nopt, pn, n_live)
    e_new = _errors(n_state, n_norms, ref, ref_norms)
    torch.cuda.synchronize()
    print("\nmax |error| vs float64 after %d steps   torch fused path / ClipAdamW" % len(grads))
    for q in QUANTITIES:
        print("  %-11s %.3e / %.3e" % (q, e_torch[q], e_new[q]))
    return dict(fresh=fresh, n_live=n_live, grads=grads, init=init, ref=ref, ref_norms=ref_norms, e_torch=e_torch,
                new_params=pn, new_opt=nopt, new_state=n_state, new_norms=n_norms)


def test_parity_with_float64_reference(parity):
    P = parity
    assert [c < 1.0 for c in (min(1.0, MAX_NORM / (n + 1e-6)) for n in P["ref_norms"])] == [True, False, True, False, True]
    _assert_within(P["new_state"], P["new_norms"], P["ref"], P["ref_norms"], P["e_torch"], "5 steps")
    assert float(P["new_opt"].steps_done) == 5 and float(P["new_opt"].skipped) == 0
    assert float(P["new_opt"].last_coef) == pytest.approx(MAX_NORM / (P["ref_norms"][-1] + 1e-6), rel=1e-6)
    sd = P["new_opt"].state_dict()
    assert all(float(st["step"]) == 5.0 and st["step"].dtype == torch.float32 for st in sd["state"].values())
    # the frozen parameter and the one without a gradient are untouched
    for p, p0 in list(zip(P["new_params"], P["init"]))[P["n_live"]:]:
        assert torch.equal(p, p0)


def test_bitwise_reproducible_and_independent_of_registration_order(parity):
    P = parity
    n_live = P["n_live"]
    again = P["fresh"]()
    opt2, norms2 = _run_new(again, n_live, P["grads"])
    assert norms2 == P["new_norms"]
    for (p, m, v), (p2, m2, v2) in zip(P["new_state"], _state_of(opt2, again, n_live)):
        assert np.array_equal(p, p2) and np.array_equal(m, m2) and np.array_equal(v, v2)
    rev = P["fresh"]()
    opt3, norms3 = _run_new(rev, n_live, P["grads"], order=list(range(len(rev)))[::-1])
    _assert_within(_state_of(opt3, rev, n_live), norms3, P["ref"], P["ref_norms"], P["e_torch"], "reversed registration")
    for i, ((p, m, v), (p3, m3, v3)) in enumerate(zip(P["new_state"], _state_of(opt3, rev, n_live))):
        assert np.array_equal(p, p3) and np.array_equal(m, m3) and np.array_equal(v, v3), f"tensor {i}"


def test_gradients_are_left_unclipped(parity):
    P = parity
    ps = P["fresh"]()
    from unidistill_amd.ops.optim import ClipAdamW
    opt = ClipAdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_norm=MAX_NORM)
    _set_grads(ps, P["n_live"], P["grads"][0])                    # norm 0.5: clipping is active
    keep = [p.grad.clone() for p in ps[:P["n_live"]]]
    opt.step()
    assert float(opt.last_coef) < 1.0
    for p, g in zip(ps, keep):
        assert torch.equal(p.grad, g)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_guard_skips_a_step_with_a_non_finite_gradient(parity, bad):
    from unidistill_amd.ops.optim import ClipAdamW
    P = parity
    n_live = P["n_live"]
    ps = P["fresh"]()
    opt = ClipAdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_norm=MAX_NORM, skip_nonfinite=True)
    poisoned = [g.clone() for g in P["grads"][0]]
    poisoned[9].view(-1)[_chunk() + 0] = bad                       # the chunk+1 tensor, second chunk
    _set_grads(ps, n_live, poisoned)
    opt.step()
    assert float(opt.skipped) == 1 and float(opt.steps_done) == 0
    assert not np.isfinite(float(opt.last_norm))
    for (p, m, v), p0 in zip(_state_of(opt, ps, n_live), P["init"]):
        assert np.array_equal(p, _flat(p0)) and not m.any() and not v.any()
    # the next finite step is step 1 of a fresh run (bias correction for step = 1)
    _run_new(ps, n_live, P["grads"][:1], opt=opt)
    fresh = P["fresh"]()
    opt1, _ = _run_new(fresh, n_live, P["grads"][:1])
    assert float(opt.steps_done) == 1 and float(opt.skipped) == 1
    for (p, m, v), (p1, m1, v1) in zip(_state_of(opt, ps, n_live), _state_of(opt1, fresh, n_live)):
        assert np.array_equal(p, p1) and np.array_equal(m, m1) and np.array_equal(v, v1)
    # guard off: PyTorch's behaviour, the poison reaches the parameters
    loose = P["fresh"]()
    lopt = ClipAdamW(loose, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_norm=MAX_NORM, skip_nonfinite=False)
    _set_grads(loose, n_live, poisoned)
    lopt.step()
    assert float(lopt.skipped) == 0 and float(lopt.steps_done) == 1
    tq = P["fresh"]()
    _run_torch(tq, n_live, [poisoned])
    assert not bool(torch.isfinite(loose[9]).all())
    for a, b in zip(loose[:n_live], tq[:n_live]):           # inf: coef = 0 poisons its own element; nan: coef = nan, everything
        assert bool(torch.isfinite(a).all()) == bool(torch.isfinite(b).all())


def test_learning_rate_follows_the_scheduler(parity):
    P = parity
    n_live, grads = P["n_live"], P["grads"][:3]
    ref, ref_norms = _run_ref(P["fresh"](), n_live, grads, milestones=(1,))
    pt = P["fresh"]()
    topt, t_norms = _run_torch(pt, n_live, grads, milestones=(1,))
    t_state = [(_flat(p), _flat(topt.state[p]["exp_avg"]), _flat(topt.state[p]["exp_avg_sq"])) for p in pt[:n_live]]
    e_torch = _errors(t_state, t_norms, ref, ref_norms)
    pn = P["fresh"]()
    nopt, n_norms = _run_new(pn, n_live, grads, milestones=(1,))
    assert nopt.param_groups[0]["lr"] == pytest.approx(LR * 0.1)
    _assert_within(_state_of(nopt, pn, n_live), n_norms, ref, ref_norms, e_torch, "MultiStepLR")
    # and the rate did matter: a constant-rate run differs
    pc = P["fresh"]()
    _run_new(pc, n_live, grads)
    assert any(not torch.equal(a, b) for a, b in zip(pc[:n_live], pn[:n_live]))


def test_checkpoints_interchange_with_torch_adamw(parity):
    from unidistill_amd.ops.optim import ClipAdamW
    P = parity
    n_live, grads = P["n_live"], P["grads"]
    # 3 steps here, 2 more with torch
    pa = P["fresh"]()
    nopt, norms_a = _run_new(pa, n_live, grads[:3])
    topt = torch.optim.AdamW(pa, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, fused=True)
    topt.load_state_dict(nopt.state_dict())
    assert topt.param_groups[0]["fused"] is True
    topt, norms_a2 = _run_torch(pa, n_live, grads[3:], opt=topt)
    a_state = [(_flat(p), _flat(topt.state[p]["exp_avg"]), _flat(topt.state[p]["exp_avg_sq"])) for p in pa[:n_live]]
    _assert_within(a_state, norms_a + norms_a2, P["ref"], P["ref_norms"], P["e_torch"], "ClipAdamW -> AdamW")
    # 3 steps with torch, 2 more here
    pb = P["fresh"]()
    topt, norms_b = _run_torch(pb, n_live, grads[:3])
    nopt = ClipAdamW(pb, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_norm=MAX_NORM)
    sd = topt.state_dict()
    assert "max_norm" not in sd["param_groups"][0]
    nopt.load_state_dict(sd)
    assert nopt.param_groups[0]["max_norm"] == MAX_NORM and nopt.param_groups[0]["skip_nonfinite"] is True
    assert float(nopt.steps_done) == 3
    nopt, norms_b2 = _run_new(pb, n_live, grads[3:], opt=nopt)
    _assert_within(_state_of(nopt, pb, n_live), norms_b + norms_b2, P["ref"], P["ref_norms"], P["e_torch"], "AdamW -> ClipAdamW")


def test_graph_capture_replays_equal_eager_steps(parity, monkeypatch):
    from unidistill_amd.ops.optim import ClipAdamW
    P = parity
    n_live, grads = P["n_live"], P["grads"]
    eager = P["fresh"]()
    eopt, _ = _run_new(eager, n_live, grads[:4])
    ps = P["fresh"]()
    opt = ClipAdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_norm=MAX_NORM)
    for p, g in zip(ps[:n_live], grads[0]):
        p.grad = g.clone()                                          # static gradient buffers from here on
    opt.step()                                                      # eager: the pointer table reaches the device
    uploads, builds = opt.grad_uploads, opt.table_builds
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    assert (opt.grad_uploads, opt.table_builds) == (uploads, builds)
    for gs in grads[1:4]:
        for p, g in zip(ps[:n_live], gs):
            p.grad.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert float(opt.steps_done) == 4
    for (p, m, v), (p2, m2, v2) in zip(_state_of(eopt, eager, n_live), _state_of(opt, ps, n_live)):
        assert np.array_equal(p, p2) and np.array_equal(m, m2) and np.array_equal(v, v2)
    assert float(eopt.last_norm) == float(opt.last_norm)
    # a table that would have to be rebuilt / re-sent while capturing raises (nothing is captured here: the flag is faked)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    ps[0].grad = ps[0].grad.clone()
    with pytest.raises(RuntimeError, match="graph capture"):
        opt.step()
    with pytest.raises(RuntimeError, match="graph capture"):
        opt._build()


def test_rejects_what_it_cannot_step(hip_lib):
    from unidistill_amd.ops.optim import ClipAdamW
    dev = _dev()
    with pytest.raises(RuntimeError, match="fp32"):
        ClipAdamW([torch.zeros(8, device=dev, dtype=torch.bfloat16, requires_grad=True)], lr=LR)
    with pytest.raises(RuntimeError, match="not dense"):
        ClipAdamW([torch.zeros(8, 8, device=dev)[:, ::2].requires_grad_()], lr=LR)
    with pytest.raises(ValueError):
        ClipAdamW([torch.zeros(8, device=dev, requires_grad=True)], lr=LR, max_norm=0.0)


# ---- Trainer ---------------------------------------------------------------------------------------------------------------
class _Names(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = set()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.add(str(func))
        return func(*args, **(kwargs or {}))


def _trainer(kind):
    from unidistill_amd import train
    torch.manual_seed(0)
    return train.Trainer(train.DetectStep("camera"), device=_dev(), optimizer=kind, channels_last=True)


@pytest.fixture(scope="module")
def trainers(hip_lib):
    from unidistill_amd import _lib, train
    dev = _dev()
    batch = train.synthetic_batch(dev, 1, ncam=1, with_points=False)
    tt = _trainer("torch")
    p0 = [p.detach().clone() for p in tt.params]
    tt.step(batch)
    p1_torch = [p.detach().clone() for p in tt.params]
    del tt
    th = _trainer("hip")
    assert all(torch.equal(a, b) for a, b in zip(p0, th.params))
    with _lib.strict(True), _Names() as seen:
        th.step(batch)
    g1 = [None if p.grad is None else p.grad.detach().clone() for p in th.params]
    p1_hip = [p.detach().clone() for p in th.params]
    state = th.state_dict()
    state = {"optimizer": {"state": {k: {n: v.clone() for n, v in st.items()} for k, st in state["optimizer"]["state"].items()},
                           "param_groups": state["optimizer"]["param_groups"]},
             "epoch": state["epoch"], "scheduler": state["scheduler"]}
    model_state = {k: v.detach().clone() for k, v in th.module.state_dict().items()}
    th.step(batch)
    p2_hip = [p.detach().clone() for p in th.params]
    torch.cuda.synchronize()
    return dict(batch=batch, p0=p0, p1_torch=p1_torch, p1_hip=p1_hip, p2_hip=p2_hip, g1=g1, seen=seen.names, opt=th.opt,
                state=state, model_state=model_state)


def test_trainer_hip_step_matches_torch_step(trainers):
    """One whole-model step from identical seeds.  Both trainers see the same gradients (the step is bitwise reproducible),
    so the float64 reference steps from the hip trainer's UNCLIPPED p.grad; first-step updates are +-lr, which is what
    scales the measured bound."""
    T = trainers
    ref = ClipAdamWReference([_flat(p) for p in T["p0"]], LR, BETAS, EPS, WD, MAX_NORM)
    ref.step([None if g is None else _flat(g) for g in T["g1"]])
    e_torch = max(float(np.abs(_flat(p) - r).max()) for p, r in zip(T["p1_torch"], ref.p))
    e_hip = max(float(np.abs(_flat(p) - r).max()) for p, r in zip(T["p1_hip"], ref.p))
    print("\ntrainer step: max |p - float64| torch %.3e / hip %.3e (lr %g, total_norm %.4f, coef %.4f)"
          % (e_torch, e_hip, LR, ref.total_norm, ref.coef))
    for i, (p, r) in enumerate(zip(T["p1_hip"], ref.p)):
        excess = np.abs(_flat(p) - r) - (2.0 * e_torch + _ulp(r))
        assert excess.max() <= 0.0, f"parameter {i} misses the parity bound by {excess.max():.3e}"
    assert float(T["opt"].skipped) == 0 and float(T["opt"].steps_done) == 2
    assert sum(int(not torch.equal(a, b)) for a, b in zip(T["p0"], T["p1_hip"])) >= 0.95 * len(T["p0"])


def test_trainer_hip_step_issues_no_torch_optimizer_ops(trainers):
    seen = trainers["seen"]
    assert any("aten." in n for n in seen)
    bad = sorted(n for n in seen if "_fused_adam" in n or "_foreach_norm" in n or "_foreach_mul" in n)
    assert not bad, bad


def test_trainer_hip_checkpoint_round_trip_is_bitwise(trainers):
    T = trainers
    tr = _trainer("hip")
    tr.module.load_state_dict(T["model_state"])
    tr.load_state_dict(T["state"])
    assert float(tr.opt.steps_done) == 1
    tr.step(T["batch"])
    torch.cuda.synchronize()
    bad = [i for i, (a, b) in enumerate(zip(tr.params, T["p2_hip"])) if not torch.equal(a, b)]
    assert not bad, (len(bad), bad[:8])


def test_ud_optim_env_selects_the_hip_path(hip_lib, monkeypatch):
    from unidistill_amd import train
    from unidistill_amd.ops.optim import ClipAdamW
    lin = lambda: train.DetectStep(model=torch.nn.Linear(4, 4))      # never stepped: only the choice of optimizer is looked at
    monkeypatch.setenv("UD_OPTIM", "hip")
    assert isinstance(train.Trainer(lin(), device=_dev()).opt, ClipAdamW)
    assert isinstance(train.Trainer(lin(), device=_dev(), optimizer="torch").opt, torch.optim.AdamW)
    monkeypatch.delenv("UD_OPTIM")
    assert isinstance(train.Trainer(lin(), device=_dev()).opt, torch.optim.AdamW)
    with pytest.raises(ValueError):
        train.Trainer(lin(), device=_dev(), optimizer="sgd")


# ---- DDP: gradients are bucket views, the gradient table is sent once -----------------------------------------------------
_DDP_SCRIPT = r'''
import os, sys, torch, torch.distributed as dist
sys.path[:0] = [{root!r}, {pkg!r}]
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(rank)
dist.init_process_group("nccl", device_id=torch.device("cuda", rank))      # "nccl" is RCCL on ROCm
from unidistill_amd import train
torch.manual_seed(0)
dev = torch.device("cuda", rank)
tr = train.Trainer(train.DetectStep("camera"), device=dev, optimizer="hip", channels_last=True)
assert tr.ddp is not None, "the step is not wrapped in DDP"
batch = train.synthetic_batch(dev, 1, rank=rank, ncam=1, with_points=False)
counts = []
for _ in range(4):
    out = tr.step(batch)
    counts.append((tr.opt.grad_uploads, tr.opt.table_builds))
assert torch.isfinite(out["loss"])
print("OPTIM_DDP_COUNTS", rank, counts, flush=True)
assert float(tr.opt.skipped) == 0 and float(tr.opt.steps_done) == 4
# bucket views: the chunk table is built once and the gradient pointers are sent once per set of buckets, then reused.
# DDP lays its buckets out a second time before the second backward (its one-time rebuild in gradient-arrival order), which
# moves every bucket view once: that is the only re-send allowed, and from then on nothing is sent.
assert all(c[1] == 1 for c in counts), counts
assert counts[0][0] == 1 and counts[1][0] <= 2 and counts[2] == counts[1] and counts[3] == counts[1], counts
flat = torch.cat([p.detach().flatten() for p in tr.params])
other = flat.clone()
dist.broadcast(other, 0)
assert torch.equal(flat, other), "ranks diverged"
dist.barrier(); dist.destroy_process_group()
print("OPTIM_DDP_OK", rank)
'''


def _run_ddp(tmp_path, nproc, port, extra_env):
    path = tmp_path / "optim_ddp.py"
    path.write_text(_DDP_SCRIPT.format(root=ROOT, pkg=PKG))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", UD_RANDOM_INIT="1", **extra_env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(path)]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.count("OPTIM_DDP_OK") == nproc, res.stdout[-1500:] + res.stderr[-3000:]


def test_one_rank_ddp_reuses_the_gradient_table(hip_lib, tmp_path):
    """UD_FORCE_DDP=1 on one rank: the gradients are DDP's bucket views."""
    _run_ddp(tmp_path, 1, 29541, {"UD_FORCE_DDP": "1"})


def test_two_rank_ddp_reuses_the_gradient_table(hip_lib, tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs (RCCL refuses two ranks on one device)")
    _run_ddp(tmp_path, 2, 29543, {})
