"""Backward through FROZEN BatchNorm statistics (ud_bn_act_bwd_frozen_ld*: an eval-mode BatchNorm inside a training graph) against
the float64 restatement of tests/bn_reference.py evaluated on the running buffers.

The cases are drawn and conditioned on the CPU (cases()), so tests/test_bn_frozen_cases_cpu.py can check without a GPU that every
one of them keeps its pre-activations at least bn_reference.MARGIN away from the ReLU threshold.  The bounds are the factors of the
reference's max-abs that tests/test_bn_act_gpu.py uses for the same quantities in training mode (bf16: test_bn_act_training, fp32:
test_bn_act_fp32_mode); eval-mode arithmetic is a strict subset of what they cover."""
import numpy as np
import pytest
import torch

import bn_reference as R

EPS = 1e-3
MAPS = [(2, 64, 9, 13), (3, 128, 16, 20), (1, 256, 5, 7)]       # odd pixel counts, the three channel-group widths
ROWS = [(777, 32), (5, 48), (1000, 16)]
SHAPES = MAPS + ROWS + [(1, 16, 1, 1)]                          # P == 1: eval mode has no "more than 1 value per channel" rule
VARIANTS = [(False, True), (True, True), (True, False), (False, False)]      # (residual, relu)
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}
# factors of max|reference|: y / dres, dx, dgamma / dbeta
FACTORS = {torch.bfloat16: (8e-3, 2e-2, 1e-2), torch.float32: (2e-5, 1e-4, 1e-4)}


def _pc(shape):
    return (shape[0], shape[1]) if len(shape) == 2 else (shape[0] * shape[2] * shape[3], shape[1])


def condition_eval(x, rm, rv, gamma, beta, eps, residual=None, margin=R.MARGIN, max_iter=10):
    """bn_reference.condition for FIXED statistics: that function recomputes the batch statistics of x, which an eval-mode
    BatchNorm does not use (and which do not exist for one row).  Same rule: nudge the elements whose float64 pre-activation lies
    within `margin` of the ReLU threshold by 2 * margin / |dz/dx| (at least one ulp of x's dtype), round, repeat.
    -> (x', min |z|, number of elements moved)."""
    dt, orig = x.dtype, x
    mean, var = rm.double(), rv.double()
    gain = (gamma.double() / torch.sqrt(var + eps)).expand_as(x)
    for _ in range(max_iter):
        z = R.from_stats(x, mean, var, gamma, beta, eps, residual, relu=False)["z"]
        near = z.abs() < margin
        if not bool(near.any()):
            break
        side = torch.where(z >= 0, torch.ones_like(z), -torch.ones_like(z))
        step = side * torch.sign(gain) * torch.maximum(2 * margin / gain.abs(), R.ulp(x, dt))
        x = torch.where(near, (x.double() + step).to(dt), x)
    zmin = float(R.from_stats(x, mean, var, gamma, beta, eps, residual, relu=False)["z"].abs().min())
    return x, zmin, int((x != orig).sum())


def draw(shape, dtype, residual, relu):
    """Seeded case on the CPU, rows [P, C] in the kernel dtype; running mean / variance away from 0 / 1 (test_bn_act_eval)."""
    P, C = _pc(shape)
    g = torch.Generator().manual_seed(P * 7 + C + 1000 * residual + 10 * relu + (dtype == torch.float32))
    x = (torch.randn(P, C, generator=g) * 2 + 0.5).to(dtype)
    r = torch.randn(P, C, generator=g).to(dtype) if residual else None
    dy = torch.randn(P, C, generator=g).to(dtype)
    gamma = torch.empty(C).uniform_(0.5, 1.5, generator=g)
    gamma[1::5] *= -1
    beta = torch.empty(C).normal_(0, 0.3, generator=g)
    rm = torch.empty(C).normal_(0, 0.5, generator=g)
    rv = torch.empty(C).uniform_(0.5, 2, generator=g)
    zmin = None
    if relu:
        x, zmin, _ = condition_eval(x, rm, rv, gamma, beta, EPS, r)
    return dict(x=x, r=r, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv, zmin=zmin)


def cases():
    for shape in SHAPES:
        for dtype in DTYPES.values():
            for residual, relu in VARIANTS:
                yield shape, dtype, residual, relu


def reference(case, relu):
    """float64: y, dr (= dres), dgamma, dbeta from bn_reference.from_stats on the running buffers; dx = scale * dr (the
    statistics are constants: the batch terms k2 * x + k0 of the training-mode dx are absent)."""
    ref = R.from_stats(case["x"], case["rm"].double(), case["rv"].double(), case["gamma"], case["beta"], EPS, case["r"], relu,
                       case["dy"])
    ref["dx"] = ref["scale"] * ref["dr"]
    return ref


def _to_op(rows, shape):
    if len(shape) == 2:
        return rows
    B, C, H, W = shape
    return rows.view(B, H, W, C).permute(0, 3, 1, 2)


def _rows(t):
    return t if t.dim() == 2 else t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _bn(shape, case, affine_grad):
    C = _pc(shape)[1]
    bn = (torch.nn.BatchNorm2d if len(shape) == 4 else torch.nn.BatchNorm1d)(C, eps=EPS, momentum=0.01).cuda()
    with torch.no_grad():
        bn.weight.copy_(case["gamma"]); bn.bias.copy_(case["beta"])
        bn.running_mean.copy_(case["rm"]); bn.running_var.copy_(case["rv"])
    bn.weight.requires_grad_(affine_grad); bn.bias.requires_grad_(affine_grad)
    return bn.eval()


class _Spy:
    """Records the (dgamma, dbeta) pointer arguments of the frozen-statistics entry points."""

    def __init__(self, monkeypatch):
        from unidistill_amd import _lib
        _lib.load()
        self.calls = []
        for name in ("ud_bn_act_bwd_frozen_ld", "ud_bn_act_bwd_frozen_ld_f32"):
            real = getattr(_lib.ud, name)
            monkeypatch.setattr(_lib.ud, name, self._wrap(name, real))

    def _wrap(self, name, real):
        def call(*a):
            self.calls.append((name, a[10], a[11]))
            return real(*a)
        return call


def _run(shape, case, relu, affine_grad, mode="plain"):
    """ops/bn_act.bn_act on an eval-mode BatchNorm, forward + backward.  mode "slice": the output concatenated with another map
    by torch.cat, whose backward hands over a strided channel slice (dy_ld > C); "out": written into a cat_buffer slot."""
    from unidistill_amd.ops import bn_act as hb
    bn = _bn(shape, case, affine_grad)
    before = [t.clone() for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    versions = [t._version for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    xd = _to_op(case["x"].cuda(), shape).detach().requires_grad_(True)
    rd = _to_op(case["r"].cuda(), shape).detach().requires_grad_(True) if case["r"] is not None else None
    dy = _to_op(case["dy"].cuda(), shape)
    if mode == "plain":
        y = hb.bn_act(bn, xd, rd, relu)
        y.backward(dy if dy.dim() == 2 else dy.contiguous(memory_format=torch.channels_last))
    else:
        B, C, H, W = shape
        extra = 32
        gfull = torch.zeros(B, C + extra, H, W, dtype=dy.dtype, device="cuda").contiguous(memory_format=torch.channels_last)
        gfull[:, :C] = dy
        if mode == "out":
            buf, slots = hb.cat_buffer(xd, [C, extra])
            slots[1].zero_()
            y = hb.bn_act(bn, xd, rd, relu, out=slots[0])
            assert y.data_ptr() == slots[0].data_ptr() and y.stride()[3] == C + extra
            hb.cat_slices(buf, [y, slots[1]]).backward(gfull)
        else:
            y = hb.bn_act(bn, xd, rd, relu)
            other = torch.zeros(B, extra, H, W, dtype=dy.dtype, device="cuda").contiguous(memory_format=torch.channels_last)
            real, copies = hb._like, []
            hb._like = lambda t, ref: (copies.append(tuple(t.shape)) if t.stride() != ref.stride() else None, real(t, ref))[1]
            try:
                torch.cat([y, other], 1).backward(gfull)
            finally:
                hb._like = real
            assert not copies, f"the strided gradient slice was copied: {copies}"
    torch.cuda.synchronize()
    for t, b, v in zip((bn.running_mean, bn.running_var, bn.num_batches_tracked), before, versions):
        assert torch.equal(t, b) and t._version == v, "eval mode touched a running buffer"
    got = dict(y=_rows(y.detach()).clone(), dx=_rows(xd.grad).clone(), dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    if rd is not None:
        got["dres"] = _rows(rd.grad).clone()
    return got


def _close(a, b, f, name):
    print(f"  {name}: max |err| {float((a.detach().double().cpu() - b.double()).abs().max()):.3e}, "
          f"bound {f * float(b.abs().max()) + 1e-6:.3e}")
    np.testing.assert_allclose(a.detach().double().cpu().numpy(), b.double().numpy(), rtol=0,
                               atol=f * float(b.abs().max()) + 1e-6, err_msg=name)


def _check(case, relu, dtype, got, affine_grad):
    ref = reference(case, relu)
    fy, fdx, fsum = FACTORS[dtype]
    _close(got["y"], ref["y"], fy, "y")
    _close(got["dx"], ref["dx"], fdx, "dx")
    if case["r"] is not None:
        _close(got["dres"], ref["dres"], fy, "dres")
    if affine_grad:
        _close(got["dgamma"], ref["dgamma"], fsum, "dgamma")
        _close(got["dbeta"], ref["dbeta"], fsum, "dbeta")
    else:
        assert got["dgamma"] is None and got["dbeta"] is None


_IDS = dict(argnames="residual,relu", argvalues=VARIANTS, ids=["relu", "res-relu", "res", "plain"])


@pytest.mark.gpu
@pytest.mark.parametrize("affine_grad", [True, False], ids=["affine", "frozen-affine"])
@pytest.mark.parametrize(**_IDS)
@pytest.mark.parametrize("dtype", list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_frozen_bn_backward_vs_float64(hip_lib, monkeypatch, shape, dtype, residual, relu, affine_grad):
    """y, dx, dres (and dgamma, dbeta with trainable affine parameters) against float64; the running buffers and their version
    counters untouched; with frozen affine parameters the entry point gets NULL sum pointers (the one-launch form) and
    bn.weight.grad stays None."""
    case = draw(shape, dtype, residual, relu)
    if relu:
        assert case["zmin"] >= R.MARGIN, case["zmin"]
    spy = _Spy(monkeypatch)
    got = _run(shape, case, relu, affine_grad)
    assert len(spy.calls) == 1 and spy.calls[0][0] == ("ud_bn_act_bwd_frozen_ld_f32" if dtype == torch.float32
                                                     else "ud_bn_act_bwd_frozen_ld")
    _, dg, db = spy.calls[0]
    assert (dg is not None and db is not None and dg != 0 and db != 0) if affine_grad else (dg is None and db is None)
    _check(case, relu, dtype, got, affine_grad)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["slice", "out"])
@pytest.mark.parametrize("affine_grad", [True, False], ids=["affine", "frozen-affine"])
@pytest.mark.parametrize("residual,relu", [(False, True), (True, True), (True, False)], ids=["relu", "res-relu", "res"])
@pytest.mark.parametrize("dtype", list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize("shape", [(2, 64, 9, 13), (1, 256, 5, 7)], ids=["2x64x9x13", "1x256x5x7"])
def test_frozen_bn_backward_strided_views(hip_lib, shape, dtype, residual, relu, affine_grad, mode):
    """dy as a channel slice of a wider channels-last map (ld = C + 32, what a concatenation's backward hands over: read in
    place, no copy) and out= into a cat_buffer slot (the saved output, the mask source with a residual, is strided then)."""
    case = draw(shape, dtype, residual, relu)
    _check(case, relu, dtype, _run(shape, case, relu, affine_grad, mode), affine_grad)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize("shape", [(3, 128, 16, 20), (1000, 16), (1, 16, 1, 1)], ids=["3x128x16x20", "1000x16", "1x16x1x1"])
def test_frozen_bn_backward_is_bitwise_reproducible(hip_lib, shape, dtype):
    """Two runs of the trainable-affine case: dx, dgamma, dbeta bit-identical (per-slice partial sums + a fixed-order finalize)."""
    case = draw(shape, dtype, True, True)
    a, b = _run(shape, case, True, True), _run(shape, case, True, True)
    for k in ("y", "dx", "dres", "dgamma", "dbeta"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_frozen_entry_point_argument_checks(hip_lib):
    """One of the two sum pointers alone, or sums without mean / invstd / workspace, is refused before any launch."""
    from unidistill_amd import _lib
    lib = _lib.load()
    P, C = 64, 32
    x, dy = torch.randn(P, C, device="cuda"), torch.randn(P, C, device="cuda")
    dx = torch.full((P, C), 7.0, device="cuda")
    v = torch.ones(C, device="cuda")
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    ws = torch.empty(lib.ud_bn_act_workspace_bytes(C), dtype=torch.uint8, device="cuda")
    s, p = _lib.stream_of(x), lambda t: t.data_ptr()
    f = lib.ud_bn_act_bwd_frozen_ld_f32
    assert f(p(x), None, p(dy), C, p(v), p(v), p(v), p(v), p(dx), None, p(dg), None, P, C, 1, p(ws), ws.numel(), s) != 0
    assert f(p(x), None, p(dy), C, p(v), p(v), None, p(v), p(dx), None, p(dg), p(db), P, C, 1, p(ws), ws.numel(), s) != 0
    assert f(p(x), None, p(dy), C, p(v), p(v), p(v), p(v), p(dx), None, p(dg), p(db), P, C, 1, None, 0, s) != 0
    assert f(p(x), None, p(dy), 16, p(v), p(v), None, None, p(dx), None, None, None, P, C, 1, None, 0, s) != 0     # ld < C
    assert f(p(x), None, p(dy), C, p(v), p(v), None, None, p(dx), None, None, None, P, 24, 1, None, 0, s) != 0     # C % 16
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all())
    assert f(p(x), None, p(dy), C, p(v), p(v), None, None, p(dx), None, None, None, P, C, 1, None, 0, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx, torch.where(x + 1 > 0, dy, torch.zeros_like(dy)))
