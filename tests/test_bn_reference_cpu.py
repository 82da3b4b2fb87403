"""The float64 BatchNorm reference of tests/bn_reference.py (used by the GPU tests of csrc/bn_act.hip) on the CPU: it equals torch's
BatchNorm + autograd in float64, its conditioning holds what it promises, and its per-element bounds reject subtly wrong
results -- a kernel that made any of these mistakes would fail the GPU assertions, not only a grossly wrong one."""
import pytest
import torch
import torch.nn.functional as F

import bn_reference as R

EPS, MOM = 1e-3, 0.1


def _case(P, C, dtype, residual, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(P, C, generator=g, dtype=torch.float64) * 2 + 0.5).to(dtype)
    r = torch.randn(P, C, generator=g, dtype=torch.float64).to(dtype) if residual else None
    dy = torch.randn(P, C, generator=g, dtype=torch.float64).to(dtype)
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    gamma[::3] *= -1                                                   # negative scales too
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    rm = torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    rv = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    return x, r, dy, gamma.float(), beta.float(), rm.float(), rv.float()


@pytest.mark.parametrize("dims", [2, 4])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_reference_equals_torch_batchnorm_in_float64(dims, residual, relu):
    B, C, H, W = 3, 32, 5, 7
    P = B * H * W
    x, r, dy, gamma, beta, rm, rv = _case(P, C, torch.float64, residual, 11 + dims)
    ref = R.reference(x, gamma, beta, EPS, r, relu, dy, MOM, rm, rv)
    BN = torch.nn.BatchNorm2d if dims == 4 else torch.nn.BatchNorm1d
    bn = BN(C, eps=EPS, momentum=MOM).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    to_t = (lambda t: t.view(B, H, W, C).permute(0, 3, 1, 2)) if dims == 4 else (lambda t: t)
    rows = (lambda t: t.permute(0, 2, 3, 1).reshape(P, C)) if dims == 4 else (lambda t: t)
    xt = to_t(x).clone().requires_grad_(True)
    rt = to_t(r).clone().requires_grad_(True) if residual else None
    yt = bn(xt)
    if residual:
        yt = yt + rt
    if relu:
        yt = F.relu(yt)
    yt.backward(to_t(dy))
    close = lambda a, b: torch.testing.assert_close(a.double(), b.double(), rtol=0, atol=1e-12)
    close(ref["y"], rows(yt.detach()))
    close(ref["dx"], rows(xt.grad))
    if residual:
        close(ref["dres"], rows(rt.grad))
    close(ref["dgamma"], bn.weight.grad)
    close(ref["dbeta"], bn.bias.grad)
    close(ref["running_mean"], bn.running_mean)
    close(ref["running_var"], bn.running_var)
    close(ref["mean"], x.mean(0))
    close(ref["var"], x.var(0, unbiased=False))
    # the kernels' folded form: dx = scale * dr + k2 * x + k0
    close(ref["dx"], ref["scale"] * ref["dr"] + ref["k2"] * x + ref["k0"])
    # eval mode
    bn.eval()
    with torch.no_grad():
        ye = bn(to_t(x))
        if residual:
            ye = ye + to_t(r)
        if relu:
            ye = F.relu(ye)
    close(R.reference(x, gamma, beta, EPS, r, relu, training=False, running_mean=bn.running_mean,
                      running_var=bn.running_var)["y"], rows(ye))


def test_reference_rejects_one_value_per_channel():
    with pytest.raises(ValueError):
        R.reference(torch.ones(1, 16), torch.ones(16), torch.zeros(16), EPS)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("residual", [False, True])
def test_conditioning_holds_its_margin(dtype, residual):
    P, C = 4000, 48
    x, r, _, gamma, beta, _, _ = _case(P, C, dtype, residual, 5)
    # plant elements right on the threshold: x = mean - beta / scale (z = 0 before rounding)
    mean, var = R.batch_stats(x)
    sc = gamma.double() / torch.sqrt(var + EPS)
    zero_at = (mean - beta.double() / sc).to(dtype)
    x[::97, ::5] = zero_at.expand(P, C)[::97, ::5]
    z0 = R.reference(x, gamma, beta, EPS, r, relu=False)["z"]
    assert float(z0.abs().min()) < R.MARGIN
    xc, zmin, moved = R.condition(x, gamma, beta, EPS, r)
    z = R.reference(xc, gamma, beta, EPS, r, relu=False)["z"]
    assert xc.dtype == dtype and xc.shape == x.shape
    assert zmin >= R.MARGIN and float(z.abs().min()) == zmin
    assert 0 < moved <= int((z0.abs() < 4 * R.MARGIN).sum())    # only elements near the threshold moved
    assert int((xc != x).sum()) == moved


@pytest.mark.parametrize("P,C,dtype", [(777, 32, torch.float32), (4000, 16, torch.float32), (777, 32, torch.bfloat16),
                                       (3000, 64, torch.bfloat16)])
def test_bounds_accept_the_rounded_reference_and_reject_each_mutation(P, C, dtype):
    """The per-element bounds admit the float64 result rounded to the kernel's output types, and reject each of: statistics
    over P minus one reduction slice of rows; one ReLU-mask element flipped at |pre-activation| >= MARGIN; the biased instead of
    the unbiased running variance; eps omitted; k0 taken from the neighbouring channel."""
    x, _, dy, gamma, beta, rm, rv = _case(P, C, dtype, False, P + C)
    x, zmin, _ = R.condition(x, gamma, beta, EPS)
    assert zmin >= R.MARGIN
    ref = R.reference(x, gamma, beta, EPS, None, True, dy, MOM, rm, rv)
    bnd = R.bounds(x, ref, dtype, EPS, None, MOM, rm, rv)
    assert float((bnd["z"]).max()) < R.MARGIN           # the margin exceeds any legitimate disagreement on z
    names = ["y", "dx", "dres", "dgamma", "dbeta", "mean", "var", "invstd", "running_mean", "running_var"]

    def rounded(d):
        out = {k: v.float().double() for k, v in d.items()}
        for k in ("y", "dx", "dres"):
            out[k] = d[k].to(dtype).double()
        return out

    assert R.violations(rounded(ref), ref, bnd, names) == []

    def mutated(**kw):
        got = rounded(ref)
        got.update({k: v.double() for k, v in kw.items()})
        return R.violations(got, ref, bnd, names)

    # statistics over P minus one slice of rows (k_bn_stats_partial dropping one workgroup's rows)
    rows = R.geometry(P, C)["lanes"] * R.geometry(P, C)["rows_per_lane"]
    assert rows < P
    m1, v1 = R.batch_stats(x[: P - rows])
    bad = R.from_stats(x, m1, v1, gamma, beta, EPS, None, True, dy)
    msgs = mutated(y=bad["y"].to(dtype), dx=bad["dx"].to(dtype), mean=bad["mean"], var=bad["var"], invstd=bad["invstd"])
    assert any(m.startswith("mean") for m in msgs) and any(m.startswith("dx") for m in msgs), msgs
    # one ReLU-mask element flipped where |z| >= MARGIN (the positive element closest to the threshold)
    z = ref["z"]
    zpos = torch.where(z > 0, z, torch.full_like(z, float("inf")))
    i = int(zpos.argmin())
    mask = z > 0
    mask.view(-1)[i] = False
    assert float(z.view(-1)[i]) >= R.MARGIN
    bad = R.from_stats(x, ref["mean"], ref["var"], gamma, beta, EPS, None, True, dy, mask=mask)
    msgs = mutated(dx=bad["dx"].to(dtype), dgamma=bad["dgamma"].float(), dbeta=bad["dbeta"].float(), dres=bad["dres"].to(dtype))
    assert {m.split(":")[0] for m in msgs} >= {"dx", "dres", "dbeta"}, msgs
    # biased running variance
    msgs = mutated(running_var=(1 - MOM) * rv.double() + MOM * ref["var"])
    assert [m.split(":")[0] for m in msgs] == ["running_var"], msgs
    # eps omitted
    bad = R.from_stats(x, ref["mean"], ref["var"], gamma, beta, 0.0, None, True, dy)
    msgs = mutated(invstd=bad["invstd"].float(), dx=bad["dx"].to(dtype))
    assert any(m.startswith("invstd") for m in msgs), msgs
    # k0 taken from the neighbouring channel
    dx = ref["scale"] * ref["dr"] + ref["k2"] * x.double() + torch.roll(ref["k0"], 1)
    msgs = mutated(dx=dx.to(dtype))
    assert [m.split(":")[0] for m in msgs] == ["dx"], msgs


def test_bf16_forward_rule():
    """bf16 y: the float64 value rounded to bf16, or where the value sits within the z bound of a rounding boundary, either
    neighbour; anything else (a second ulp, or a different value away from a boundary) is an error."""
    v = torch.tensor([1.0, 1.0 + 2 ** -8, 1.0 + 2 ** -8 + 1e-9, 3.0, -0.0], dtype=torch.float64)
    dz = torch.full_like(v, 1e-6)
    exact = v.float().bfloat16()
    mism, amb, bad = R.bf16_forward_mismatches(exact, v, dz)
    assert not bool(bad.any()) and not bool(mism.any())
    assert amb.tolist() == [False, True, True, False, False]
    up = torch.tensor([1.0, 1.0 + 2 ** -7, 1.0 + 2 ** -7, 3.0 + 2 ** -6, 0.0], dtype=torch.float64).bfloat16()
    mism, amb, bad = R.bf16_forward_mismatches(up, v, dz)
    assert mism.tolist() == [False, True, True, True, False] and bad.tolist() == [False, False, False, True, False]


def test_geometry_mirrors_the_launch_arithmetic():
    g = R.geometry(159997, 16)
    assert (g["gw"], g["slices"], g["capped"], g["final_t"], g["bwd_unrolled"]) == (16, 1024, True, 256, True)
    g = R.geometry(270336, 64)
    assert g["trips"] == 3 and g["slices"] == 1024 and g["capped"]
    g = R.geometry(5, 48)
    assert (g["gw"], g["slices"], g["final_t"], g["pow2_chunks"]) == (16, 1, 64, False)
