"""The BatchNorm kernels of csrc/bn_act.hip (ud_bn_stats*, ud_bn_act_fwd*, ud_bn_act_bwd*, ud_bn_stats_from_partials) against the
float64 reference of tests/bn_reference.py, at the network's own sizes and at the edges of every launch path, with per-element
bounds derived from the kernels' arithmetic.  Inputs are seeded per case and conditioned off the ReLU threshold, so a failure
replays and every element it reports is a kernel error, not a knife-edge rounding of the mask."""
import pytest
import torch

import bn_reference as R

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-3, 0.01           # the sparse / dense blocks' BatchNorm settings (spconv_backbone.py, base_bev_backbone.py)
# bf16 forward: y is the float64 value rounded to bf16; it may differ (by one ulp) only where the float64 value lies within the
# z bound of a rounding boundary, and only on a small fraction of the elements: the kernel's actual z error (fp32 statistics,
# ~sqrt(n) u of the terms T = |x scale| + |shift| + |r| for n <= 140 adds, plus the fma's rounding: ~4e-6 T) crosses a boundary
# with probability ~2 * 4e-6 T / (2^-8 |z|) = 2e-3 T/|z|; T/|z| <= 4 on all but a tail -> 2^-7.
MISMATCH_FRAC = 2.0 ** -7

# shape, the bn_act.hip launch path it reaches (asserted against bn_reference.geometry, which mirrors slices_for / stream_grid)
SHAPES = [
    # [M, C] sparse voxel rows (spconv_backbone.py, config.py max_voxels 120-160 k)
    ((159997, 16), dict(gw=16, slices=1024, capped=True, final_t=256, bwd_unrolled=True)),    # cap 1024 reached, _final<256> 4-load loop
    ((61441, 32), dict(gw=32, slices=961, capped=False, final_t=256, bwd_unrolled=True)),     # slices > 768 below the cap
    ((20011, 64), dict(gw=64, slices=626, final_t=256, bwd_unrolled=False)),                  # slices 129-768: _final<256>, 1-load loop
    ((7333, 128), dict(gw=64, slices=230, final_t=256, stats_unrolled=True)),                 # 2 channel groups, stats 4-load loop
    ((600001, 16), dict(gw=16, slices=1024, capped=True, trips=2)),                           # gw 16 with a second grid-stride trip
    # channels-last maps
    ((24, 64, 64, 176), dict(gw=64, slices=1024, capped=True, trips=3)),                      # ResNet layer1 (P = 270 336), 3 trips
    ((24, 256, 64, 176), dict(gw=64, slices=512, final_t=256, trips=9)),                      # ResNet layer1 wide: 9 trips
    ((24, 2048, 8, 22), dict(gw=64, slices=64, final_t=64, stats_unrolled=True, trips=2)),    # layer4: _final<64>, 32 groups
    ((4, 128, 180, 180), dict(gw=64, slices=1024, capped=False, bwd_unrolled=True, trips=2)), # BEV trunk 180^2
    ((4, 256, 90, 90), dict(gw=64, slices=512, trips=1)),                                     # BEV trunk 90^2
    ((24, 512, 16, 44), dict(gw=64, slices=256, trips=2)),                                    # depth net
    # small edges
    ((1000, 16), dict(gw=16, slices=8, final_t=64, stats_unrolled=False)),                    # the round-6 voxel-row cases
    ((777, 32), dict(gw=32, slices=13, final_t=64)),
    ((300, 128), dict(gw=64, slices=10, final_t=64)),
    ((100, 16), dict(gw=16, slices=1, final_t=64)),                                           # P < one workgroup's 128 lanes
    ((2, 32), dict(gw=32, slices=1)),                                                         # P = 2
    ((2, 64), dict(gw=64, slices=1)),
    ((5, 48), dict(gw=16, slices=1, pow2_chunks=False)),                                      # C = 48: C/8 = 6 chunks
    ((3, 48, 5, 7), dict(gw=16, pow2_chunks=False)),                                          # B*H*W = 105, not a multiple of 8
    ((1, 2688, 6, 7), dict(gw=64, slices=2, pow2_chunks=False)),                              # C = 2688: 336 chunks, 2 column blocks
]
VARIANTS = [(False, True), (True, True), (True, False), (False, False)]      # (residual, relu)


def _pc(shape):
    return (shape[0], shape[1]) if len(shape) == 2 else (shape[0] * shape[2] * shape[3], shape[1])


def _to_op(rows, shape):
    """rows [P, C] -> the tensor the op takes: [M, C] rows or a channels-last [B, C, H, W] map over the same memory."""
    if len(shape) == 2:
        return rows
    B, C, H, W = shape
    return rows.view(B, H, W, C).permute(0, 3, 1, 2)


def _rows(t):
    return t if t.dim() == 2 else t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _draw(shape, dtype, residual, seed, relu=True):
    """Seeded case on the device: x, residual, dy in the kernel dtype (rows [P, C]), gamma / beta / running buffers in fp32; x
    conditioned off the ReLU threshold when a ReLU follows."""
    P, C = _pc(shape)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = (torch.randn(P, C, generator=g, device="cuda") * 2 + 0.5).to(dtype)
    r = torch.randn(P, C, generator=g, device="cuda").to(dtype) if residual else None
    dy = torch.randn(P, C, generator=g, device="cuda").to(dtype)
    gamma = torch.rand(C, generator=g, device="cuda") + 0.5
    gamma[1::5] *= -1
    beta = torch.randn(C, generator=g, device="cuda") * 0.3
    rm = torch.randn(C, generator=g, device="cuda") * 0.1
    rv = torch.rand(C, generator=g, device="cuda") + 0.5
    moved, zmin, margin = 0, None, R.MARGIN
    if relu:
        x0 = x
        x, zmin, _ = R.condition(x, gamma, beta, EPS, r, margin)
        # the margin must exceed the bound on the kernel's z; a channel of a few rows with a tiny variance (P = 5) has
        # invstd ~ eps^-1/2 and a larger bound: condition again with twice that bound
        dz = float(R.bounds(x, R.reference(x, gamma, beta, EPS, r, relu=True), dtype, EPS, r)["z"].max())
        if dz >= margin:
            margin = 2 * dz
            x, zmin, _ = R.condition(x, gamma, beta, EPS, r, margin)
        assert zmin >= margin, (zmin, margin)
        moved = int((x != x0).sum())
    return dict(x=x, r=r, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv, moved=moved, zmin=zmin, margin=margin)


def _bn(shape, case, training=True):
    C = _pc(shape)[1]
    bn = (torch.nn.BatchNorm2d if len(shape) == 4 else torch.nn.BatchNorm1d)(C, eps=EPS, momentum=MOM).cuda()
    with torch.no_grad():
        bn.weight.copy_(case["gamma"]); bn.bias.copy_(case["beta"])
        bn.running_mean.copy_(case["rm"]); bn.running_var.copy_(case["rv"])
    return bn.train(training)


def _run(shape, case, relu, ld_extra=0):
    """ops/bn_act.bn_act forward + backward; ld_extra > 0: y written into a channel slice of a [B, C + ld_extra, H, W]
    concatenation (ud_bn_act_fwd_ld, y_ld > C) and the gradient read in place from the concatenation's (dy_ld > C)."""
    from unidistill_amd.ops import bn_act as hb
    bn = _bn(shape, case)
    xd = _to_op(case["x"].clone(), shape).detach().requires_grad_(True)
    rd = _to_op(case["r"].clone(), shape).detach().requires_grad_(True) if case["r"] is not None else None
    dy = _to_op(case["dy"], shape)
    if ld_extra:
        B, C, H, W = shape
        buf, slots = hb.cat_buffer(xd, [C, ld_extra])
        slots[1].zero_()
        y = hb.bn_act(bn, xd, rd, relu, out=slots[0])
        assert y.data_ptr() == slots[0].data_ptr() and y.stride()[3] == C + ld_extra
        cat = hb.cat_slices(buf, [y, slots[1]])
        gfull = torch.zeros(B, C + ld_extra, H, W, dtype=dy.dtype, device="cuda").contiguous(memory_format=torch.channels_last)
        gfull[:, :C] = dy
        cat.backward(gfull)
    else:
        y = hb.bn_act(bn, xd, rd, relu)
        y.backward(dy if dy.dim() == 2 else dy.contiguous(memory_format=torch.channels_last))
    got = dict(y=_rows(y.detach()), dx=_rows(xd.grad), dgamma=bn.weight.grad, dbeta=bn.bias.grad,
               running_mean=bn.running_mean, running_var=bn.running_var)
    if rd is not None:
        got["dres"] = _rows(rd.grad)
    assert int(bn.num_batches_tracked) == 1
    return {k: v.clone() for k, v in got.items()}


def _check(shape, dtype, case, relu, got, tag=""):
    x, r = case["x"], case["r"]
    ref = R.reference(x, case["gamma"], case["beta"], EPS, r, relu, case["dy"], MOM, case["rm"], case["rv"])
    bnd = R.bounds(x, ref, dtype, EPS, r, MOM, case["rm"], case["rv"])
    if relu:
        # no legitimate disagreement on z reaches the conditioning margin: a mask difference would be a kernel error
        assert float(bnd["z"].max()) < case["margin"], (float(bnd["z"].max()), case["margin"])
    names = ["y", "dx", "dgamma", "dbeta", "running_mean", "running_var"] + (["dres"] if r is not None else [])
    msgs = R.violations(got, ref, bnd, names)
    if dtype == torch.bfloat16:
        mism, amb, bad = R.bf16_forward_mismatches(got["y"], ref["y"], bnd["z"])
        if bool(bad.any()):
            lines = [f"  {tuple(i)}: z={float(ref['z'][tuple(i)]):+.9e} got={float(got['y'][tuple(i)]):+.9e} "
                     f"rounded ref={float(ref['y'][tuple(i)].float().bfloat16()):+.9e} z bound={float(bnd['z'][tuple(i)]):.3e}"
                     for i in bad.nonzero()[:8].tolist()]
            msgs.append(f"y (bf16 rule): {int(bad.sum())} elements differ from the rounded float64 value away from a rounding "
                        f"boundary or by more than one ulp\n" + "\n".join(lines))
        frac = float(mism.double().mean())
        if frac > MISMATCH_FRAC:
            msgs.append(f"y (bf16 rule): {frac:.2e} of the elements differ from the rounded float64 value > {MISMATCH_FRAC:.2e}")
    assert not msgs, f"{tag} shape {shape} {dtype} relu={relu} residual={r is not None}\n" + "\n".join(msgs)
    return ref, bnd


@pytest.mark.parametrize("residual,relu", VARIANTS, ids=["relu", "res-relu", "res", "plain"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,path", SHAPES, ids=["x".join(map(str, s)) for s, _ in SHAPES])
def test_bn_act_vs_float64(hip_lib, shape, path, dtype, residual, relu):
    """y, dx, dres, dgamma, dbeta and the running buffers within their per-element bounds; the HIP kernels ran (profiling
    counters); a second call on the same inputs is bitwise equal."""
    from unidistill_amd import _lib
    P, C = _pc(shape)
    geo = R.geometry(P, C)
    assert {k: geo[k] for k in path} == path, geo
    case = _draw(shape, dtype, residual, seed=P * 7 + C + 1000 * residual + 10 * relu, relu=relu)
    names = ("bn_act.stats", "bn_act.k_fwd", "bn_act.k_bwd_reduce", "bn_act.k_bwd_dx")
    for n in names:
        _lib.prof_read(n, reset=True)
    _lib.prof_enable(True)
    try:
        got = _run(shape, case, relu)
        torch.cuda.synchronize()
    finally:
        _lib.prof_enable(False)
    assert [_lib.prof_read(n)[1] for n in names] == [1, 1, 1, 1]
    _check(shape, dtype, case, relu, got)
    again = _run(shape, case, relu)
    for k in ("y", "dx", "dgamma", "dbeta"):
        assert torch.equal(got[k], again[k]), f"{k} differs between two calls on the same inputs"


@pytest.mark.parametrize("residual,relu", VARIANTS, ids=["relu", "res-relu", "res", "plain"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(4, 128, 180, 180), (2, 64, 9, 13), (3, 48, 5, 7)])
def test_bn_act_into_a_wider_map_vs_float64(hip_lib, shape, dtype, residual, relu):
    """The _ld entry points: y written as a channel slice of a wider map (y_ld = C + 32), the gradient read in place from the
    concatenation's (dy_ld = C + 32), with and without a residual (the saved output is the mask source then)."""
    P, C = _pc(shape)
    case = _draw(shape, dtype, residual, seed=P + C + 3, relu=relu)
    _check(shape, dtype, case, relu, _run(shape, case, relu, ld_extra=32), "ld")


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(24, 64, 64, 176), (159997, 16), (5, 48), (2, 2688, 3, 5)])
def test_bn_act_eval_vs_float64(hip_lib, shape, dtype, residual):
    """Eval mode: the running buffers folded in fp32 (bn_act.batch_stats) + ud_bn_act_fwd*, against float64."""
    from unidistill_amd.ops import bn_act as hb
    P, C = _pc(shape)
    case = _draw(shape, dtype, residual, seed=P + C + 11, relu=False)
    bn = _bn(shape, case, training=False)
    with torch.no_grad():
        y = hb.bn_act(bn, _to_op(case["x"], shape), None if case["r"] is None else _to_op(case["r"], shape), True)
    x, r = case["x"], case["r"]
    ref = R.reference(x, case["gamma"], case["beta"], EPS, r, True, training=False, running_mean=case["rm"],
                      running_var=case["rv"])
    bnd = R.bounds(x, ref, dtype, EPS, r, sb=R.eval_stat_bounds(ref, case["rm"]))
    # eval inputs are not conditioned: an element within the z bound of 0 may come out 0 or its small positive value
    edge = ref["z"].abs() <= bnd["z"]
    yb = torch.where(edge, bnd["y"] + ref["z"].abs(), bnd["y"])
    msgs = R.violations(dict(y=_rows(y)), ref, dict(y=yb), ["y"])
    assert not msgs, "\n".join(msgs)


def test_seed_sweep_of_the_voxel_row_cases(hip_lib):
    """64 seeded, conditioned draws of each small case of test_bn_act_gpu.py::test_bn_act_voxel_rows (bf16 rows, residual off /
    on, ReLU): every output within its bound.  All inputs keep |pre-activation| >= MARGIN, so a mismatch here is a kernel error
    in k_bn_stats_* / k_bn_bwd_*; the message lists each offending element with its row, channel and float64 pre-activation.
    Prints the number of elements the conditioning moved."""
    moved = total = 0
    failures = []
    for M, C in [(1000, 16), (777, 32), (300, 128), (5, 48)]:
        for residual in (False, True):
            for seed in range(64):
                case = _draw((M, C), torch.bfloat16, residual, seed=10007 * seed + M + C + residual)
                moved += case["moved"]
                total += M * C
                try:
                    _check((M, C), torch.bfloat16, case, True, _run((M, C), case, True), f"seed {seed}")
                except AssertionError as e:
                    failures.append(str(e))
    print(f"\nseed sweep: {moved} of {total} elements moved by the conditioning (margin {R.MARGIN}); {len(failures)} failing draws")
    assert not failures, "\n\n".join(failures[:8])


def test_residual_into_a_slice_matches_the_unfused_gradients(hip_lib):
    """bn_act(bn, x, residual, relu=True, out=slice): the backward's mask source is the saved output, a strided slice here; the
    gradients must equal those of the dense-output call bit for bit."""
    shape = (2, 64, 9, 13)
    outs = []
    for fused in (True, False):
        case = _draw(shape, torch.float32, True, seed=77)
        got = _run(shape, case, True, ld_extra=64 if fused else 0)
        outs.append(got)
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("shape", [(1, 32), (1, 16, 1, 1)])
def test_training_with_one_value_per_channel_raises(hip_lib, shape):
    """torch's BatchNorm raises ValueError for P = 1 in training mode; so does the HIP path, before touching any buffer."""
    from unidistill_amd.layers.dense import batchnorm_act
    C = shape[1]
    bn = (torch.nn.BatchNorm2d if len(shape) == 4 else torch.nn.BatchNorm1d)(C).cuda().train()
    x = torch.randn(*shape, device="cuda")
    if len(shape) == 4:
        x = x.contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        batchnorm_act(bn, x)
    with pytest.raises(ValueError):
        bn(x.float())                                          # the reference behaviour
    assert int(bn.num_batches_tracked) in (0, 1)               # (torch's module counts the step before it raises)
    assert bool((bn.running_mean == 0).all()) and bool((bn.running_var == 1).all())


# ---- C. BatchNorm partial sums from the convolution epilogues -------------------------------------------------------------------
PRODUCERS = [
    # name, dtype, kernel size, (B, Cin, H, W, Cout), the profiling counter of the kernel that must run
    ("bf16-3x3", torch.bfloat16, 3, (2, 64, 33, 41, 128), "conv2d.k_conv3x3"),
    ("bf16-1x1", torch.bfloat16, 1, (3, 128, 40, 37, 80), "conv2d.k_conv1x1"),
    ("f32-direct-3x3", torch.float32, 3, (2, 64, 33, 41, 128), "conv2d.k_conv3x3_f32"),
    ("f32-persistent-1x1", torch.float32, 1, (3, 128, 40, 37, 96), "conv2d.k_conv1x1_f32"),
    ("f32-tile-1x1", torch.float32, 1, (3, 64, 40, 37, 96), "conv2d.k_conv1x1_f32"),
]


@pytest.mark.parametrize("ratio", [0.0, 8.0], ids=["zero-mean", "mean8std"])
@pytest.mark.parametrize("name,dtype,ks,shape,counter", PRODUCERS, ids=[p[0] for p in PRODUCERS])
def test_conv_epilogue_partials_vs_float64(hip_lib, name, dtype, ks, shape, counter, ratio):
    """Per-tile (sum, sum of squares) of the stored output from each convolution epilogue without a float64 check elsewhere,
    summed, and the mean / var / running buffers ud_bn_stats_from_partials makes of them, against float64 statistics of the
    stored output.  ratio 8: a conv bias of 8x the output's std (center_head.py's shared conv has a bias), so the unshifted
    variance E[y^2] - E[y]^2 cancels ~65:1.  The bound is derived (bn_reference.partial_bounds: fp32 chains of <= 128 rows per
    tile, tiles in double); var_error_ratio_bound(8) = 1.6e-3 relative in the worst case.  The measured errors are printed next
    to those of the pivot-shifted stand-alone pass (ud_bn_stats*) on the same output.  Measured on MI355X, max relative var
    error: zero mean 5e-8 - 1.4e-7 for every producer; |mean|/std = 8: bf16 3x3 / 1x1 1.0e-7 / 1.4e-7, fp32 direct 3x3 1.8e-6,
    fp32 persistent 1x1 1.6e-6, fp32 per-tile 1x1 3.7e-6 -- up to ~15x the pivot-shifted pass (<= 3e-7 there), the cost of the
    unshifted E[y^2] - E[y]^2, and far inside the derived bound and the 1e-3 that would call for a shifted epilogue."""
    from unidistill_amd import _lib
    from unidistill_amd.ops import bn_act as hb, conv2d as c16, conv2d_f32 as c32
    B, cin, H, W, cout = shape
    g = torch.Generator(device="cuda").manual_seed(sum(shape) + ks + int(ratio))
    x = torch.randn(B, cin, H, W, generator=g, device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
    w = torch.randn(cout, cin, ks, ks, generator=g, device="cuda") * (cin * ks * ks) ** -0.5
    bias = torch.full((cout,), ratio, device="cuda") if ratio else None
    gamma = torch.rand(cout, generator=g, device="cuda") + 0.5
    beta = torch.randn(cout, generator=g, device="cuda") * 0.3
    rm0 = torch.randn(cout, generator=g, device="cuda") * 0.1
    rv0 = torch.rand(cout, generator=g, device="cuda") + 0.5
    old = (c32.USE_WINOGRAD, c32.USE_WINO4)
    _lib.prof_read(counter, reset=True)
    _lib.prof_enable(True)
    try:
        if dtype == torch.float32 and ks == 3:
            c32.USE_WINOGRAD = c32.USE_WINO4 = False       # the direct kernel (the Winograd ones have their own float64 test)
            assert not c32.wino_pays(H, W, cin, cout) and not c32.wino4_pays(H, W, cin, cout)
        if name == "f32-persistent-1x1":
            assert c32.persistent_1x1(cin) and c32.P1X1_STATS
        if name == "f32-tile-1x1":
            assert not c32.persistent_1x1(cin)
        mod = c16 if dtype == torch.bfloat16 else c32
        conv = mod.conv3x3 if ks == 3 else mod.conv1x1
        wt = w.to(dtype) if dtype == torch.bfloat16 else w
        with torch.no_grad():
            y = conv(x, wt, bias, True)
        torch.cuda.synchronize()
    finally:
        _lib.prof_enable(False)
        c32.USE_WINOGRAD, c32.USE_WINO4 = old
    assert _lib.prof_read(counter)[1] == 1, f"{name}: {counter} did not run"
    part, slices, rows = y._ud_bn_partial
    P = B * H * W
    assert rows == P and y.dtype == dtype
    yr = _rows(y).double()
    mean64, std64 = yr.mean(0), yr.std(0)
    if ratio:
        assert float((mean64.abs() / std64).min()) > 0.75 * ratio        # the cancellation this case is about
    st = part[:slices * cout * 2].view(slices, cout, 2).double().sum(0)
    ref = R.reference(yr, gamma, beta, EPS, momentum=MOM, running_mean=rm0, running_var=rv0)
    dm, dq, sb = R.partial_bounds(yr, ref, EPS)
    assert bool(((st[:, 0] / P - yr.mean(0)).abs() <= dm).all()), "sum"
    assert bool(((st[:, 1] / P - (yr * yr).mean(0)).abs() <= dq).all()), "sum of squares"
    bnd = R.bounds(yr, ref, dtype, EPS, None, MOM, rm0, rv0, sb=sb)
    errs = {}
    for via in ("partials", "pivot"):
        rm, rv = rm0.clone(), rv0.clone()
        vec = hb.batch_stats(y, gamma, beta, rm, rv, True, MOM, EPS, None, (part, slices, rows) if via == "partials" else None)
        got = dict(mean=vec[0], var=vec[1], invstd=vec[2], scale=vec[3], shift=vec[4], running_mean=rm, running_var=rv)
        errs[via] = float(((got["var"].double() - ref["var"]).abs() / ref["var"]).max())
        if via == "partials":
            msgs = R.violations(got, ref, bnd, ["mean", "var", "invstd", "scale", "shift", "running_mean", "running_var"])
            assert not msgs, f"{name} ratio {ratio}\n" + "\n".join(msgs)
    assert errs["partials"] <= R.var_error_ratio_bound(ratio)
    print(f"\n{name} |mean|/std={ratio:g}: max relative var error {errs['partials']:.2e} (epilogue partials), "
          f"{errs['pivot']:.2e} (pivot-shifted pass)")
