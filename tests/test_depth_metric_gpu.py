"""GPU: the depth metric (csrc/depth_metric.hip, ops/depth_metric.py, evaluation.DepthMetric, train.ValidationStep) against the
float64 restatement of tests/depth_metric_ref.py.

Integer terms (count, d1..d3, bin_acc, bin_acc1) must be exact; the inputs are checked, on the restatement alone, to hold no
labelled pixel on a knife edge.  Floating terms have a MEASURED tolerance: the same expression evaluated with plain PyTorch
fp32 ops on the same device is the yardstick.  Per term (the largest absolute error over the groups and ranges) the kernel's
error may be at most 4 x that evaluation's, plus one ulp of the float64 result where PyTorch's error happens to be zero.  The
factor 4 allows a different but still fp32 summation order inside the softmax."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import depth_metric_ref as R

pytestmark = pytest.mark.gpu
D_LO, D_STEP = 2.0, 0.5
EXTRA = 80                      # context channels behind the depth logits in the channels-last slice


def _bound(D):
    return [D_LO, D_LO + D * D_STEP, D_STEP]


def _edges(D, n_ranges):
    span = D * D_STEP
    if n_ranges == 1:
        return [D_LO, D_LO + span]
    return [D_LO + f * span for f in (0.125, 0.375, 0.625, 0.875)]          # labelled pixels below and above fall in no bucket


def _draw(D, BN, fH, fW, seed):
    """Seeded inputs with the two cheap margins built in: the arg-max logit is raised by 0.01 (no near-tie), a depth within
    1e-3 of a range edge is moved by 0.01.  The delta thresholds are left to the knife-edge check and the choice of the seed."""
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(BN, D + EXTRA, fH, fW, generator=g) * 2.0
    feat[:, :D].scatter_add_(1, feat[:, :D].argmax(1, keepdim=True), torch.full((BN, 1, fH, fW), 0.01))
    dmin = D_LO + torch.rand(BN, fH, fW, generator=g) * (D * D_STEP * 0.999)
    for e in _edges(D, 1) + _edges(D, 3):
        dmin[(dmin - e).abs() < 1e-3] += 0.01
    dmin[torch.rand(BN, fH, fW, generator=g) < 0.5] = float("inf")           # about half the pixels have no LiDAR return
    if BN * fH * fW == 1:
        dmin[...] = D_LO + 0.4 * D * D_STEP                                   # the single pixel is a labelled one
    return feat, dmin


# first seeds, found on the CPU, whose draw holds no knife-edge pixel (the test still checks, and reseeds at most 3 times)
SEEDS = {(5, 1): 5001, (5, 6): 5006, (5, 12): 5014, (64, 1): 64001, (64, 6): 64007, (64, 12): 64013,
         (112, 1): 112001, (112, 6): 112006, (112, 12): 112012, (256, 1): 256001, (256, 6): 256006, (256, 12): 256020}


@functools.lru_cache(maxsize=None)
def _case(D, BN, fH, fW):
    """The input of one (D, shape) and its restatement's per-pixel terms, computed once and shared by the layouts, groupings
    and range sets; reseeded (at most 3 times) while a labelled pixel sits on a knife edge of either range set."""
    for reseed in range(4):
        feat, dmin = _draw(D, BN, fH, fW, SEEDS[D, BN] + reseed)
        pix = R.pixel_terms(feat[:, :D].numpy(), dmin.numpy(), D_LO, D_STEP)
        if R.knife_edges(pix, _edges(D, 1) + _edges(D, 3)) == 0:
            break
    else:
        raise AssertionError("no input without a knife-edge pixel in 3 reseeds")
    return feat, dmin, pix, reseed


def _accumulate(logits, dmin, D, edges, groups, state=None):
    from unidistill_amd.ops import depth_metric as op
    if state is None:
        state = torch.zeros(groups, len(edges) - 1, 12, dtype=torch.float64, device="cuda")
    return op.depth_metric_accumulate(logits, dmin, state, _bound(D), edges, groups)


def _layout(feat, D, channels_last):
    """NCHW logits of their own, or the first D channels of a channels-last [BN, D + EXTRA, fH, fW] tensor: a view, no copy."""
    if channels_last:
        x = feat.cuda().contiguous(memory_format=torch.channels_last)[:, :D]
        assert x.stride(1) == 1 or x.shape[2] * x.shape[3] == 1
        return x
    return feat[:, :D].contiguous().cuda()


def _check(state, ref, yard, what):
    """state: the kernel's float64 [G, R, 12]; ref: the restatement; yard: the plain-PyTorch fp32 evaluation."""
    state = state.cpu().numpy()
    for t in R.INTEGER_TERMS:
        assert np.array_equal(state[..., t], ref[..., t]), (what, t, state[..., t], ref[..., t])
    for t in R.FLOAT_TERMS:
        e_k, e_t = np.abs(state[..., t] - ref[..., t]).max(), np.abs(yard[..., t] - ref[..., t]).max()
        bound = 4.0 * e_t + (np.spacing(np.abs(ref[..., t]).max()) if e_t == 0.0 else 0.0)
        print(f"{what} term {t}: |ref| {np.abs(ref[..., t]).max():.6g}  |err| kernel {e_k:.3e}  torch-fp32 {e_t:.3e}")
        assert e_k <= bound, f"{what} term {t}: kernel error {e_k:.3e} > 4 x torch-fp32 error {e_t:.3e}"
    assert np.isfinite(state).all()


SHAPES = [(1, 1, 1), (6, 3, 7), (12, 16, 44)]
# ncam_groups = 6 does not divide the single image of (1, 1, 1): that combination is a refusal (test_refusals), not a case
CASES = [(D, s, cl, G, nr) for D in (5, 64, 112, 256) for s in SHAPES for cl in (False, True) for G in (1, 6) for nr in (1, 3)
         if s[0] % G == 0]


# ---- 1. against the float64 restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,shape,channels_last,groups,n_ranges", CASES)
def test_against_float64_restatement(hip_lib, D, shape, channels_last, groups, n_ranges):
    feat, dmin, pix, reseed = _case(D, *shape)
    assert reseed <= 3
    edges = _edges(D, n_ranges)
    ref = R.depth_metric_state(None, None, D_LO, D_STEP, edges, groups, pix=pix)
    x, d = _layout(feat, D, channels_last), dmin.cuda()
    yard = R.torch_fp32_state(x, d, D_LO, D_STEP, edges, groups)
    state = _accumulate(x, d, D, edges, groups)
    assert ref[..., 0].sum() >= 1
    if n_ranges == 3 and shape[0] > 1:
        assert ref[..., 0].sum() < pix["labelled"].sum()                      # some labelled pixels lie outside every bucket
    _check(state, ref, yard, f"D={D} {shape} {'NHWC' if channels_last else 'NCHW'} G={groups} R={n_ranges}")


# ---- 2. decisions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", [False, True])
def test_decisions(hip_lib, channels_last):
    D = 5                                                  # bins [2, 2.5), ..., [4, 4.5); hi = 4.5
    nan, inf = float("nan"), float("inf")
    below_hi = float(np.nextafter(np.float32(4.5), np.float32(0)))
    dvals = [2.0, 4.5, inf, nan, -3.0, 2.6, 3.0, below_hi, 1.9999999, -inf]
    dmin = torch.tensor(dvals, dtype=torch.float32).reshape(1, 2, 5)
    feat = torch.zeros(1, D + EXTRA, 2, 5)
    feat[0, :D] = torch.tensor([1.0, 3.0, 3.0, 0.0, 3.0]).view(D, 1, 1)       # three equal maxima: the arg-max is bin 1
    x, d = _layout(feat, D, channels_last), dmin.cuda()
    # one bucket over everything: d_lo itself counts, d_lo + D * step, +-inf, NaN, negative and just-below-d_lo do not
    s = _accumulate(x, d, D, [-1e9, 1e9], 1).cpu().numpy()[0, 0]
    assert s[0] == 4                                                          # 2.0, 2.6, 3.0, below_hi
    assert s[9] == 1 and s[10] == 3                                           # bins 0, 1, 2, 4 against arg-max 1
    pix = R.pixel_terms(feat[:, :D].numpy(), dmin.numpy(), D_LO, D_STEP)
    assert pix["labelled"].ravel().tolist() == [True, False, False, False, False, True, True, True, False, False]
    assert pix["ahat"][pix["labelled"]].tolist() == [1, 1, 1, 1]
    # an inner edge belongs to the upper bucket; 2.0 and 2.6 lie below the first edge and are counted nowhere
    s = _accumulate(x, d, D, [2.75, 3.0, 4.0, 4.5], 1).cpu().numpy()[0]
    assert s[:, 0].tolist() == [0, 1, 1]
    ref = R.depth_metric_state(None, None, D_LO, D_STEP, [2.75, 3.0, 4.0, 4.5], 1, pix=pix)
    assert np.array_equal(s[:, list(R.INTEGER_TERMS)], ref[0][:, list(R.INTEGER_TERMS)])
    # the upper end of the last bucket is excluded
    s = _accumulate(x, d, D, [2.0, 3.0], 1).cpu().numpy()[0, 0]
    assert s[0] == 2                                                          # 2.0 and 2.6; 3.0 is outside


def test_labelled_set_is_the_label_kernels(hip_lib):
    """On a synthetic cloud and rig the metric counts exactly the cells ud_depth_labels labels: per camera the same number,
    none of the others, all of these."""
    from test_depth_sup import D_BOUND, DS, FINAL_DIM, random_cloud_case
    from unidistill_amd.ops import depth_metric as op, depth_sup
    pts, s2e, intrin, ida, bda = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in random_cloud_case())
    dmin, label = depth_sup.lidar_depth_labels(pts, s2e, intrin, ida, bda, D_BOUND, FINAL_DIM, DS)
    B, ncam, fH, fW = dmin.shape
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(B * ncam, 112, fH, fW, generator=g).cuda()
    wide = [-1e30, 1e30]

    def count(dm):
        st = torch.zeros(ncam, 1, 12, dtype=torch.float64, device="cuda")
        return op.depth_metric_accumulate(logits, dm, st, D_BOUND, wide, ncam)[:, 0, 0].cpu()
    per_cam = (label >= 0).sum((0, 2, 3)).cpu().double()
    assert per_cam.min() > 100 and (label < 0).sum() > 100
    assert torch.equal(count(dmin), per_cam)
    inf = torch.full_like(dmin, float("inf"))
    assert float(count(torch.where(label >= 0, inf, dmin)).sum()) == 0.0                # nothing outside label >= 0 counts
    assert torch.equal(count(torch.where(label >= 0, dmin, inf)), per_cam)              # everything inside does


# ---- 3. numerics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", [False, True])
def test_extreme_logits(hip_lib, channels_last):
    """+-80 on the labelled bin and on another one (p_b underflows to 0 in fp32: its nll is -ln 1e-44, finite), and a D-wide
    constant row (a uniform softmax; the tie goes to bin 0)."""
    D, BN, fH, fW = 64, 2, 3, 8
    g = torch.Generator().manual_seed(77)
    feat = torch.randn(BN, D + EXTRA, fH, fW, generator=g)
    dmin = torch.full((BN, fH, fW), D_LO + 5.25 * D_STEP)                      # bin 5 everywhere
    dmin[1, :, ::3] = float("inf")
    for k, (vl, vo) in enumerate(((-80.0, 80.0), (80.0, -80.0), (80.0, 80.0), (-80.0, -80.0))):
        feat[:, 5, :, k] = vl
        feat[:, 40, :, k] = vo
    feat[:, :D, :, 4] = 80.0
    feat[:, :D, :, 5] = -80.0
    feat[:, :D, :, 6] = 0.0
    edges = _edges(D, 1)
    pix = R.pixel_terms(feat[:, :D].numpy(), dmin.numpy(), D_LO, D_STEP)
    ref = R.depth_metric_state(None, None, D_LO, D_STEP, edges, 1, pix=pix)
    x, d = _layout(feat, D, channels_last), dmin.cuda()
    state = _accumulate(x, d, D, edges, 1)
    _check(state, ref, R.torch_fp32_state(x, d, D_LO, D_STEP, edges, 1), f"extremes {'NHWC' if channels_last else 'NCHW'}")
    # the underflowing pixels alone: nll is exactly -ln(1e-44) per pixel
    under = torch.full_like(dmin, float("inf"))
    under[:, :, 0] = dmin[:, :, 0]
    n_under = int(torch.isfinite(under).sum())
    s = _accumulate(x, under.cuda(), D, edges, 1).cpu().numpy()[0, 0]
    assert s[0] == n_under and np.isfinite(s).all()
    assert abs(s[11] - n_under * -np.log(1e-44)) <= 1e-13 * s[11]


# ---- 4. accumulation and reproducibility ------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", [False, True])
def test_accumulation_and_repeat(hip_lib, channels_last):
    from unidistill_amd import evaluation
    D, shape = 112, (12, 16, 44)
    feat, dmin, pix, _ = _case(D, *shape)
    edges = _edges(D, 3)
    x, d = _layout(feat, D, channels_last), dmin.cuda()
    m = evaluation.DepthMetric(_bound(D), ncam=6, range_edges=edges, per_camera=True, device="cuda")
    m.add_batch(x[:6], d[:6].view(1, 6, 16, 44))
    m.add_batch(x[6:], d[6:].view(1, 6, 16, 44))
    ref = R.depth_metric_state(None, None, D_LO, D_STEP, edges, 6, pix=pix)
    _check(m.state, ref, R.torch_fp32_state(x, d, D_LO, D_STEP, edges, 6), "two add_batch calls")
    one = _accumulate(x, d, D, edges, 6)
    ints = list(R.INTEGER_TERMS)
    assert torch.equal(m.state[..., ints], one[..., ints])
    # the same call twice from a zeroed state: bitwise
    again = _accumulate(x, d, D, edges, 6)
    assert torch.equal(one, again)
    # an all-unlabelled batch and an empty batch leave the state bitwise unchanged
    before = one.clone()
    _accumulate(x, torch.full_like(d, float("inf")), D, edges, 6, state=one)
    assert torch.equal(one, before)
    _accumulate(x[:0], d[:0], D, edges, 6, state=one)
    assert torch.equal(one, before)
    # compute(): the figures of the restatement's sums
    got = m.compute()
    tot = ref.sum((0, 1))
    assert got["n"] == int(tot[0]) and len(got["ranges"]) == 3 and len(got["cameras"]) == 6
    assert abs(got["abs_rel"] - tot[2] / tot[0]) < 1e-5 and abs(got["rmse"] - np.sqrt(tot[4] / tot[0])) < 1e-4
    m.reset()
    assert float(m.state.abs().max()) == 0.0 and m.compute()["n"] == 0
    # bf16 logits are widened
    sb = _accumulate(x.bfloat16(), d, D, edges, 6)
    assert torch.equal(sb[..., 0], one[..., 0])


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(hip_lib):
    from unidistill_amd import _lib
    from unidistill_amd.ops import depth_metric as op
    dev = torch.device("cuda")
    x = torch.zeros(6, 257, 2, 3, device=dev)
    d = torch.full((6, 2, 3), 3.0, device=dev)
    state = torch.zeros(6, 8, 12, dtype=torch.float64, device=dev)
    ws = torch.full((1 << 16,), 7, dtype=torch.uint8, device=dev)
    assert 0 < hip_lib.ud_depth_metric_workspace_bytes(6, 2, 3) <= ws.numel()

    def raw(D=112, G=1, R=1, BN=6, edges=None):
        e = (ctypes.c_double * 10)(*(edges if edges is not None else [2.0] + [50.0 + i for i in range(9)]))
        return hip_lib.ud_depth_metric_accumulate(x.data_ptr(), 257 * 6, 6, 3, 1, d.data_ptr(), BN, D, 2, 3, G, 2.0, 0.5, e, R,
                                                  state.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_of(x))
    for kw in (dict(D=257), dict(D=0), dict(R=0), dict(R=9), dict(G=0), dict(G=4), dict(BN=5, G=2),
               dict(R=2, edges=[2.0, 5.0, 4.0] + [9.0] * 7)):
        assert raw(**kw) != 0, kw
    torch.cuda.synchronize()
    assert float(state.abs().max()) == 0.0 and bool((ws == 7).all())           # nothing ran: state and scratch untouched
    assert raw(BN=0) == 0 and raw() == 0                                        # the empty batch is fine, and so is the good call
    torch.cuda.synchronize()
    assert float(state[0, 0, 0]) == 36.0 and not bool((ws == 7).all())
    state.zero_()
    # the Python op raises for the same, and for CPU tensors
    with pytest.raises(RuntimeError):
        op.depth_metric_accumulate(x, d, state[:1, :1], [2.0, 130.5, 0.5], [2.0, 130.5], 1)          # D = 257
    for edges in ([2.0], list(range(2, 12))):
        with pytest.raises((RuntimeError, ValueError, AssertionError)):
            op.depth_metric_accumulate(x[:, :5], d, state[:1], _bound(5), edges, 1)
    with pytest.raises((RuntimeError, ValueError, AssertionError)):
        op.depth_metric_accumulate(x[:, :5], d, state[:4, :1], _bound(5), [2.0, 4.5], 4)              # 6 % 4 != 0
    with pytest.raises(RuntimeError, match="GPU only"):
        op.depth_metric_accumulate(x[:, :5].cpu(), d.cpu(), state[:1, :1], _bound(5), [2.0, 4.5], 1)
    with pytest.raises(RuntimeError, match="GPU only"):
        op.depth_metric_accumulate(x[:, :5], d, state[:1, :1].cpu(), _bound(5), [2.0, 4.5], 1)
    torch.cuda.synchronize()
    assert float(state.abs().max()) == 0.0


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------
class _NoEval:
    def add_batch(self, *a):
        pass


def test_validation_step_end_to_end(hip_lib):
    """A one-camera student from build_model on two synthetic batches: the step's metric equals the restatement applied to the
    depth logits and labels evaluated separately, and the predictions are bitwise those of the step without the metric."""
    from unidistill_amd import _lib, evaluation, train
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = train.build_model("camera").to(dev)
    enc = model.camera_encoder.backbone
    D = enc.depth_channels
    batches = [train.synthetic_batch(dev, 1, ncam=1, seed=s) for s in (1234, 99)]
    m = evaluation.DepthMetric(enc.d_bound, ncam=1, device=dev)
    with_metric, plain = train.ValidationStep(model, _NoEval(), depth_metric=m), train.ValidationStep(model, _NoEval())
    # the camera model's eval-mode image BatchNorm on NCHW activations has no hand-written kernel: library path allowed
    with _lib.strict(False), torch.no_grad():
        got = [with_metric(b, [i], None) for i, b in enumerate(batches)]
        want = [plain(b, [i], None) for i, b in enumerate(batches)]
        model.eval()
        sep = []
        for b in batches:
            _, logits = enc(b["imgs"], b["mats_dict"], is_return_depth="logits")
            dmin, label = enc.lidar_depth_labels(b["points"], b["mats_dict"])
            sep.append((logits.float().cpu().numpy(), dmin.cpu().numpy().reshape(-1, *dmin.shape[2:]), int((label >= 0).sum())))
        model.train()
    for a, b in zip(got, want):
        assert len(a) == len(b) == 1
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert torch.equal(a[0][k], b[0][k]), k
    lo, step = float(enc.d_bound[0]), float(enc.d_bound[2])
    edges = [lo, lo + D * step]
    ref = sum(R.depth_metric_state(x, d, lo, step, edges, 1) for x, d, _ in sep)
    out = m.compute()
    assert out["n"] == sum(n for _, _, n in sep) == int(ref[0, 0, 0]) and out["n"] > 20
    tot = ref[0, 0]
    want_fig = evaluation.depth_figures(tot)
    state = m.state.cpu().numpy()
    ints = list(R.INTEGER_TERMS)
    print("end to end:", out)
    # the logits are random-weight outputs, so a pixel may sit on a knife edge; those decide the integer terms' slack
    pix = [R.pixel_terms(x, d, lo, step) for x, d, _ in sep]
    knife = sum(R.knife_edges(p, edges) for p in pix)
    assert np.abs(state[0, 0, ints] - tot[ints]).max() <= knife
    for k in ("abs_rel", "sq_rel", "rmse", "rmse_log", "mae", "nll"):
        assert abs(out[k] - want_fig[k]) <= 1e-5 * abs(want_fig[k]) + 1e-6 * knife, (k, out[k], want_fig[k])
