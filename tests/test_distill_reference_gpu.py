"""GPU: the kernels of csrc/distill.hip (k_box_corners, k_feat, k_rel, the deterministic scatter with both sorters, k_mask_*, k_resp
through the strided entry points) against the float64 restatement of tests/distill_reference.py on the cases of tests/distill_cases.py:
a non-square map, channel counts around the wave size, key points on and outside the map's edge, the sorter boundaries, six and eight
tasks in three memory layouts, and mask boxes outside each side of the map.

Index-like outputs (`valid`, the mask) are exact; the mask may differ by one float32 ulp where the device's exp rounds the other way.
Losses and gradients, per compared quantity: 4x what a float32 evaluation of the restatement loses against its float64 one on the same
inputs, never below 1e-6 of the quantity's largest magnitude.  Gradient values that depend on a sign within distill_reference.MARGIN of
undecided are left out (at most 1 % per case, tests/test_distill_reference_cpu.py).  Constructed zeros and untouched values are exact,
and every gradient is bitwise the same when computed again.

Measured on an MI355X (kernel deviation / float32 restatement's deviation / allowed), the largest over the layouts of a case; no mask
value used the one-ulp allowance (104 / 105 / 105 / 31 non-zero values); every touched gradient value was compared except 4 of 7696
(scatter m455, feature); all 6460 / 8398 heat-map gradient values were compared
  corners                 BEV pixels 4.8e-07 / 9.5e-07 / 4.2e-05
  feature  C 1            loss 3.5e-07 / 4.7e-07 / 1.9e-06    gradient 8.8e-08 / 8.8e-08 / 3.5e-07
           C 63           loss 4.5e-08 / 4.5e-08 / 1.2e-06    gradient 1.5e-09 / 1.5e-09 / 6.0e-09
           C 64           loss 2.5e-07 / 2.5e-07 / 1.2e-06    gradient 1.4e-09 / 1.4e-09 / 5.5e-09
           C 65           loss 1.9e-08 / 1.0e-07 / 1.2e-06    gradient 1.5e-09 / 1.5e-09 / 6.2e-09
           C 130          loss 4.6e-09 / 4.6e-09 / 1.2e-06    gradient 7.7e-10 / 7.7e-10 / 3.1e-09
  relation C 1            loss 8.0e-09 / 5.2e-08 / 5.0e-07    gradient 4.1e-07 / 4.1e-07 / 1.7e-06
           C 63           loss 1.0e-08 / 3.0e-09 / 7.1e-08    gradient 2.1e-09 / 2.1e-09 / 8.3e-09
           C 64           loss 1.5e-08 / 7.5e-09 / 7.0e-08    gradient 2.2e-09 / 2.2e-09 / 8.8e-09
           C 65           loss 1.1e-08 / 3.3e-08 / 1.3e-07    gradient 1.6e-09 / 1.7e-09 / 6.8e-09
           C 130          loss 2.2e-08 / 2.2e-08 / 8.7e-08    gradient 1.0e-09 / 1.0e-09 / 4.2e-09
  scatter m56   feature   loss 2.9e-08 / 9.0e-08 / 1.7e-06    gradient 1.1e-08 / 1.1e-08 / 4.4e-08
                relation  loss 2.7e-08 / 2.8e-09 / 2.5e-07    gradient 6.4e-09 / 7.1e-09 / 2.9e-08
  scatter m57   feature   loss 4.1e-08 / 1.6e-07 / 1.6e-06    gradient 9.4e-09 / 9.4e-09 / 3.8e-08
                relation  loss 2.7e-09 / 2.7e-09 / 2.3e-07    gradient 1.4e-08 / 1.4e-08 / 5.8e-08
  scatter m227  feature   loss 2.3e-08 / 9.6e-08 / 2.0e-06    gradient 1.4e-08 / 1.8e-08 / 7.2e-08
                relation  loss 2.8e-09 / 1.2e-08 / 1.8e-07    gradient 1.1e-08 / 1.4e-08 / 5.7e-08
  scatter m228  feature   loss 5.2e-08 / 5.2e-08 / 1.7e-06    gradient 2.2e-08 / 3.4e-08 / 1.4e-07
                relation  loss 1.1e-08 / 4.2e-09 / 2.5e-07    gradient 1.2e-08 / 1.2e-08 / 4.7e-08
  scatter m455  feature   loss 4.2e-08 / 2.0e-07 / 1.7e-06    gradient 2.4e-08 / 2.7e-08 / 1.1e-07
                relation  loss 1.0e-09 / 1.0e-09 / 2.2e-07    gradient 1.3e-08 / 4.2e-08 / 1.7e-07
  scatter m456  feature   loss 1.1e-07 / 1.3e-07 / 1.7e-06    gradient 3.9e-08 / 2.5e-08 / 9.8e-08
                relation  loss 2.6e-08 / 2.6e-08 / 3.1e-07    gradient 4.1e-08 / 3.1e-08 / 1.2e-07
  scatter map512 feature  loss 3.0e-07 / 5.4e-07 / 2.1e-06    gradient 7.9e-08 / 1.1e-07 / 4.4e-07
                relation  loss 4.4e-07 / 3.8e-07 / 1.5e-06    gradient 9.5e-07 / 8.6e-07 / 3.4e-06
  scatter map_wide feature loss 4.0e-07 / 6.4e-07 / 2.6e-06   gradient 1.4e-07 / 1.4e-07 / 5.7e-07
                relation  loss 6.5e-07 / 6.8e-07 / 2.7e-06    gradient 1.6e-04 / 1.6e-04 / 6.4e-04
  accumulate              feature 2.8e-07 / 2.8e-07 / 4.2e-06    relation 2.6e-07 / 3.3e-07 / 4.2e-06
  response 6 tasks 1e-4   cls 3.0e-09 / 3.0e-09 / 8.2e-08    reg 1.5e-08 / 1.5e-08 / 4.0e-07
                          heat-map gradients 4.8e-10 / 4.8e-10 / 4.4e-09    regression gradients 1.6e-11 / 1.6e-11 / 1.3e-10
  response 6 tasks 1e-3   cls 7.9e-09 / 7.9e-09 / 8.2e-08    reg and the gradients as for 1e-4
  response 8 tasks 1e-4   cls 4.3e-09 / 4.3e-09 / 7.2e-08    reg 1.1e-08 / 1.9e-08 / 4.0e-07
                          heat-map gradients 4.3e-10 / 4.3e-10 / 4.2e-09    regression gradients 1.2e-11 / 1.2e-11 / 9.7e-11
  response 8 tasks 1e-3   cls 1.4e-08 / 1.4e-08 / 7.2e-08    reg and the gradients as for 1e-4
Before the 16384-entry LDS sort was taken out of csrc/distill.hip, scatter m455 failed with "HIP runtime / launch failure (-3)".
"""
import numpy as np
import pytest
import torch

import distill_cases as C
import distill_reference as D

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


class _Report:
    """Prints every figure before anything is asserted; check() at the end fails with all quantities over their bound."""

    def __init__(self, title):
        self.title, self.over = title, []

    def compare(self, what, got, ref64, ref32, sel=None):
        if isinstance(got, torch.Tensor):
            got = got.detach().cpu().numpy()
        got, ref64, ref32 = (np.asarray(v, np.float64) for v in (got, ref64, ref32))
        if sel is not None:
            got, ref64, ref32 = got[sel], ref64[sel], ref32[sel]
        if ref64.size == 0:
            return
        assert np.isfinite(got).all(), f"{self.title} {what}: not finite"
        f32 = float(np.abs(ref32 - ref64).max())
        tol = max(4 * f32, 1e-6 * float(np.abs(ref64).max()))
        dev = float(np.abs(got - ref64).max())
        print(f"{self.title} | {what}: kernel {dev:.3e} float32 restatement {f32:.3e} allowed {tol:.3e} (largest magnitude "
              f"{float(np.abs(ref64).max()):.3e}, {ref64.size} values)")
        if not dev <= tol:
            self.over.append(f"{what}: {dev:.3e} > {tol:.3e}")

    def check(self):
        assert not self.over, f"{self.title}: " + "; ".join(self.over)


# ---- corners and validity --------------------------------------------------------------------------------------------------------
def test_box_corners_and_valid(hip_lib):
    """The corner kernel on the box cases' rows, and `valid` on the mask cases' rows: an all-zero row inside the valid range, an
    all-zero sample (valid[0] stays set: the scan never goes below row 0), S = 7, 9, 10 with a row that is zero only in its first seven
    columns, a NaN entry, M = 1."""
    from unidistill_amd.ops import distill as ds
    geo = C.box_geometry()
    pc = (C.BOX_PC_MIN[0], C.BOX_PC_MIN[1], -5.0, 10.0, 6.0, 3.0)
    corners, valid = ds.box_corners_bev(_dev(geo["gt"]), pc, (C.BOX_PIXEL[0], C.BOX_PIXEL[1], 0.2), 1)
    assert np.array_equal(valid.cpu().numpy(), geo["valid"])
    rep = _Report("corners")
    rep.compare("BEV pixels", corners, geo["corners_of_gt"][0], D.box_corners(geo["gt"], C.BOX_PC_MIN, C.BOX_PIXEL, np.float32)[0])
    rep.check()
    pc = (C.MASK_PC_MIN[0], C.MASK_PC_MIN[1], -5.0, 0.0, 0.0, 3.0)
    for c in [C.mask_case(S) for S in (7, 9, 10)] + [C.mask_case_m1()]:
        _, valid = ds.box_corners_bev(_dev(c["gt"]), pc, (0.075, 0.1, 0.2), 8)
        assert np.array_equal(valid.cpu().numpy(), c["valid"])


# ---- box losses ------------------------------------------------------------------------------------------------------------------
def _box_run(c, kind, channels_last):
    from unidistill_amd.ops import distill as ds
    s = _dev(c["s"])
    if channels_last:
        s = s.contiguous(memory_format=torch.channels_last)
    s.requires_grad_(True)
    fn = ds.BEVDistillLoss if kind else ds.FeatureDistillLoss
    loss = fn(s, _dev(c["t"]), _dev(c["corners"]), _dev(c["valid"]))
    (loss * c["upstream"]).backward()
    return float(loss.detach()), s.grad


def _box_check(title, c, kind, channels_last):
    rep = _Report(title)
    r64, r32 = c["f64"], c["f32"]
    loss, grad = _box_run(c, kind, channels_last)
    loss2, grad2 = _box_run(c, kind, channels_last)
    assert loss == loss2 and torch.equal(_bits(grad), _bits(grad2))       # reproducible
    B, C_, H, W = c["s"].shape
    g = grad.cpu().numpy()
    rep.compare("loss", np.array([loss]), np.array([r64["loss"]]), np.array([r32["loss"]]))
    keep = ~r64["left_out"]
    rep.compare("gradient", g, r64["grad"], r32["grad"], keep)
    untouched = ~np.broadcast_to(r64["touched"].reshape(B, 1, H, W), g.shape)
    print(f"{title} | gradient compared on {int((keep & ~untouched).sum())} of {int((~untouched).sum())} touched values")
    assert float(np.abs(g[untouched]).max()) == 0.0                        # nothing outside the footprints
    return rep, g


@pytest.mark.parametrize("C_", C.BOX_CHANNELS)
@pytest.mark.parametrize("kind", [0, 1], ids=["feature", "relation"])
def test_box_losses_match_float64(hip_lib, kind, C_):
    """H = 24, W = 40.  Swapping H and W in make_bilin moves every key point (the row would come from b and the column from a scaled
    the other way): loss and gradient of the box fully inside are off by O(1).  Dropping one of the q.in[] tests lets a padding tap of
    the four straddling boxes and of the boxes at column -1/2 / W - 1/2 read the neighbouring row (or memory outside the map) with a
    weight of up to 1/2 and scatters gradient there: the loss moves, and pixels the restatement leaves untouched become non-zero.
    C = 1, 63, 65, 130: a wave's channel loop with idle lanes, a ragged second trip and a third one; a lane that adds channel c + 64
    without the c < C test changes the norms and sums at once.  The box that samples only padding runs k_rel's zero-norm branch."""
    c = C.box_case(kind, C_)
    reps = []
    for cl in (False, True):
        rep, g = _box_check(f"{'relation' if kind else 'feature'} C {C_} {'channels-last' if cl else 'nchw'}", c, kind, cl)
        (b, pix), = c["agree_pixels"]
        assert float(np.abs(g.reshape(2, C_, -1)[b][:, pix]).max()) == 0.0    # student == teacher there: sign(0) = 0, exactly
        reps.append(rep)
    for rep in reps:
        rep.check()


@pytest.mark.parametrize("kind", [0, 1], ids=["feature", "relation"])
@pytest.mark.parametrize("name", list(C.SCATTER_CASES))
def test_scatter_at_the_sorter_boundaries(hip_lib, name, kind):
    """M = 56 / 57: 2016 terms fill the 2048-entry sort, 2052 need the 4096-entry one; M = 227 / 228: 8172 terms are the largest LDS
    sort, 8208 go to the rank sort; M = 455 / 456: the boundary the code used to name, whose 16384-entry LDS sort asked for 16 bytes
    more than a CU has (every M in 228..455 failed at launch); map_wide: 7200 terms on 2^19 pixels take the rank sort for the key
    width.  A sorter chosen one size too small drops the terms past its end: those are the last box's, which sits alone on pixels of
    its own (non-zero in the restatement, asserted on the CPU), so its gradient would be missing.  Runs of up to 2400 terms cross
    thread, wave and 256-entry boundaries: a run cut at a boundary stores a partial sum over the full one, off by O(1) of the value."""
    c = C.scatter_case(name, kind)
    rep, _ = _box_check(f"scatter {name} {'relation' if kind else 'feature'}", c, kind, False)
    rep.check()


@pytest.mark.parametrize("kind", [0, 1], ids=["feature", "relation"])
def test_box_bwd_acc_adds_into_a_channels_last_map(hip_lib, kind):
    """ud_distill_box_bwd_acc called as feature_tap's backward calls it, into a pre-filled channels-last map: touched pixels get the
    gradient added, every other value keeps its bits."""
    from unidistill_amd import _lib
    from unidistill_amd.ops import distill as ds
    c = C.acc_case(kind)
    B, C_, H, W = c["s"].shape
    M = c["corners"].shape[1]
    s, t, corners, valid = _dev(c["s"]), _dev(c["t"]), _dev(c["corners"]), _dev(c["valid"].astype(np.uint8))
    gscale = torch.tensor([c["scale"]], dtype=torch.float32, device="cuda")
    outs = []
    for _ in range(2):
        g = _dev(c["prefill"]).contiguous(memory_format=torch.channels_last)
        assert not g.is_contiguous()
        ws = _lib.workspace(s.device, hip_lib.ud_distill_box_bwd_workspace_bytes(B, M, C_), "distill_bwd")
        _lib.ud.ud_distill_box_bwd_acc(kind, s, ds._strides(s), t, ds._strides(t), corners, valid, B, M, C_, H, W, gscale, g,
                                       ds._strides(g), ws, ws.numel(), _lib.stream_of(s))
        outs.append(g)
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    rep = _Report(f"accumulate {'relation' if kind else 'feature'}")
    rep.compare("map after", outs[0], c["after_f64"], c["after_f32"], ~c["f64"]["left_out"])
    untouched = ~np.broadcast_to(c["f64"]["touched"].reshape(B, 1, H, W), c["s"].shape)
    assert np.array_equal(outs[0].cpu().numpy().view(np.int32)[untouched], c["prefill"].view(np.int32)[untouched])
    assert untouched.any() and not untouched.all()
    rep.check()


# ---- response loss ---------------------------------------------------------------------------------------------------------------
def _resp_tensors(hm, reg, layout, grad, seed):
    """-> (per-task dicts, grads()): separate NCHW leaves, channels-last leaves, or channel slices of ONE packed channels-last tensor
    with a spare channel after every head (what the packed head returns: batch stride, channel stride and pixel stride all differ from
    a dense map's, per tensor)."""
    n = len(hm)
    per_task = [[hm[i]] + list(reg[6 * i:6 * i + 6]) for i in range(n)]
    names = ("hm",) + C.HEADS
    if layout != "packed":
        fmt = torch.channels_last if layout == "nhwc" else torch.contiguous_format
        leaves = [[_dev(x).contiguous(memory_format=fmt).requires_grad_(grad) for x in xs] for xs in per_task]
        dicts = [dict(zip(names, xs)) for xs in leaves]
        return dicts, lambda: ([xs[0].grad.cpu().numpy() for xs in leaves], [x.grad.cpu().numpy() for xs in leaves for x in xs[1:]])
    B, _, H, W = hm[0].shape
    total = sum(x.shape[1] + 1 for xs in per_task for x in xs)
    pk = torch.randn(B, total, H, W, generator=torch.Generator().manual_seed(seed)) * 3    # the spare channels: nobody may read them
    at, c0 = [], 0
    for xs in per_task:
        row = []
        for x in xs:
            pk[:, c0:c0 + x.shape[1]] = torch.from_numpy(x)
            row.append((c0, x.shape[1]))
            c0 += x.shape[1] + 1
        at.append(row)
    pk = pk.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(grad)
    dicts = [{nm: pk[:, a:a + w] for nm, (a, w) in zip(names, row)} for row in at]

    def grads():
        g = pk.grad.cpu().numpy()
        used = np.zeros(total, bool)
        for row in at:
            for a, w in row:
                used[a:a + w] = True
        assert float(np.abs(g[:, ~used]).max()) == 0.0                    # the spare channels get exactly nothing
        return [g[:, row[0][0]:row[0][0] + row[0][1]] for row in at], [g[:, a:a + w] for row in at for a, w in row[1:]]
    return dicts, grads


def _resp_run(c, layout):
    from unidistill_amd.ops import distill as ds
    sd, grads = _resp_tensors(c["s_hm"], c["s_reg"], layout, True, 11)
    td, _ = _resp_tensors(c["t_hm"], c["t_reg"], layout, False, 12)
    lc, lr = ds.ResponseDistillLoss(sd, td, None, None, None, None, clamp=c["clamp"], mask=_dev(c["mask"]))
    (C.RESP_W_CLS * lc + C.RESP_W_REG * lr).backward()
    g_hm, g_reg = grads()
    return float(lc), float(lr), np.concatenate(g_hm, 1), np.concatenate(g_reg, 1)


def _resp_check(ntasks, clamp, layout):
    c = C.response_case(ntasks, clamp)
    r64, r32 = c["f64"], c["f32"]
    rep = _Report(f"response {ntasks} tasks clamp {clamp} {layout}")
    lc, lr, g_hm, g_reg = _resp_run(c, layout)
    lc2, lr2, g_hm2, g_reg2 = _resp_run(c, layout)
    assert (lc, lr) == (lc2, lr2) and np.array_equal(g_hm.view(np.int32), g_hm2.view(np.int32))
    assert np.array_equal(g_reg.view(np.int32), g_reg2.view(np.int32))
    cat = lambda xs: np.concatenate(xs, 1)
    rep.compare("cls", np.array([lc]), np.array([r64["cls"]]), np.array([r32["cls"]]))
    rep.compare("reg", np.array([lr]), np.array([r64["reg"]]), np.array([r32["reg"]]))
    keep = ~np.broadcast_to(r64["left_out"][:, None], g_hm.shape)
    rep.compare("heat-map gradients", g_hm, cat(r64["g_hm"]), cat(r32["g_hm"]), keep)
    rep.compare("regression gradients", g_reg, cat(r64["g_reg"]), cat(r32["g_reg"]))
    print(f"{rep.title} | heat-map gradients compared on {int(keep.sum())} of {keep.size} values")
    # exact: which values are zero.  The heat-map gradient is non-zero on one channel per pixel at most (the first maximum), the
    # regression gradient exactly where mask != 0 and s != t; a wrong stride reads another channel or pixel and moves these patterns
    assert np.array_equal(g_hm[keep] != 0, cat(r64["g_hm"])[keep] != 0)
    assert np.array_equal(g_reg != 0, cat(r64["g_reg"]) != 0)
    B, HW = C.RESP_B, C.RESP_H * C.RESP_W
    zero_mask = np.broadcast_to((c["mask"] == 0)[:, None], g_hm.shape)
    assert zero_mask.any() and not g_hm[zero_mask].any() and not g_reg[np.broadcast_to((c["mask"] == 0)[:, None], g_reg.shape)].any()
    first = np.cumsum((0,) + c["ncls"])
    fh, fr = g_hm.reshape(B, -1, HW), g_reg.reshape(B, -1, HW)
    b, p = C.PIX_TIE
    (t0, c0), (t1, c1) = C.TIE_AT
    assert fh[b, first[t0] + c0, p] > 0 and fh[b, first[t1] + c1, p] == 0 and np.count_nonzero(fh[b, :, p]) == 1
    b, p = C.PIX_EQ
    assert not fh[b, :, p].any()                                           # smax == tmax: sign(0) = 0
    b, p = C.PIX_REG
    assert not fr[b, :, p].any() and fh[b, :, p].any()
    return rep


@pytest.mark.parametrize("clamp", [1e-4, 1e-3])
@pytest.mark.parametrize("layout", ["nchw", "nhwc", "packed"])
def test_response_loss_six_tasks_match_float64(hip_lib, layout, clamp):
    """Six tasks, 6 heat maps with (1, 2, 2, 1, 2, 2) classes and 36 regression tensors, each with its own (batch, channel, pixel)
    strides.  In the packed layout a batch stride taken as channels x H W, a channel stride of H W or a pixel stride of 1 reads
    another head's values or a spare channel (random, 3x the scale): both losses move by O(1) and the zero pattern of the gradients
    no longer follows mask and ties; a gradient written with the student's strides instead of its own lands in the wrong element.
    reg_total (66) enters the regression loss and every regression gradient as 1 / 66."""
    _resp_check(6, clamp, layout).check()


@pytest.mark.parametrize("clamp", [1e-4, 1e-3])
def test_response_loss_eight_tasks_are_the_limit(hip_lib, clamp):
    """8 heat maps and 48 regression tensors fill RespArgs; nine tasks are refused with the project's error before anything runs."""
    from unidistill_amd.ops import distill as ds
    _resp_check(8, clamp, "packed").check()
    c = C.response_case(9, clamp)
    sd, _ = _resp_tensors(c["s_hm"], c["s_reg"], "nchw", True, 11)
    td, _ = _resp_tensors(c["t_hm"], c["t_reg"], "nchw", False, 12)
    with pytest.raises(RuntimeError, match=r"ud_distill_resp_fwd_strided failed: unsupported configuration"):
        ds.ResponseDistillLoss(sd, td, None, None, None, None, clamp=clamp, mask=_dev(c["mask"]))
    assert all(x.grad is None for d in sd for x in d.values())


# ---- Gaussian mask ---------------------------------------------------------------------------------------------------------------
def _mask_check(c, title):
    from unidistill_amd.ops import distill as ds
    B = c["gt"].shape[0]
    pc = (C.MASK_PC_MIN[0], C.MASK_PC_MIN[1], -5.0, 0.0, 0.0, 3.0)
    got = ds.calculate_box_mask_gaussian((B, 1, C.MASK_H, C.MASK_W), _dev(c["gt"]), pc, (0.075, 0.1, 0.2), 8).cpu().numpy()
    ref = c["mask"]
    assert got.shape == ref.shape and got.dtype == np.float32
    ulps = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    print(f"{title} | mask: {int((ulps == 1).sum())} of {int((ref != 0).sum())} non-zero values differ by one float32 ulp, "
          f"{int((ulps > 1).sum())} by more")
    assert np.array_equal(got == 0, ref == 0) and np.array_equal(got == 1, ref == 1)
    assert int(ulps.max()) <= 1


@pytest.mark.parametrize("S", [7, 9, 10])
def test_gaussian_mask_is_the_restatement(hip_lib, S):
    """H = 20, W = 28, pixels of 0.6 x 0.8 m.  Centres outside each side by less than r, r, r + 1 and 1000 pixels (drawn, drawn, empty,
    empty), radius 0, zero and NaN dimensions, two overlapping boxes, a zero-sum row with real boxes after it (not drawn), an all-zero
    sample, and a row that is zero in its first seven columns only: drawn for S = 9 and 10, the end of the sample for S = 7."""
    _mask_check(C.mask_case(S), f"S {S}")
    if S == 10:
        _mask_check(C.mask_case_m1(), "M 1")
