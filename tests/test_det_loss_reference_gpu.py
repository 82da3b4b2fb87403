"""GPU: the detection loss's default kernels (k_focal_fwd / k_focal_bwd, k_reg_fwd<false> / k_reg_bwd<false>, k_sum_partials), called
directly on leaves the test builds, against the float64 restatement of tests/det_loss_reference.py at shapes where every part of them
runs: more than two trips of the focal grid (n = 34560 > 2 x 64 x 256, ragged), a second trip of the regression chunks (2400 slots >
8 x 256, ragged), eight tasks, most blocks idle, and one constructed slot on each side of every decision (tests/det_loss_cases.py).

Tolerances follow tests/test_rot_iou_gpu.py and tests/test_det_loss_rot_gpu.py, per compared quantity: 4x what a float32 evaluation of the
restatement loses against its float64 one on the same inputs, never below 1e-6 of the quantity's largest magnitude; head gradients are
compared per gathered value at the positive slots at least det_loss_reference.MARGIN away from every decision.

Measured on an MI355X (kernel deviation / float32 restatement's deviation / allowed), the largest over both layouts
(head gradients: the gathered value closest to its bound; nb = 8 gives the same losses as nb = 10)
  focal two_trips    prob 8.2e-08 / 8.2e-08 / 1.0e-06    pos 1.5e-05 / 1.2e-05 / 2.1e-04    neg 2.1e-04 / 4.5e-05 / 3.0e-03
                     dlogit at the fixed logits 2.9e-05 / 2.9e-05 / 1.2e-04    elsewhere 2.0e-06 / 1.9e-06 / 7.6e-06
  focal tiny         prob 5.8e-08 / 5.8e-08 / 1.0e-06    pos 2.6e-07 / 3.7e-07 / 4.7e-06    neg 1.7e-05 / 1.9e-05 / 7.7e-05
                     dlogit at the fixed logits 2.9e-05 / 2.9e-05 / 1.1e-04    elsewhere 1.9e-07 / 1.4e-07 / 1.1e-06
  focal eight_tasks  prob 7.8e-08 / 7.8e-08 / 1.0e-06    pos 5.9e-07 / 8.4e-07 / 7.7e-06    neg 1.8e-05 / 2.0e-05 / 8.0e-05
                     dlogit at the fixed logits 2.7e-05 / 2.7e-05 / 1.1e-04    elsewhere 2.4e-07 / 2.3e-07 / 1.2e-06
  reg two_trips      box 2.3e-07 / 2.1e-07 / 3.5e-06    iou_loss 3.6e-08 / 8.3e-08 / 1.1e-06    iou_aware 8.0e-08 / 5.6e-08 / 8.5e-07
                     head gradients 4.8e-10 / 4.2e-10 / 1.9e-09 (3536 of 3622 positive slots)    box_loss alone 1.2e-10 / 4.2e-11 / 1.0e-09
  reg tiny           box 9.5e-07 / 9.5e-07 / 1.5e-05    iou_loss 1.0e-07 / 1.0e-07 / 8.6e-07    iou_aware 2.8e-08 / 2.8e-08 / 2.3e-06
                     head gradients 3.1e-07 / 6.8e-08 / 2.0e-06 (4 of 4)    box_loss alone 3.1e-07 / 6.8e-08 / 2.0e-06
  reg edges          box 2.2e-07 / 2.2e-07 / 4.0e-06    iou_loss 5.0e-08 / 6.6e-08 / 1.2e-06    iou_aware 1.6e-08 / 2.3e-08 / 3.5e-07
                     head gradients 5.1e-09 / 5.3e-09 / 5.6e-08 (96 of 96)    box_loss alone 4.3e-09 / 4.3e-09 / 4.5e-08
Without the prob term dlogit measures the same to two digits.  The fixed logits +-9 sit next to the sigmoid clamp, where 1 - p cancels and
float32 itself loses 2e-5 relative: they are a quantity of their own so that they do not loosen the bound of all other elements.
"""
import ctypes

import pytest
import torch

import det_loss_cases as C
import det_loss_reference as D

pytestmark = pytest.mark.gpu


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


class _Report:
    """Prints every figure before anything is asserted; check() at the end fails with all quantities over their bound."""

    def __init__(self, title):
        self.title, self.over = title, []

    def compare(self, what, got, ref64, ref32, sel=None):
        got, ref64, ref32 = got.detach().cpu().double(), ref64.double(), ref32.double()
        if sel is not None:
            got, ref64, ref32 = got[sel], ref64[sel], ref32[sel]
        if ref64.numel() == 0:
            return
        assert bool(torch.isfinite(got).all()), f"{self.title} {what}: not finite"
        f32 = float((ref32 - ref64).abs().max())
        tol = max(4 * f32, 1e-6 * float(ref64.abs().max()))
        dev = float((got - ref64).abs().max())
        print(f"{self.title} | {what}: kernel {dev:.3e} float32 restatement {f32:.3e} allowed {tol:.3e} (largest magnitude "
              f"{float(ref64.abs().max()):.3e}, {ref64.numel()} values)")
        if not dev <= tol:
            self.over.append(f"{what}: {dev:.3e} > {tol:.3e}")

    def check(self):
        assert not self.over, f"{self.title}: " + "; ".join(self.over)


# ---- focal term ------------------------------------------------------------------------------------------------------------------
def _focal_leaves(c, packed):
    """-> (hms on the GPU, grads()): separate contiguous leaves, or channel slices of one packed [B, Ctot, H, W] leaf with a spare
    channel after every head, so that the batch stride is not ncls HW."""
    T, B, ncm, H, W = c["shape"]
    if not packed:
        hms = [x.detach().clone().cuda().requires_grad_(True) for x in c["logits"]]
        return hms, lambda: [h.grad.cpu() for h in hms]
    g = torch.Generator().manual_seed(5)
    pk = torch.randn(B, sum(c["ncls"]) + T, H, W, generator=g) * 3            # the spare channels hold values nobody may read
    c0, at = 0, []
    for x in c["logits"]:
        pk[:, c0:c0 + x.shape[1]] = x.detach()
        at.append((c0, x.shape[1]))
        c0 += x.shape[1] + 1
    pk = pk.cuda().requires_grad_(True)
    hms = [pk[:, a:a + n] for a, n in at]

    def grads():
        gr = pk.grad.cpu()
        used = torch.zeros(gr.shape[1], dtype=torch.bool)
        for a, n in at:
            used[a:a + n] = True
        assert float(gr[:, ~used].abs().max()) == 0.0
        return [gr[:, a:a + n] for a, n in at]
    return hms, grads


def _focal_run(c, packed, with_prob):
    from unidistill_amd.ops import det_loss
    w_pos, w_neg, w_p = (w.float().cuda() for w in c["w"])
    hms, grads = _focal_leaves(c, packed)
    prob, pos, neg = det_loss.focal_terms(hms, c["gt"].cuda(), C.ALPHA, C.GAMMA)
    total = (w_pos * pos).sum() + (w_neg * neg).sum()
    if with_prob:
        total = total + (w_p * prob).sum()
    total.backward()
    return prob.detach().cpu(), pos.detach().cpu(), neg.detach().cpu(), grads()


def _focal_check(name, packed):
    c = C.focal_case(name)
    T, B, ncm, H, W = c["shape"]
    r64, r32 = c["f64"], c["f32"]
    rep = _Report(f"focal {name} {'packed' if packed else 'planes'}")
    prob, pos, neg, dl = _focal_run(c, packed, True)
    _, pos_n, neg_n, dl_n = _focal_run(c, packed, False)                       # prob unused: its gradient arrives as zeros
    rep.compare("prob", prob, r64["prob"], r32["prob"])
    rep.compare("pos", pos, r64["pos"], r32["pos"])
    rep.compare("neg", neg, r64["neg"], r32["neg"])
    cat = lambda vs: torch.cat([v.reshape(-1) for v in vs])
    # next to the clamp (the fixed +-9) 1 - p cancels, float32 loses more there: those eight logits per task are a quantity of their own
    fixed = []
    for n in c["ncls"]:
        m = torch.zeros(B, n, H * W, dtype=torch.bool)
        for b, ch, p0 in C.fixed_positions(n, B, H * W):
            m[b, ch, p0:p0 + 4] = True
        fixed.append(m)
    fixed = cat(fixed)
    for what, sel in (("at the fixed logits", fixed), ("elsewhere", ~fixed)):
        rep.compare(f"dlogit {what}", cat(dl), cat(r64["dl"]), cat(r32["dl"]), sel)
        rep.compare(f"dlogit {what}, prob unused", cat(dl_n), cat(r64["dl_noprob"]), cat(r32["dl_noprob"]), sel)
    # exact zeros: padded class channels, the task without a positive, logits outside the sigmoid clamp
    for t, n in enumerate(c["ncls"]):
        assert float(prob[t, :, n:].abs().max()) == 0.0 if n < ncm else True
        assert float(prob[t, :, :n].min()) > 0.0
        flat = dl[t].reshape(B, n, H * W), dl_n[t].reshape(B, n, H * W)
        for b, ch, p0 in C.fixed_positions(n, B, H * W):
            for f in flat:
                assert f[b, ch, p0:p0 + 2].tolist() == [0.0, 0.0]              # +-12: the clamp binds, no gradient
            assert bool((flat[0][b, ch, p0 + 2:p0 + 4] != 0).all())            # +-9: inside, the gradient through prob passes
    assert float(pos[T - 1]) == 0.0 and float(pos_n[T - 1]) == 0.0
    assert torch.equal(_bits(pos), _bits(pos_n)) and torch.equal(_bits(neg), _bits(neg_n))
    # reproducible: a second evaluation is bitwise the same
    prob2, pos2, neg2, dl2 = _focal_run(c, packed, True)
    assert torch.equal(_bits(prob2), _bits(prob)) and torch.equal(_bits(pos2), _bits(pos)) and torch.equal(_bits(neg2), _bits(neg))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(dl2, dl))
    return rep


@pytest.mark.parametrize("packed", [False, True], ids=["planes", "packed"])
def test_focal_terms_match_float64(hip_lib, packed):
    # "tiny" right after "two_trips": the partial sums live in one shared workspace, stale ones of the larger map would show here
    reps = [_focal_check(name, packed) for name in ("two_trips", "tiny", "eight_tasks")]
    for rep in reps:
        rep.check()


@pytest.mark.parametrize("name", ["two_trips", "tiny"])
def test_focal_backward_entry_point_padded_channels_and_null_g_prob(hip_lib, name):
    """ud_det_focal_bwd called directly, where autograd cannot look: the padded class channels of dlogit (the wrapper slices them off)
    stay exactly 0 although g_prob is not 0 there, and a NULL g_prob is the zero gradient."""
    from unidistill_amd import _lib
    from unidistill_amd.ops import det_loss
    c = C.focal_case(name)
    T, B, ncm, H, W = c["shape"]
    ncls = c["ncls"]
    w_pos, w_neg, w_p = (w.float().cuda() for w in c["w"])
    gt = c["gt"].cuda()
    with torch.no_grad():
        prob, _, _ = det_loss.focal_terms([x.detach().cuda() for x in c["logits"]], gt, C.ALPHA, C.GAMMA)
    prob = prob.contiguous()
    out = []
    for g_prob in (w_p.contiguous(), None):
        dl = torch.full_like(prob, float("nan"))
        _lib.ud.ud_det_focal_bwd((ctypes.c_int * T)(*ncls), T, B, ncm, H * W, gt, prob, g_prob, w_pos, w_neg, C.ALPHA, float(C.GAMMA), dl,
                                 _lib.stream_of(prob))
        out.append(dl.cpu())
    rep = _Report(f"focal {name} entry point")
    cat = lambda vs: torch.cat([v.reshape(-1) for v in vs])
    for dl, key in zip(out, ("dl", "dl_noprob")):
        assert bool(torch.isfinite(dl).all())
        for t, n in enumerate(ncls):
            if n < ncm:
                assert float(dl[t, :, n:].abs().max()) == 0.0
        rep.compare(key, cat([dl[t, :, :n] for t, n in enumerate(ncls)]), cat(c["f64"][key]), cat(c["f32"][key]))
    rep.check()
    _, _, _, dl_auto = _focal_run(c, False, False)
    assert all(torch.equal(_bits(out[1][t, :, :n]), _bits(dl_auto[t])) for t, n in enumerate(ncls))


# ---- gathered regression / IoU terms ---------------------------------------------------------------------------------------------
def _reg_run(c, nb, packed, only_box=False, tgt=None):
    from unidistill_amd.ops import det_loss
    T, B, K, H, W = c["shape"]
    dev = lambda v: v.cuda()
    w_box, w_iou, w_aw = (dev(v.float()) for v in c["w"])
    preds, leaves, slots = C.preds_from_planes(c["planes"], packed, H, W)
    box, il, aw = det_loss.reg_terms(preds, dev(c["ind"]), dev(c["mask"]), dev(c["tgt"] if tgt is None else tgt), dev(c["num_obj"]),
                                     C.SX, C.SY, nb, iou_mode="reference")
    total = (box * w_box).sum()
    if not only_box:
        total = total + (il * w_iou).sum() + (aw * w_aw).sum()
    total.backward()
    return box.detach().cpu(), il.detach().cpu(), aw.detach().cpu(), C.plane_grads(leaves, slots, packed, T, B, H * W)


@pytest.mark.parametrize("packed", [False, True], ids=["planes", "packed"])
@pytest.mark.parametrize("nb", [10, 8])
@pytest.mark.parametrize("name", list(C.REG_CASES))
def test_reg_terms_match_float64(hip_lib, name, nb, packed):
    c = C.reg_case(name, nb)
    T, B, K, H, W = c["shape"]
    mask, ind = c["mask"], c["ind"]
    rep = _Report(f"reg {name} nb {nb} {'packed' if packed else 'planes'}")
    box, il, aw, grads = _reg_run(c, nb, packed)
    box64, il64, aw64, g64, margin = c["f64"]
    box32, il32, aw32, g32, _ = c["f32"]
    # the NaN velocity target: its column is NaN on both sides and nothing else is
    assert torch.equal(torch.isnan(box[:, :nb]), torch.isnan(box64))
    assert int(torch.isnan(box).sum()) == (1 if nb == 10 else 0) and (nb == 8 or bool(torch.isnan(box[c["nan_at"][0], 8])))
    assert float(box[:, nb:].abs().max()) == 0.0 if nb < 10 else True
    fin = ~torch.isnan(box64)
    rep.compare("box", box[:, :nb], box64, box32, fin)
    rep.compare("iou_loss", il, il64, il32)
    rep.compare("iou_aware", aw, aw64, aw32)
    ok = (margin >= D.MARGIN) & mask
    gk = C.gathered(grads, ind)                                                # [T,B,K,11]
    for j in range(11):
        rep.compare(f"gradient {j}", gk[..., j], g64[..., j], g32[..., j], ok)
    print(f"{rep.title} | gradients compared on {int(ok.sum())} of {int(mask.sum())} positive slots")
    # only box_loss used: the other two gradients arrive as zeros
    cb = C.reg_case(name, nb, True)
    box_b, il_b, aw_b, grads_b = _reg_run(c, nb, packed, only_box=True)
    gb = C.gathered(grads_b, ind)
    for j in range(11):
        rep.compare(f"gradient {j}, box_loss alone", gb[..., j], cb["f64"][3][..., j], cb["f32"][3][..., j], ok)
    assert float(grads_b[:, :, 10].abs().max()) == 0.0
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in ((box_b, box), (il_b, il), (aw_b, aw)))
    # nothing outside the positive slots: masked slots and every other pixel stay exactly zero (the spare packed channels: plane_grads)
    assert bool(torch.isfinite(grads).all()) and bool(torch.isfinite(il).all()) and bool(torch.isfinite(aw).all())
    hit = torch.zeros(T, B, 1, H * W, dtype=torch.bool)
    hit.scatter_(3, ind[:, :, None, :], mask[:, :, None, :])
    assert float(grads.masked_fill(hit, 0).abs().max()) == 0.0 and float(grads_b.masked_fill(hit, 0).abs().max()) == 0.0
    if nb == 8:
        assert float(grads[:, :, 8:10].abs().max()) == 0.0
    for t in range(T):
        if not bool(mask[t].any()):                                             # an empty task with num_obj = 0: exact zeros, no 0 / 0
            assert float(c["num_obj"][t]) == 0.0
            assert float(box[t].abs().max()) == 0.0 and float(il[t]) == 0.0 and float(aw[t]) == 0.0
            assert float(grads[t].abs().max()) == 0.0
    if name == "tiny":
        assert not bool(mask[2].any()) and float(c["num_obj"][1]) == 0.25
    # reproducible: a second evaluation is bitwise the same; with nb = 8 the targets may be 8 wide as well
    tgt = c["tgt"][..., :8].contiguous() if nb == 8 else None
    box2, il2, aw2, grads2 = _reg_run(c, nb, packed, tgt=tgt)
    assert torch.equal(_bits(box2), _bits(box)) and torch.equal(_bits(il2), _bits(il)) and torch.equal(_bits(aw2), _bits(aw))
    assert torch.equal(_bits(grads2), _bits(grads))
    rep.check()


def test_hip_assigner_positive_pixels_are_distinct(hip_lib):
    """The precondition of k_reg_bwd (a store, not an accumulation) on the HIP assigner's output where boxes crowd onto the same anchors:
    trial 3 of tests/test_assign_gpu.py."""
    from test_dense_head import _head, TASKS
    asg = _head().target_assigner
    trial = 3
    g = torch.Generator().manual_seed(40 + trial)
    names = [n for t in TASKS for n in t["class_names"]]
    B, M = 3, 30
    gt = torch.zeros(B, M, 10)
    for b, n in enumerate([M, 9, 0]):
        xy = (torch.rand(n, 2, generator=g) * 2 - 1) * 33.5
        if n:
            xy[: n // 2] = xy[0] + torch.randn(n // 2, 2, generator=g) * 0.6               # crowded
        gt[b, :n, 0:2] = xy
        gt[b, :n, 2] = torch.randn(n, generator=g)
        gt[b, :n, 3:6] = torch.rand(n, 3, generator=g) * 3 + 0.5
        gt[b, :n, 6] = (torch.rand(n, generator=g) * 2 - 1) * 6.0
        gt[b, :n, 7:9] = torch.randn(n, 2, generator=g)
        gt[b, :n, 9] = torch.randint(1, len(names) + 1, (n,), generator=g).float()
    asg.fused = True
    out = asg.assign_targets(gt.cuda())
    assert "_stacked" in out and out["_stacked"]["ind"].is_cuda                      # the kernel's output, not the tensor-op path's
    st = out["_stacked"]
    assert int(st["mask"].sum()) > 9 * 9                                             # crowded indeed: more positives than one box gives
    assert C.positive_pixels_distinct(st["ind"], st["mask"])


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def test_nine_tasks_are_refused_without_a_launch(hip_lib):
    from unidistill_amd import _lib
    from unidistill_amd.ops import det_loss
    T, B, ncm, HW, K = 9, 1, 1, 16, 4
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    hm = [f(B, 1, 4, 4) for _ in range(T)]
    gt, prob, pos_neg, dl = f(T, B, ncm, HW), f(T, B, ncm, HW), f(T, 2), f(T, B, ncm, HW)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    ncls = (ctypes.c_int * T)(*[1] * T)
    stream = _lib.stream_of(gt)
    table = (ctypes.c_void_p * T)(*[h.data_ptr() for h in hm])
    with pytest.raises(RuntimeError, match=r"ud_det_focal_fwd failed: invalid argument \(-1\)"):
        _lib.ud.ud_det_focal_fwd(table, (ctypes.c_longlong * T)(*[HW] * T), ncls, T, B, ncm, HW, gt, 0.25, 2.0, prob, pos_neg, ws,
                                 ws.numel(), stream)
    with pytest.raises(RuntimeError, match=r"ud_det_focal_bwd failed: invalid argument \(-1\)"):
        _lib.ud.ud_det_focal_bwd(ncls, T, B, ncm, HW, gt, prob, None, f(T), f(T), 0.25, 2.0, dl, stream)
    heads = [f(B, 1, 4, 4) for _ in range(T * 11)]
    htable = (ctypes.c_void_p * (T * 11))(*[h.data_ptr() for h in heads])
    ind, mask = torch.zeros(T, B, K, dtype=torch.long, device="cuda"), torch.ones(T, B, K, dtype=torch.uint8, device="cuda")
    tgt, num_obj, losses, loc, dhead = f(T, B, K, 10), f(T), f(T, 12), f(T, B, K, 19), f(T, B, 11, HW)
    for fwd, bwd in (("ud_det_reg_fwd", "ud_det_reg_bwd"), ("ud_det_reg_fwd_rot", "ud_det_reg_bwd_rot")):
        with pytest.raises(RuntimeError, match=fwd + r" failed: invalid argument \(-1\)"):
            getattr(_lib.ud, fwd)(htable, (ctypes.c_longlong * (T * 11))(*[HW] * (T * 11)), T, B, K, HW, 10, ind, mask, tgt, 10, num_obj,
                                  C.SX, C.SY, losses, loc, ws, ws.numel(), stream)
        with pytest.raises(RuntimeError, match=bwd + r" failed: invalid argument \(-1\)"):
            getattr(_lib.ud, bwd)(T, B, K, HW, 10, ind, mask, loc, f(T, 10), f(T), f(T), dhead, stream)
    assert hip_lib.ud_det_loss_workspace_bytes(9) == 0 and hip_lib.ud_det_loss_workspace_bytes(8) > 0
    torch.cuda.synchronize()
    for out in (prob, pos_neg, dl, losses, loc, dhead):                             # nothing ran: every output still holds its fill
        assert bool((out == 7.0).all())
    # the wrapper's own gate: nine tasks are not taken, eight are
    pd = {k: f(B, w, 4, 4) for k, w in zip(("hm",) + C.NAMES, (1,) + C.WIDTH)}
    assert det_loss.supported([pd] * 8, 10) and not det_loss.supported([pd] * 9, 10)
