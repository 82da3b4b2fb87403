"""CPU: the float64 restatement of the detection loss's default terms (tests/det_loss_reference.py) is the tensor-op formulation
CenterHeadIouAware._loss_terms_torch, values and gradients, on every case the GPU test uses; and those cases keep away from the decisions
they are not meant to sit on (conditions on the inputs, not measurements)."""
import pytest
import torch

import det_loss_cases as C
import det_loss_reference as D
from test_dense_head import _head

# focal case, regression case, tasks of the regression case taken in turn (the focal cases decide the task count)
PAIRS = [("two_trips", "two_trips", 3), ("tiny", "tiny", 3), ("tiny", "edges", 3), ("eight_tasks", "tiny", 8)]


def _close(got, ref, what):
    scale = float(ref[torch.isfinite(ref)].abs().max()) if bool(torch.isfinite(ref).any()) else 1.0
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12 * scale, equal_nan=True, msg=lambda m: f"{what}: {m}")


@pytest.mark.parametrize("nb", [10, 8])
@pytest.mark.parametrize("focal,reg,T", PAIRS, ids=[f"{f}-{r}" for f, r, _ in PAIRS])
def test_restatement_is_the_tensor_op_formulation(focal, reg, T, nb):
    fc, rc = C.focal_case(focal), C.reg_inputs(reg)
    sel = torch.arange(T) % C.T_REG
    _, B, K, H, W = rc["shape"]
    ncm = fc["shape"][2]
    f64 = lambda v: v.double()
    planes, ind, mask, tgt, num_obj = f64(rc["planes"][sel]), rc["ind"][sel], rc["mask"][sel], f64(rc["tgt"][sel]), f64(rc["num_obj"][sel])
    w_pos, w_neg, w_p = fc["w"]
    w_box, w_iou, w_aw = (w[sel] for w in rc["w"])
    heads = tuple(n for n in C.NAMES if nb == 10 or n != "vel")

    def leaves():
        hm = [x.double().clone().requires_grad_(True) for x in fc["logits"]]
        pl = planes.clone().requires_grad_(True)
        return hm, pl

    def total(prob, pos, neg, box, il, aw):
        return ((w_pos * pos).sum() + (w_neg * neg).sum() + (w_p * prob).sum() + (w_box[:, :nb] * box).sum() + (w_iou * il).sum()
                + (w_aw * aw).sum())

    # the project's formulation on float64 CPU tensors (stride 1 and the voxel size (sx, sy): the two only enter as their product)
    head = _head()
    head.num_classes = list(fc["ncls"])
    hm_a, pl_a = leaves()
    preds = []
    for t in range(T):
        pd, j = {"hm": hm_a[t]}, 0
        for nm, wd in zip(C.NAMES, C.WIDTH):
            pd[nm] = pl_a[t, :, j:j + wd].reshape(B, wd, H, W)
            j += wd
        preds.append(pd)
    pos_a, neg_a, box_a, il_a, aw_a = head._loss_terms_torch(preds, fc["gt"].double(), ind, mask, tgt, num_obj, ncm, heads, nb, C.ALPHA,
                                                             C.GAMMA, 1, (C.SX, C.SY), {})
    prob_a = torch.stack([torch.nn.functional.pad(pd["hm"], (0, 0, 0, 0, 0, ncm - pd["hm"].shape[1])) for pd in preds])
    ga = torch.autograd.grad(total(prob_a, pos_a, neg_a, box_a, il_a, aw_a), hm_a + [pl_a])
    # the restatement
    hm_b, pl_b = leaves()
    prob_b, pos_b, neg_b = D.focal_ref(hm_b, fc["gt"].double(), C.ALPHA, C.GAMMA)
    box_b, il_b, aw_b, _ = D.reg_ref(C.gathered(pl_b, ind), tgt, mask, num_obj, C.SX, C.SY, nb)
    gb = torch.autograd.grad(total(prob_b, pos_b, neg_b, box_b, il_b, aw_b), hm_b + [pl_b])
    for name, a, b in (("prob", prob_a, prob_b), ("pos", pos_a, pos_b), ("neg", neg_a, neg_b), ("box", box_a, box_b),
                       ("iou_loss", il_a, il_b), ("iou_aware", aw_a, aw_b)):
        _close(b.detach(), a.detach(), name)
    assert int(torch.isnan(box_a).sum()) == (len(sel[sel == 0]) if nb == 10 else 0)       # the NaN velocity target: task 0's column 8
    for i, (a, b) in enumerate(zip(ga, gb)):
        assert bool(torch.isfinite(a).all())
        _close(b, a, f"gradient {i}")
    if nb == 8:
        assert float(gb[-1][:, :, 8:10].abs().max()) == 0.0


@pytest.mark.parametrize("name", list(C.FOCAL_CASES))
def test_focal_inputs_keep_off_the_sigmoid_clamp(name):
    c = C.focal_case(name)
    T, B, ncm, H, W = c["shape"]
    for t, x in enumerate(c["logits"]):
        assert float(((x.double().abs() - D.LOGIT_CLAMP).abs()).min()) >= 1e-3
        flat = x.reshape(B, -1, H * W)
        for b, ch, p0 in C.fixed_positions(c["ncls"][t], B, H * W):
            assert flat[b, ch, p0:p0 + 4].tolist() == list(C.FIXED_LOGITS)
    gt = c["gt"]
    assert int((gt[T - 1, :, :c["ncls"][T - 1]] == 1).sum()) == 0 and int((gt[0, :, :c["ncls"][0]] == 1).sum()) > 0
    assert bool(((gt > 0) & (gt < 1)).any()) and bool((gt == 0).any())
    if name == "two_trips":
        assert B * ncm * H * W > 2 * 64 * 256 and (B * ncm * H * W) % (64 * 256) != 0       # a third, ragged trip of k_focal_fwd's grid


@pytest.mark.parametrize("nb", [10, 8])
@pytest.mark.parametrize("name", list(C.REG_CASES))
def test_regression_inputs_keep_off_the_decisions(name, nb):
    c = C.reg_case(name, nb)
    T, B, K, H, W = c["shape"]
    mask, margin = c["mask"], c["f64"][4]
    assert C.positive_pixels_distinct(c["ind"], mask)
    assert bool(torch.isinf(margin[~mask]).all())
    _, switch = D.bev_target(C.gathered(c["planes"].double(), c["ind"]), c["tgt"].double(), C.SX, C.SY)
    assert float(switch[mask].min()) >= D.MARGIN if bool(mask.any()) else True       # the forward value jumps there
    left_out = int(((margin < D.MARGIN) & mask).sum())
    print(f"{name} nb {nb}: {left_out} of {int(mask.sum())} positive slots within {D.MARGIN} of a decision")
    if name == "edges":
        assert float(margin.min()) >= C.EDGE_DISTANCE - 1e-6         # 0.05 as constructed; the inputs are then rounded to float32
        assert left_out == 0
    else:
        assert left_out <= 0.05 * int(mask.sum())
    t, b, k = c["nan_at"]
    assert bool(mask[t, b, k]) and int(torch.isnan(c["tgt"]).sum()) == 1 and bool(torch.isnan(c["tgt"][t, b, k, 8]))
    if name == "two_trips":
        assert B * K > 8 * 256 and (B * K) % 256 != 0                 # a second, ragged trip of k_reg_fwd's 8 chunks of 256
        assert 0.4 < float(mask.float().mean()) < 0.6
    if name == "tiny":
        assert c["num_obj"].tolist() == [3.0, 0.25, 0.0] and mask.sum(dim=(1, 2)).tolist() == [3, 1, 0]
