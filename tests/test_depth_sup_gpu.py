"""GPU: LiDAR depth supervision (csrc/depth_sup.hip, ops/depth_sup.py) against the float64 restatement of tests/depth_sup_ref.py.

Labels: exact on constructed frustum planes, equal to the restatement on a random cloud outside the cells it marks near-edge
(at most 2 % of them: tests/test_depth_sup.py), independent of the order of the points, untouched by points that must not count.
Loss: forward and backward against float64 with a MEASURED tolerance -- the same expression evaluated with plain PyTorch fp32
ops on the same device is the yardstick, the kernel's error may be at most twice that evaluation's -- then through the model."""
import numpy as np
import pytest
import torch

import depth_sup_ref as R
from test_depth_sup import D_BOUND, DS, FINAL_DIM, random_cloud_case
from unidistill_amd import synthetic as syn

pytestmark = pytest.mark.gpu
FH, FW = FINAL_DIM[0] // DS, FINAL_DIM[1] // DS


def _labels(pts, s2e, intrin, ida, bda, d_bound=D_BOUND, final_dim=FINAL_DIM, ds=DS):
    from unidistill_amd.ops import depth_sup
    c = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dmin, label = depth_sup.lidar_depth_labels(c(pts), c(s2e), c(intrin), c(ida), c(bda), d_bound, final_dim, ds)
    return dmin.cpu().numpy(), label.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)


@pytest.fixture(scope="module")
def cloud():
    """The random-cloud input, its restatement (computed once) and the kernel's result."""
    case = random_cloud_case()
    ref = R.depth_labels(*case, D_BOUND, FINAL_DIM, DS)
    return case, ref


# ---- 1. frustum planes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", [0, 57, 111])
def test_frustum_planes_exact(hip_lib, j):
    """One point per (camera, cell) at the cell's centre pixel and in the middle of depth bin j, mapped to the ego frame with the
    forward chain: every cell of the camera gets label j and the depth of its point.  One cloud per camera, so that a neighbour
    camera's points (the fields of view overlap) cannot win a cell."""
    g = syn.rng(3)
    s2e, intrin, ida, bda = syn.camera_rig(g, B=2, ncam=6, bda_aug=True)
    s2e, intrin, ida = s2e[:, 0], intrin[:, 0], ida[:, 0]
    v, u = np.meshgrid((np.arange(FH) + 0.5) * DS, (np.arange(FW) + 0.5) * DS, indexing="ij")
    depth = D_BOUND[0] + (j + 0.5) * D_BOUND[2]
    d = np.full(u.size, depth)
    for c in range(6):
        pts = np.zeros((2, u.size, 5), np.float32)
        want = np.zeros((2, FH, FW), np.float32)
        for b in range(2):
            pts[b, :, :3] = R.frustum_points(s2e[b, c], intrin[b, c], ida[b, c], bda[b], u.ravel(), v.ravel(), d)
            P, mz, A = R.camera_projection(s2e[b, c], intrin[b, c], ida[b, c], bda[b])
            uu, vv, dd = R.project(P, mz, A, pts[b, :, :3].astype(np.float64))      # of the fp32 points the kernel reads
            assert np.abs(uu - u.ravel()).max() < 0.05 and np.abs(vv - v.ravel()).max() < 0.05 and np.abs(dd - depth).max() < 1e-4
            want[b] = dd.astype(np.float32).reshape(FH, FW)
        dmin, label = _labels(pts, s2e, intrin, ida, bda)
        assert np.all(label[:, c] == j), (j, c, np.unique(label[:, c]))
        ulp = np.abs(_bits(dmin[:, c]) - _bits(want)).max()
        assert ulp <= 1, (j, c, ulp)


# ---- 2. random cloud --------------------------------------------------------------------------------------------------------
def test_random_cloud_vs_restatement(hip_lib, cloud):
    case, (rdmin, rlabel, near) = cloud
    dmin, label = _labels(*case)
    ok = ~near
    print(f"cells {near.size}, near-edge {int(near.sum())}, labelled {int((rlabel >= 0).sum())}, "
          f"label mismatches outside near-edge {int((label != rlabel)[ok].sum())}, inside {int((label != rlabel)[near].sum())}")
    assert ((label >= 0) & ok).reshape(2, 6, -1).sum(-1).max() > 100
    assert np.array_equal(label[ok], rlabel[ok])
    assert np.array_equal(_bits(dmin)[ok], _bits(rdmin)[ok])
    assert np.all(np.isposinf(dmin[label < 0]) | (dmin[label < 0] >= D_BOUND[1]))


# ---- 3. order and repeat ----------------------------------------------------------------------------------------------------
def test_point_order_and_repeat(hip_lib, cloud):
    (pts, *mats), _ = cloud
    a = _labels(pts, *mats)
    b = _labels(pts, *mats)
    perm = syn.rng(11).permutation(pts.shape[1])
    s = _labels(pts[:, perm], *mats)
    for x, y in ((a, b), (a, s)):
        assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1], y[1])


# ---- 4. points that must not count ------------------------------------------------------------------------------------------
def _exact_rig():
    """A camera looking along +x from the origin with power-of-two-friendly intrinsics and no augmentation: the projection of
    an ego point (X, Y, Z) is d = X, u = 352 - 512 Y / X, v = 128 - 512 Z / X with every step exact for the points below."""
    s2e = np.eye(4, dtype=np.float32)
    s2e[:3, :3] = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float32)
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = 512.0
    K[0, 2], K[1, 2] = 352.0, 128.0
    return s2e[None, None], K[None, None], np.eye(4, dtype=np.float32)[None, None], None


def test_points_that_must_not_count(hip_lib, cloud):
    (pts, *_), _ = cloud
    rig = _exact_rig()
    base_pts = pts[:1]
    base = _labels(base_pts, *rig)
    assert (base[1] >= 0).sum() > 100
    nan, inf = np.float32("nan"), np.float32("inf")
    below58 = np.nextafter(np.float32(58.0), np.float32(0.0))
    rows = {"nan x": (nan, 1, 0), "nan z": (5, 1, nan), "+inf": (inf, 0, 0), "-inf y": (5, -inf, 0), "all inf": (inf, inf, -inf),
            "behind the camera": (-5, 0.5, 0.25), "d == d_bound[1]": (58, 0, 0), "u == W": (4, -2.75, 0),
            "v == H": (4, 0, -1.0), "d below d_bound[0]": (1.9990234375, 0, 0), "padding row": (0, 0, 0)}
    for name, xyz in rows.items():
        extra = np.zeros((1, 1, pts.shape[2]), np.float32)
        extra[0, 0, :3] = xyz
        got = _labels(np.concatenate([base_pts, extra], 1), *rig)
        assert np.array_equal(_bits(got[0]), _bits(base[0])) and np.array_equal(got[1], base[1]), name
    # all of them at once, in front of the cloud
    extra = np.zeros((1, len(rows), pts.shape[2]), np.float32)
    extra[0, :, :3] = np.array(list(rows.values()), np.float32)
    got = _labels(np.concatenate([extra, base_pts], 1), *rig)
    assert np.array_equal(_bits(got[0]), _bits(base[0])) and np.array_equal(got[1], base[1])
    # the same borders from the inside DO count (so the rows above were rejected by their own comparison, not by accident)
    lone = np.zeros((1, 3, 5), np.float32)
    lone[0, :, :3] = [(below58, 0, 0), (4, -2.7421875, 0.9921875), (2, 1.375, 0.5)]     # (u, v) = (352, 128), (703, 1), (0, 0)
    dmin, label = _labels(lone, *rig)
    assert label[0, 0, 8, 22] == 111 and dmin[0, 0, 8, 22] == below58
    assert label[0, 0, 0, 43] == 4 and dmin[0, 0, 0, 43] == 4.0
    assert label[0, 0, 0, 0] == 0 and dmin[0, 0, 0, 0] == 2.0
    assert (label >= 0).sum() == 3
    # empty cloud
    dmin, label = _labels(np.zeros((1, 0, 5), np.float32), *rig)
    assert np.all(label == -1) and np.all(np.isposinf(dmin)) and label.shape == (1, 1, FH, FW)


# ---- 5-7. loss --------------------------------------------------------------------------------------------------------------
BN, LC = 2, 8


def _loss_case(D, channels_last, empty_image, seed=0):
    g = torch.Generator().manual_seed(1000 * D + seed)
    feat = torch.randn(BN, D + LC, FH, FW, generator=g) * 2.0
    lab = torch.randint(0, D, (BN, FH, FW), generator=g)
    lab[torch.rand(BN, FH, FW, generator=g) > 0.3] = -1                  # about 30 % foreground
    if empty_image:
        lab[0] = -1
    feat = feat.cuda()
    if channels_last:
        feat = feat.contiguous(memory_format=torch.channels_last)
    return feat, lab.int().cuda()


def _check_loss(feat, lab, D, what):
    """-> the figures; asserts kernel error <= 2 x the error of the plain-PyTorch fp32 evaluation on the device."""
    from unidistill_amd.ops import depth_sup
    ref_loss, ref_dx = R.depth_loss(feat[:, :D], lab)
    xk = feat.clone().requires_grad_(True)
    loss_k = depth_sup.depth_loss(xk[:, :D], lab)
    loss_k.backward()
    xt = feat.clone().requires_grad_(True)
    loss_t = R.depth_loss_expr(xt[:, :D], lab.long())
    loss_t.backward()
    assert torch.isfinite(loss_k) and torch.isfinite(xk.grad).all()
    assert float(xk.grad[:, D:].abs().max()) == 0.0                      # the context channels get no gradient from this loss
    e_loss_k, e_loss_t = abs(float(loss_k) - float(ref_loss)), abs(float(loss_t) - float(ref_loss))
    e_dx_k = float((xk.grad[:, :D].double().cpu() - ref_dx).abs().max())
    e_dx_t = float((xt.grad[:, :D].double().cpu() - ref_dx).abs().max())
    print(f"{what}: loss {float(ref_loss):.9g}  |err| kernel {e_loss_k:.3e} torch-fp32 {e_loss_t:.3e};  "
          f"max|dx| {float(ref_dx.abs().max()):.3e}  max|err| kernel {e_dx_k:.3e} torch-fp32 {e_dx_t:.3e}")
    assert e_loss_k <= 2.0 * e_loss_t, (what, e_loss_k, e_loss_t)
    assert e_dx_k <= 2.0 * e_dx_t, (what, e_dx_k, e_dx_t)
    nofg = (lab < 0).unsqueeze(1).expand(-1, D, -1, -1)
    assert float(xk.grad[:, :D][nofg].abs().max()) == 0.0                # exact zeros where there is no label
    return loss_k.detach(), xk.grad


@pytest.mark.parametrize("empty_image", [False, True])
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("D", [3, 64, 65, 112])
def test_loss_forward_backward_vs_float64(hip_lib, D, channels_last, empty_image):
    feat, lab = _loss_case(D, channels_last, empty_image)
    _check_loss(feat, lab, D, f"D={D} {'NHWC' if channels_last else 'NCHW'}{' image 0 empty' if empty_image else ''}")


@pytest.mark.parametrize("channels_last", [False, True])
def test_loss_clamps(hip_lib, channels_last):
    """+-80 on the labelled bin and on another bin: log p and log(1 - p) reach binary_cross_entropy's -100 clamp, (1 - p) p its
    1e-12 clamp.  Pixels cycle through the four combinations; the rest stay ordinary."""
    D = 64
    feat, lab = _loss_case(D, channels_last, False, seed=1)
    lab[:, ::2, ::3] = 5
    other = 9
    for k, (vl, vo) in enumerate(((-80.0, 80.0), (80.0, -80.0), (80.0, 80.0), (-80.0, -80.0))):
        feat[:, 5, k::8, ::3] = vl
        feat[:, other, k::8, ::3] = vo
    loss, dx = _check_loss(feat, lab, D, f"clamps {'NHWC' if channels_last else 'NCHW'}")
    assert float(loss) > 10.0                                            # the clamped terms are in it


def test_loss_without_foreground_and_repeat(hip_lib):
    from unidistill_amd.ops import depth_sup
    D = 112
    feat, lab = _loss_case(D, True, False)
    x = feat.clone().requires_grad_(True)
    loss = depth_sup.depth_loss(x[:, :D], torch.full_like(lab, -1))
    loss.backward()
    assert float(loss) == 0.0 and float(x.grad.abs().max()) == 0.0
    runs = []
    for _ in range(2):
        x = feat.clone().requires_grad_(True)
        loss = depth_sup.depth_loss(x[:, :D], lab)
        (loss * 3.0).backward()
        runs.append((loss.detach().clone(), x.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # bf16 logits are widened, the gradient comes back in bf16
    xb = feat[:, :D].bfloat16().requires_grad_(True)
    lb = depth_sup.depth_loss(xb, lab)
    lb.backward()
    assert xb.grad.dtype == torch.bfloat16 and abs(float(lb) - float(runs[0][0])) < 0.05 * float(runs[0][0])


# ---- 8. through the model ---------------------------------------------------------------------------------------------------
def _model_batch(g):
    """The shrunk camera detector's golden batch plus a LiDAR cloud that hits its images: points built with the forward chain
    on 60 % of the feature cells at random depths, and a random cloud around them."""
    import test_model_step_gpu as T
    b = T._batch(g)
    B, ncam = g["sensor2ego"].shape[:2]
    H, W = T.S.IMG_DIM
    rng = syn.rng(5)
    v, u = np.meshgrid((np.arange(H // 16) + 0.5) * 16, (np.arange(W // 16) + 0.5) * 16, indexing="ij")
    clouds = []
    for s in range(B):
        parts = [syn.lidar_cloud(rng, 2000, 1)[:, :5]]
        for c in range(ncam):
            pick = rng.random(u.size) < 0.6
            xyz = R.frustum_points(g["sensor2ego"][s, c], g["intrin"][s, c], g["ida"][s, c], g["bda"][s],
                                   u.ravel()[pick], v.ravel()[pick], rng.uniform(2.5, 13.5, int(pick.sum())))
            parts.append(np.concatenate([xyz, np.zeros((len(xyz), 2))], 1).astype(np.float32))
        clouds.append(np.concatenate(parts, 0))
    b["points"] = torch.from_numpy(syn.pad_clouds(clouds)).cuda()
    return b


def test_detect_step_with_depth_supervision(golden, hip_lib, lenient):
    import test_model_step_gpu as T
    from unidistill_amd import train
    from unidistill_amd.ops import depth_sup
    g = golden("model_step")
    model = T._model(g, "student")
    batch = _model_batch(g)
    enc = model.camera_encoder.backbone
    D = enc.depth_channels
    depth_w = enc.depth_net[0].weight
    # Head parameters to compare bit for bit: the one-dimensional ones (biases, BatchNorm scales), whose gradients are fixed-order
    # reductions.  At these shrunk widths the convolutions run in the library (lenient), and its weight gradients differ in the
    # last bits from one run to the next even without the depth loss, so they can say nothing here; the two runs without the
    # loss below establish that the compared gradients do reproduce.
    head_ps = [p for p in model.det_head.dense_head.parameters() if p.requires_grad and p.dim() == 1]
    captured = []
    hook = enc.depth_net.register_forward_hook(lambda m, i, o: captured.append(o))

    def run(weight):
        step = train.DetectStep(model=model, depth_weight=weight).cuda().train()
        model.zero_grad(set_to_none=True)
        captured.clear()
        out = step(batch)
        out["loss"].backward()
        return out, depth_w.grad.clone(), [p.grad.clone() for p in head_ps if p.grad is not None]
    run(None)
    out0, gd0, gh0 = run(None)
    out0b, gd0b, gh0b = run(None)
    assert "loss_depth" not in out0["tb"] and torch.equal(out0["loss"], out0b["loss"])
    assert len(gh0) >= 2 and all(torch.equal(a, b) for a, b in zip(gh0, gh0b)) and any(float(a.abs().max()) > 0 for a in gh0)
    out3, gd3, gh3 = run(3.0)
    hook.remove()
    label = enc.lidar_depth_labels(batch["points"], batch["mats_dict"])[1]
    assert int((label >= 0).sum()) > 20
    ld = out3["tb"]["loss_depth"]
    assert float(ld) > 0.0
    assert torch.equal(ld, depth_sup.depth_loss(captured[-1].detach()[:, :D], label))          # the same kernel: bitwise
    want = out0["loss"].detach() + 3.0 * ld
    assert abs(float(out3["loss"]) - float(want)) <= 2.0 ** -22 * max(abs(float(want)), 3.0 * float(ld))
    assert not torch.allclose(gd0, gd3, rtol=1e-3, atol=0.0)
    # the depth loss reaches the head only through the shared image-branch weights: its gradients are the None run's, bit for bit
    assert len(gh0) == len(gh3) and all(torch.equal(a, b) for a, b in zip(gh0, gh3))
    # a camera-only batch cannot be depth-supervised
    no_points = {k: v for k, v in batch.items() if k != "points"}
    with pytest.raises(ValueError, match="points"):
        train.DetectStep(model=model, depth_weight=3.0).cuda().train()(no_points)


def test_distill_step_with_depth_supervision_two_streams(golden, hip_lib, lenient):
    import test_model_step_gpu as T
    from unidistill_amd import train
    g = golden("model_step")
    step = train.DistillStep("camera_exp_distill_lidar", student=T._model(g, "student"), teacher=T._model(g, "teacher"),
                             geometry=T.S.GEOMETRY, depth_weight=3.0)
    assert step.overlap_teacher
    step.cuda().train()
    batch = _model_batch(g)
    out = step(batch)
    out["loss"].backward()
    torch.cuda.synchronize()
    assert torch.isfinite(out["loss"]) and float(out["tb"]["loss_depth"]) > 0.0
    assert step.model.camera_encoder.backbone.depth_net[0].weight.grad is not None
    with pytest.raises(ValueError, match="points"):
        step({k: v for k, v in batch.items() if k != "points"})
