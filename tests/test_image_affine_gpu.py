"""GPU: ud_image_affine (ImageAffineTransformation on the device) is bit-exact to the reference's PIL pipeline --
against the golden (tests/golden/image_affine.npz, from the reference's img_transform on Pillow), against Pillow
directly over seeded draws, fused with ImageNormalize, batched with per-frame parameters, through collate_fn and
through one distillation step."""
import numpy as np
import pytest
import torch

import oracle
from test_image_affine_cpu import IDA_CONF, N_DRAWS, emulate, frame, sha, unpack_augs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cases(g):
    augs = unpack_augs(g, "case")
    frames = np.stack([frame(int(i)) for i in g["case_frame"]])
    outs = np.stack([g[f"case{k}_out"] for k in range(len(augs))])
    return frames, augs, outs


def test_golden_cases_bit_exact(hip_lib, golden):
    from unidistill_amd.ops import input_prep as ip
    g = golden("image_affine")
    frames, augs, outs = _cases(g)
    x = torch.from_numpy(frames).to(DEV)
    y, mats = ip.image_affine(x, augs, normalize=False)
    assert y.dtype == torch.uint8 and y.shape == outs.shape
    for k in range(len(augs)):
        assert np.array_equal(y[k].cpu().numpy(), outs[k]), k
    np.testing.assert_array_equal(mats, g["case_ida_mat"])
    assert torch.equal(x.cpu(), torch.from_numpy(frames))                            # input untouched


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_golden_draws_bit_exact(hip_lib, golden, mode):
    from unidistill_amd.ops import input_prep as ip
    g = golden("image_affine")
    augs = unpack_augs(g, mode)
    x = torch.from_numpy(np.stack([frame(i) for i in range(N_DRAWS)])).to(DEV)
    y, mats = ip.image_affine(x, augs, normalize=False)
    got = [sha(y[i].cpu().numpy()) for i in range(N_DRAWS)]
    assert got == [str(h) for h in g[mode + "_out_sha256"]]
    np.testing.assert_array_equal(mats, g[mode + "_ida_mat"])


def test_seeded_draws_bit_exact_vs_pillow(hip_lib):
    Image = pytest.importorskip("PIL.Image")
    from unidistill_amd.ops import input_prep as ip
    np.random.seed(7)
    torch.manual_seed(7)
    t = ip.ImageAffineTransformation(True, **IDA_CONF)
    augs = [t.sample_augs() for _ in range(50)]
    for r, dims in ((0.386, (617, 347)), (0.55, (880, 495))):                  # both resize endpoints
        for flip in (False, True):
            for ang in (0.0, 5.4, -5.4):
                cw = max(0, dims[0] - 704) // 2
                augs.append((r, dims, (cw, dims[1] - 256, cw + 704, dims[1]), flip, ang))
    augs.append(ip.ImageAffineTransformation(False, **IDA_CONF).sample_augs())  # eval
    assert any(a[3] for a in augs[:50]) and not all(a[3] for a in augs[:50])
    src = torch.randint(0, 256, (len(augs), 900, 1600, 3), dtype=torch.uint8)
    src[:, :, 200:260] = 255                                                     # saturated edges hit the clamp
    src[:, :, 260:300] = 0
    y, _ = ip.image_affine(src.to(DEV), augs, normalize=False)
    y = y.cpu().numpy()
    for i, a in enumerate(augs):
        img = Image.fromarray(src[i].numpy()).resize(a[1]).crop(a[2])
        if a[3]:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        ref = np.asarray(img.rotate(a[4]))
        assert np.array_equal(y[i], ref), (i, a)


def test_transposes_bit_exact_vs_pillow(hip_lib):
    """Pillow rotates by 180 degrees, and by 90 / 270 on square images, through transposes; the kernel takes them as
    integer maps (rotate_constants).  Both against Pillow itself, square and non-square crops."""
    Image = pytest.importorskip("PIL.Image")
    from unidistill_amd.ops import input_prep as ip
    torch.manual_seed(13)
    src = torch.randint(0, 256, (900, 1600, 3), dtype=torch.uint8)
    cases = [((256, 256), (0.3, (480, 270), (100, 14, 356, 270), flip, ang))
             for flip in (False, True) for ang in (90.0, 270.0, -90.0, 180.0, 450.0)]
    cases += [((256, 704), (0.47, (752, 423), (20, 167, 724, 423), flip, 180.0)) for flip in (False, True)]
    for fdim, a in cases:
        y, _ = ip.image_affine(src.to(DEV), [a], final_dim=fdim, normalize=False)
        img = Image.fromarray(src.numpy()).resize(a[1]).crop(a[2])
        if a[3]:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        assert np.array_equal(y.cpu().numpy(), np.asarray(img.rotate(a[4]))), (fdim, a)


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("to_rgb", [True, False])
def test_fused_normalize_bit_identical(hip_lib, golden, channels_last, to_rgb):
    from unidistill_amd.ops import input_prep as ip
    g = golden("image_affine")
    frames, augs, outs = _cases(g)
    x = torch.from_numpy(frames).to(DEV)
    u8, _ = ip.image_affine(x, augs, normalize=False)
    want = ip.image_normalize(u8, to_rgb=to_rgb, channels_last=channels_last)
    got, _ = ip.image_affine(x, augs, normalize=True, to_rgb=to_rgb, channels_last=channels_last)
    assert got.shape == (len(augs), 3, 256, 704) and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    if channels_last:
        assert got.is_contiguous(memory_format=torch.channels_last)
    ref = np.moveaxis(oracle.image_normalize(outs, ip.IMG_MEAN, ip.IMG_STD, to_rgb), -1, -3)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), np.ascontiguousarray(ref).view(np.int32))


def test_one_launch_equals_frame_by_frame(hip_lib):
    from unidistill_amd.ops import input_prep as ip
    np.random.seed(11)
    t = ip.ImageAffineTransformation(True, **IDA_CONF)
    B, S, Ncam = 2, 1, 3
    frames = np.stack([frame(i) for i in range(B * S * Ncam)]).reshape(B, S, Ncam, 900, 1600, 3)
    augs = [[[t.sample_augs() for _ in range(Ncam)] for _ in range(S)] for _ in range(B)]
    x = torch.from_numpy(frames).to(DEV)
    before = x.clone()
    y, mats = ip.image_affine(x, augs)
    assert y.shape == (B, S, Ncam, 3, 256, 704) and mats.shape == (B, S, Ncam, 4, 4)
    for b in range(B):
        for c in range(Ncam):
            yi, mi = ip.image_affine(x[b, 0, c], [augs[b][0][c]])            # one frame, no leading dims
            assert torch.equal(y[b, 0, c], yi) and np.array_equal(mats[b, 0, c], mi)
    ya, ma = t.apply(x, augs)                                                  # the transform's device entry
    assert torch.equal(ya, y) and np.array_equal(ma, mats)
    assert torch.equal(x, before)


def test_edge_cases(hip_lib):
    from unidistill_amd.ops import input_prep as ip
    torch.manual_seed(3)
    # identity size: no resample (and a 180-degree rotation: Pillow's transpose)
    small = torch.randint(0, 256, (48, 64, 3), dtype=torch.uint8)
    for ang in (0.0, 180.0, 3.0):
        a = (1.0, (64, 48), (0, 0, 64, 48), False, ang)
        y, _ = ip.image_affine(small.to(DEV), [a], final_dim=(48, 64), normalize=False)
        want = emulate(small.numpy(), a, (48, 64))
        assert np.array_equal(y.cpu().numpy(), want), ang
        if ang == 0.0:
            assert np.array_equal(want, small.numpy())
    # tables planned for the host first (same sizes) must not be handed to the device: the cache is per device
    aug0 = (0.44, (704, 396), (0, 140, 704, 396), False, 1.5)
    ip.plan_frames([aug0], 900, 1600, (256, 704), torch.device("cpu"))
    y, _ = ip.image_affine_host_frames(frame(7), [aug0], "cuda", normalize=False)
    assert np.array_equal(y.cpu().numpy(), emulate(frame(7), aug0))
    # a crop wholly outside the resized image: all fill
    src = torch.from_numpy(frame(5)).to(DEV)
    out = (0.44, (704, 396), (2000, 0, 2704, 256), False, 2.0)
    y, _ = ip.image_affine(src, [out], normalize=False)
    assert int(y.sum()) == 0
    yn, _ = ip.image_affine(src, [out])
    zero = ip.image_normalize(torch.zeros(256, 704, 3, dtype=torch.uint8, device=DEV))
    assert torch.equal(yn, zero)
    # non-contiguous inputs: rows of a wider buffer, every other frame
    aug = (0.5, (800, 450), (40, 194, 744, 450), True, -3.0)
    wide = torch.zeros(2, 900, 1616, 3, dtype=torch.uint8)
    wide[:, :, 8:1608] = torch.from_numpy(frame(6))
    view = wide.to(DEV)[:, :, 8:1608]
    assert not view.is_contiguous()
    y_view, _ = ip.image_affine(view, [aug, aug], normalize=False)
    y_cont, _ = ip.image_affine(view.contiguous(), [aug, aug], normalize=False)
    assert torch.equal(y_view, y_cont)
    assert np.array_equal(y_view[1].cpu().numpy(), emulate(frame(6), aug))
    stack = torch.from_numpy(np.stack([frame(i) for i in range(4)])).to(DEV)
    y_step, _ = ip.image_affine(stack[::2], [aug, aug], normalize=False)
    y_ref, _ = ip.image_affine(stack[::2].contiguous(), [aug, aug], normalize=False)
    assert torch.equal(y_step, y_ref)
    with pytest.raises(ValueError):                                              # pixels not dense (RGBA view)
        ip.image_affine(torch.zeros(900, 1600, 4, dtype=torch.uint8, device=DEV)[..., :3], [aug])
    with pytest.raises(ValueError):
        ip.image_affine(torch.zeros(900, 1600, 3, dtype=torch.float32, device=DEV), [aug])
    with pytest.raises(ValueError):
        ip.image_affine(src, [aug, aug])


def test_collate_raw_frames_match_reference_pipeline(hip_lib, golden):
    """PIL -> ImageNormalize -> collate (the golden's outputs through the oracle's mmcv restatement) vs raw frames
    through collate_fn: bit-equal imgs and ida_mats.  Also with the augs drawn by the transform in collate_fn."""
    from unidistill_amd.ops import input_prep as ip
    g = golden("image_affine")
    frames, augs, outs = _cases(g)
    n = len(augs)
    data = [{"imgs_raw": frames[None], "ida_aug": [augs], "gt_boxes": np.zeros((2, 9), np.float32),
             "gt_labels": np.zeros(2)}]
    out = ip.collate_fn(data, device=DEV)
    ref = np.moveaxis(oracle.image_normalize(outs, ip.IMG_MEAN, ip.IMG_STD, True), -1, -3)[None, None]
    assert out["imgs"].shape == (1, 1, n, 3, 256, 704)
    np.testing.assert_array_equal(out["imgs"].cpu().numpy().view(np.int32), np.ascontiguousarray(ref).view(np.int32))
    ida = out["mats_dict"]["ida_mats"]
    assert ida.dtype == torch.float32 and ida.shape == (1, 1, n, 4, 4)
    np.testing.assert_array_equal(ida.cpu().numpy(), g["case_ida_mat"].astype(np.float32)[None, None])
    # augs drawn in collate_fn, seeded: the reference's draws
    np.random.seed(20231016)
    t = ip.ImageAffineTransformation(True, **IDA_CONF)
    raw = np.stack([frame(i) for i in range(6)]).reshape(1, 6, 900, 1600, 3)
    out2 = ip.collate_fn([{"imgs_raw": raw}], device=DEV, ida_transform=t)
    np.testing.assert_array_equal(out2["mats_dict"]["ida_mats"].cpu().numpy()[0, 0],
                                  g["train_ida_mat"][:6].astype(np.float32))
    y, _ = ip.image_affine(torch.from_numpy(raw).to(DEV), unpack_augs(g, "train")[:6])
    assert torch.equal(out2["imgs"][0], y)


def test_distill_step_same_losses_both_routes(hip_lib, golden):
    """One fp32 DistillStep at B = 1: raw frames through the new collate_fn path vs the golden's PIL outputs through
    the existing imgs_u8 path give bit-equal losses."""
    from unidistill_amd import train
    from unidistill_amd.ops import input_prep as ip
    g = golden("image_affine")
    frames, augs, outs = _cases(g)
    dev = torch.device(DEV)
    torch.manual_seed(0)
    np.random.seed(0)
    step = train.DistillStep("camera_exp_distill_lidar")
    tr = train.Trainer(step, device=dev, channels_last=True)
    base = train.synthetic_batch(dev, 1, ncam=len(augs))
    extra = {"points": base["points"][0].cpu().numpy(), "gt_boxes": base["gt_boxes"][0].cpu().numpy(),
             "gt_labels": base["gt_labels"][0].cpu().numpy(),
             "mats_dict": {k: v[0].cpu().numpy() for k, v in base["mats_dict"].items()}}
    r1 = ip.collate_fn([dict(extra, imgs_raw=frames[None], ida_aug=[augs])], device=dev)
    mats2 = dict(extra["mats_dict"], ida_mats=g["case_ida_mat"][None])
    r2 = ip.collate_fn([dict(extra, imgs_u8=outs[None], mats_dict=mats2)], device=dev)
    assert torch.equal(r1["imgs"], r2["imgs"])
    assert torch.equal(r1["mats_dict"]["ida_mats"], r2["mats_dict"]["ida_mats"])
    losses = []
    for batch in (r1, r2):
        out = tr.module(batch)
        torch.cuda.synchronize()
        losses.append({k: v.detach().cpu() for k, v in out.items() if torch.is_tensor(v) and v.numel() == 1})
    assert losses[0].keys() == losses[1].keys() and "loss" in losses[0]
    for k in losses[0]:
        assert torch.equal(losses[0][k], losses[1][k]), k
        assert torch.isfinite(losses[0][k]).all(), k
