"""GPU: ud_jpeg_decode / ops.jpeg.jpeg_decode against the committed digests of Pillow's decode, the
failure status of broken frames, and the imgs_jpeg collate route against the imgs_raw route."""
import hashlib
import io
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

JDIR = os.path.join(GOLDEN, "jpeg")
MANIFEST = json.load(open(os.path.join(JDIR, "manifest.json")))
SUPPORTED = sorted(k for k, v in MANIFEST.items() if v["supported"])
BIG = sorted(k for k in SUPPORTED if MANIFEST[k]["shape"][:2] == [900, 1600])


def load(name):
    with open(os.path.join(JDIR, name + ".jpg"), "rb") as fh:
        return fh.read()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def pillow(data):
    try:
        from PIL import Image
    except ImportError:
        return None
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def check_frame(name, got):
    """got (uint8 [H, W, 3] host) equals Pillow's decode: the committed digest, with a readable diff when Pillow or
    the full array is at hand."""
    if sha(got) == MANIFEST[name]["sha256"]:
        return
    ref = pillow(load(name))
    if ref is None:
        small = np.load(os.path.join(JDIR, "small.npz"))
        ref = small[name] if name in small.files else None
    msg = f"{name}: decode differs from Pillow's (digest)"
    if ref is not None and ref.shape == got.shape:
        bad = np.argwhere(ref != got)
        msg += f"; {len(bad)} values differ, first {bad[:4].tolist()}, max |d| {np.abs(ref.astype(int) - got).max()}"
    raise AssertionError(msg)


def corrupt_code(data):
    """The same file with 24 bytes of its scan replaced by stuffed FF bytes: all-ones bits, never a valid code."""
    from unidistill_amd.ops import jpeg
    rc, rec = jpeg.parse(data)
    assert rc == jpeg.OK
    mid = rec.ecs_off + rec.ecs_bytes // 2
    mid -= (mid - rec.ecs_off) % 2
    b = bytearray(data)
    while b[mid - 1] == 0xFF:                   # do not split a stuffed pair or a marker
        mid += 1
    b[mid:mid + 24] = b"\xff\x00" * 12
    return bytes(b)


@pytest.fixture(scope="module")
def dev(hip_lib):
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SUPPORTED)
def test_fixture_bit_exact(dev, name):
    from unidistill_amd.ops import jpeg
    out, status = jpeg.jpeg_decode([load(name)], dev)
    assert status.cpu().tolist() == [0]
    check_frame(name, out[0].cpu().numpy())


@pytest.mark.gpu
def test_mixed_batch_24_frames(dev):
    """24 frames of 1600x900: every quality, sampling mode and restart setting of the big fixtures, in a mixed order."""
    from unidistill_amd.ops import jpeg
    names = [BIG[(7 * i + i // len(BIG)) % len(BIG)] for i in range(24)]
    before = dict(jpeg.STATS)
    out, status = jpeg.jpeg_decode([load(n) for n in names], dev)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * 24
    assert jpeg.STATS["frames"] - before["frames"] == 24 and jpeg.STATS["fallback"] == before["fallback"]
    rounds = jpeg.STATS["last_sync_iters"].cpu().numpy()
    assert (rounds >= 1).all()
    host = out.cpu().numpy()
    for i, n in enumerate(names):
        check_frame(n, host[i])


@pytest.mark.gpu
def test_broken_frames_set_status_neighbours_exact(dev):
    from unidistill_amd.ops import jpeg
    good = ["s3_q75_420_odd", "s3_q75_420_odd", "s3_q75_420_odd"]
    data = load(good[0])
    truncated = data[:len(data) * 2 // 3]
    broken = corrupt_code(data)
    out, status = jpeg.jpeg_decode([data, truncated, data, broken, data], dev)
    st = status.cpu().numpy()
    assert st[0] == 0 and st[2] == 0 and st[4] == 0
    assert st[1] != 0 and st[3] != 0, st
    assert st[3] & jpeg.ST_CODE, st
    host = out.cpu().numpy()
    for i in (0, 2, 4):
        check_frame(good[0], host[i])
    assert not host[1].any() and not host[3].any()


@pytest.mark.gpu
def test_restart_corruption_in_one_segment(dev):
    """A broken code inside a restart-interval frame marks that frame; the frame next to it in the batch is exact."""
    from unidistill_amd.ops import jpeg
    d = load("s0_q90_422_rst_blocks")
    out, status = jpeg.jpeg_decode([corrupt_code(d), d], dev)
    st = status.cpu().numpy()
    assert st[0] != 0 and st[1] == 0
    check_frame("s0_q90_422_rst_blocks", out[1].cpu().numpy())


@pytest.mark.gpu
def test_repeatable_and_on_input_stream(dev):
    from unidistill_amd.ops import jpeg
    from unidistill_amd.ops.input_prep import input_stream
    files = [load(n) for n in BIG[:3]]
    a, sa = jpeg.jpeg_decode(files, dev)
    pre = torch.zeros_like(a)
    b, sb = jpeg.jpeg_decode(files, dev, out=pre)
    assert b.data_ptr() == pre.data_ptr()
    assert torch.equal(a, b) and torch.equal(sa, sb)
    # the work is on the input stream: from a side stream, the result is ordered behind it for the caller
    side = torch.cuda.Stream(device=dev)
    assert input_stream(dev) != side
    with torch.cuda.stream(side):
        c, _ = jpeg.jpeg_decode(files, dev)
        same = torch.equal(a, c)
    assert same


@pytest.mark.gpu
def test_out_is_ordered_after_the_callers_stream(dev):
    """A caller-supplied out still being written on the caller's stream (a long kernel, then a fill) is decoded into
    only after that work: the decode on the input stream waits for the caller's stream first."""
    from unidistill_amd.ops import jpeg
    files = [load(n) for n in BIG[:2]]
    ref, _ = jpeg.jpeg_decode(files, dev)
    torch.cuda.synchronize()
    out = torch.empty_like(ref)
    torch.cuda._sleep(50_000_000)               # keeps the caller's stream busy for tens of ms
    out.fill_(7)                                # queued behind the sleep
    got, st = jpeg.jpeg_decode(files, dev, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert not st.cpu().any()
    assert torch.equal(got, ref)


@pytest.mark.gpu
def test_bytes_after_eoi_decode_exact(dev):
    """Padding and data after EOI are ignored, as Pillow ignores them; the frame and its neighbour stay exact."""
    from unidistill_amd.ops import jpeg
    d = load("s3_q75_420_odd")
    padded = d + b"\x00" * 1000 + b"\xff\xd9\xff\xd8trailing bytes\xff"
    out, status = jpeg.jpeg_decode([padded, d], dev)
    assert status.cpu().tolist() == [0, 0]
    host = out.cpu().numpy()
    check_frame("s3_q75_420_odd", host[0])
    check_frame("s3_q75_420_odd", host[1])
    ref = pillow(padded)
    if ref is not None:
        assert np.array_equal(host[0], ref)


@pytest.mark.gpu
def test_mixed_sizes_raise_and_fallback_counts(dev):
    from unidistill_amd.ops import jpeg
    with pytest.raises(ValueError, match="share H x W"):
        jpeg.jpeg_decode([load("f5_q50_420_17x9"), load("f8_q90_420_8x8")], dev)
    if pillow(load("reject_progressive")) is None:
        with pytest.raises(ValueError, match="Pillow"):
            jpeg.jpeg_decode([load("reject_progressive")], dev)
        return
    before = jpeg.STATS["fallback"]
    prog = load("reject_progressive")
    out, status = jpeg.jpeg_decode([prog, load("reject_gray")], dev)
    assert jpeg.STATS["fallback"] == before + 2
    assert status.cpu().tolist() == [0, 0]
    assert np.array_equal(out[0].cpu().numpy(), pillow(prog))
    check_frame("reject_gray", out[1].cpu().numpy())


# ---- collate ---------------------------------------------------------------------------------------------------
CONF = dict(resize_lim=(0.386, 0.55), final_dim=(256, 704), rot_lim=(-5.4, 5.4), H=900, W=1600, rand_flip=True,
            bot_pct_lim=(0.0, 0.0))


def _batch(dev):
    """B = 2, 1 sweep x 3 cameras of 1600x900 JPEGs and the same frames decoded (checked against the digests)."""
    from unidistill_amd.ops import jpeg
    names = [[BIG[(3 * b + c) % len(BIG)] for c in range(3)] for b in range(2)]
    files = [[[load(n) for n in cams]] for cams in names]
    dec, st = jpeg.jpeg_decode([load(n) for cams in names for n in cams], dev)
    assert not st.cpu().any()
    host = dec.cpu().numpy()
    for i, n in enumerate(n for cams in names for n in cams):
        check_frame(n, host[i])                 # from here on these ARE Pillow's frames
    raw = host.reshape(2, 1, 3, 900, 1600, 3)
    return files, raw


@pytest.mark.gpu
def test_collate_jpeg_equals_raw_route(dev):
    from unidistill_amd.ops import input_prep as ip
    files, raw = _batch(dev)
    t = ip.ImageAffineTransformation(is_train=True, **CONF)
    np.random.seed(3)
    augs = [[[t.sample_augs() for _ in range(3)]] for _ in range(2)]
    a = ip.collate_fn([{"imgs_jpeg": files[b], "ida_aug": augs[b]} for b in range(2)], device=dev, with_points=False)
    r = ip.collate_fn([{"imgs_raw": raw[b], "ida_aug": augs[b]} for b in range(2)], device=dev, with_points=False)
    assert a["imgs"].dtype == torch.float32 and a["imgs"].shape == (2, 1, 3, 3, 256, 704)
    assert torch.equal(a["imgs"], r["imgs"])
    assert torch.equal(a["mats_dict"]["ida_mats"], r["mats_dict"]["ida_mats"])
    # uint8: the decoded frames through image_affine without normalisation, against the host-frame route
    from unidistill_amd.ops import jpeg
    flat = [f for s in files for cams in s for f in cams]
    dec, _ = jpeg.jpeg_decode(flat, dev)
    fa = [x for s in augs for cams in s for x in cams]
    u8a, ma = ip.image_affine(dec, fa, final_dim=(256, 704), normalize=False)
    u8r, mr = ip.image_affine_host_frames(raw.reshape(6, 900, 1600, 3), fa, dev, final_dim=(256, 704), normalize=False)
    assert u8a.dtype == torch.uint8 and torch.equal(u8a, u8r) and np.array_equal(ma, mr)


@pytest.mark.gpu
def test_collate_jpeg_draws_from_transform_and_reports_failures(dev):
    from unidistill_amd.ops import input_prep as ip
    files, raw = _batch(dev)
    t = ip.ImageAffineTransformation(is_train=True, **CONF)
    np.random.seed(11)
    a = ip.collate_fn([{"imgs_jpeg": files[b]} for b in range(2)], device=dev, ida_transform=t)
    np.random.seed(11)
    r = ip.collate_fn([{"imgs_raw": raw[b]} for b in range(2)], device=dev, ida_transform=t)
    assert torch.equal(a["imgs"], r["imgs"]) and torch.equal(a["mats_dict"]["ida_mats"], r["mats_dict"]["ida_mats"])
    bad = [[list(cams) for cams in s] for s in files]
    bad[1][0][2] = corrupt_code(bad[1][0][2])
    with pytest.raises(ValueError, match="sample 1 sweep 0 camera 2"):
        ip.collate_fn([{"imgs_jpeg": bad[b]} for b in range(2)], device=dev, ida_transform=t)


@pytest.mark.gpu
def test_distill_step_loss_identical_between_routes(dev):
    """One fp32 DistillStep at B = 1 (6 cameras) fed by the imgs_jpeg route and by the imgs_raw route with the same
    frames decoded: bit-equal losses."""
    from unidistill_amd import train
    from unidistill_amd.ops import input_prep as ip
    from unidistill_amd.ops import jpeg
    names = [BIG[i % len(BIG)] for i in range(6)]
    files = [load(n) for n in names]
    dec, st = jpeg.jpeg_decode(files, dev)
    assert not st.cpu().any()
    raw = dec.cpu().numpy()
    for i, n in enumerate(names):
        check_frame(n, raw[i])
    t = ip.ImageAffineTransformation(is_train=True, **CONF)
    np.random.seed(7)
    augs = [t.sample_augs() for _ in range(6)]
    torch.manual_seed(0)
    np.random.seed(0)
    step = train.DistillStep("camera_exp_distill_lidar")
    tr = train.Trainer(step, device=dev, channels_last=True)
    base = train.synthetic_batch(dev, 1, ncam=6)
    extra = {"points": base["points"][0].cpu().numpy(), "gt_boxes": base["gt_boxes"][0].cpu().numpy(),
             "gt_labels": base["gt_labels"][0].cpu().numpy(),
             "mats_dict": {k: v[0].cpu().numpy() for k, v in base["mats_dict"].items()}}
    r1 = ip.collate_fn([dict(extra, imgs_jpeg=[files], ida_aug=[augs])], device=dev)
    r2 = ip.collate_fn([dict(extra, imgs_raw=raw[None], ida_aug=[augs])], device=dev)
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
