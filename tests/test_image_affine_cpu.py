"""CPU: the host side of the device ImageAffineTransformation (ops/input_prep.py) against the reference golden
tests/golden/image_affine.npz -- seeded parameter draws, float64 ida_mats, and the resampling tables / rotation constants
that drive ud_image_affine: a numpy evaluation of exactly the integer arithmetic the kernels do reproduces the golden's PIL
outputs bit for bit.  Bad inputs raise.

The golden comes from the reference's own ImageAffineTransformation.sample_augs + functional.img_transform (on the stand-ins
of tests/golden/_ref_import.py) and Pillow.  Regenerate it where the reference tree and Pillow are available:
    UNIDISTILL_REF=<reference checkout> python tests/test_image_affine_cpu.py
Source frames are a closed-form integer pattern (``frame``), not an RNG stream; the golden stores their SHA-256."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
IDA_CONF = dict(resize_lim=(0.386, 0.55), final_dim=(256, 704), rot_lim=(-5.4, 5.4), H=900, W=1600, rand_flip=True,
                bot_pct_lim=(0.0, 0.0))                                          # base_nuscenes_cfg.py ida_aug_cfg
N_DRAWS, SEED = 24, 20231016
# full-output cases: (frame index, augs); eval, resize 0.386 (617 px wide: the crop runs past the right edge), flip,
# +5.4 and -5.4 degrees
CASES = [(0, None),
         (1, (0.386, (617, 347), (0, 91, 704, 347), False, 0.0)),
         (2, (0.5, (800, 450), (40, 194, 744, 450), True, 0.0)),
         (3, (0.55, (880, 495), (88, 239, 792, 495), False, 5.4)),
         (4, (0.47, (752, 423), (20, 167, 724, 423), True, -5.4))]


def frame(i, H=900, W=1600):
    """Closed-form uint8 RGB test frame: saturated stripes (the negative bicubic lobes hit the clamp), fine
    texture and smooth gradients, in blocks that move with the frame index."""
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    y, x = y[..., None], x[..., None]
    c = np.arange(3, dtype=np.int64)
    region = (x // 97 + y // 61 + i) % 4
    stripes = np.where(((x // 3 + y // 2 + c) % 2) == 0, 255, 0)
    texture = (x * x + 3 * y * y + 7 * c + 31 * i) % 256
    smooth = ((x + 2 * y + 150 * c + 13 * i) * 255) // (W + 2 * H + 450 + 13 * 32)
    blocks = np.where((x % 97) < 48, 255 * (c != i % 3), 0)
    v = np.select([region == 0, region == 1, region == 2], [stripes, texture, smooth], blocks)
    return np.ascontiguousarray(v.astype(np.uint8))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def draws(ip_cls, is_train, n):
    """n parameter draws of an ImageAffineTransformation under np.random.seed(SEED)."""
    np.random.seed(SEED)
    t = ip_cls(is_train, **IDA_CONF)
    return [t.sample_augs() for _ in range(n)]


def pack_augs(augs):
    return (np.array([a[0] for a in augs], np.float64), np.array([a[1] for a in augs], np.int64),
            np.array([a[2] for a in augs], np.int64), np.array([a[3] for a in augs], bool),
            np.array([a[4] for a in augs], np.float64))


def unpack_augs(g, prefix):
    r, d, c, f, a = (g[prefix + k] for k in ("_resize", "_dims", "_crop", "_flip", "_rotate"))
    return [(float(r[i]), tuple(int(v) for v in d[i]), tuple(int(v) for v in c[i]), bool(f[i]), float(a[i]))
            for i in range(len(r))]


def case_augs(g, k):
    return unpack_augs(g, "case")[k]


def emulate(img, augs, final_dim=(256, 704)):
    """numpy evaluation of ud_image_affine's arithmetic from the host plan (tables + rotation constants)."""
    from unidistill_amd.ops import input_prep as ip
    H, W, _ = img.shape
    fH, fW = final_dim
    resize, (newW, newH), crop, flip, rotate = augs
    ht, vt = ip.resample_table(W, newW), ip.resample_table(H, newH)
    x = img.astype(np.int64)
    mid = np.empty((H, newW, 3), np.int64)
    for o in range(newW):
        lo, n = ht[o, 0], ht[o, 1]
        mid[:, o] = np.clip(((1 << 21) + np.einsum("k,hkc->hc", ht[o, 2:2 + n].astype(np.int64), x[:, lo:lo + n])) >> 22,
                            0, 255)
    res = np.empty((newH, newW, 3), np.int64)
    for o in range(newH):
        lo, n = vt[o, 0], vt[o, 1]
        res[o] = np.clip(((1 << 21) + np.einsum("k,kwc->wc", vt[o, 2:2 + n].astype(np.int64), mid[lo:lo + n])) >> 22,
                         0, 255)
    yy, xx = np.mgrid[0:fH, 0:fW]
    a = ip.rotate_constants(rotate, fW, fH)
    if a is None:
        xs, ys = xx, yy
    else:
        xs, ys = (a[2] + a[1] * yy + a[0] * xx) >> 16, (a[5] + a[4] * yy + a[3] * xx) >> 16
    ok = (xs >= 0) & (xs < fW) & (ys >= 0) & (ys < fH)
    if flip:
        xs = fW - 1 - xs
    xr, yr = crop[0] + xs, crop[1] + ys
    ok &= (xr >= 0) & (xr < newW) & (yr >= 0) & (yr < newH)
    out = np.zeros((fH, fW, 3), np.uint8)
    out[ok] = res[yr[ok], xr[ok]]
    return out


def test_frames_match_golden_digest(golden):
    g = golden("image_affine")
    for i, h in enumerate(g["frame_sha256"]):
        assert sha(frame(i)) == str(h), i


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_parameter_draws_and_ida_mats_match_reference(golden, mode):
    from unidistill_amd.ops import input_prep as ip
    g = golden("image_affine")
    got = draws(ip.ImageAffineTransformation, mode == "train", N_DRAWS)
    want = unpack_augs(g, mode)
    assert len(got) == len(want) == N_DRAWS
    for a, b in zip(got, want):
        assert (a[0], tuple(a[1]), tuple(a[2]), bool(a[3]), float(a[4])) == b        # exact float64 equality
    mats = np.stack([ip.ida_matrix(a[0], a[2], a[3], a[4]) for a in got])
    np.testing.assert_array_equal(mats.view(np.int64), g[mode + "_ida_mat"].view(np.int64))
    if mode == "eval":
        assert want[0] == (0.44, (704, 396), (0, 140, 704, 396), False, 0.0)


def test_loader_side_forward_draws_per_camera(golden):
    """forward(data_dict) draws per camera in dict order, like the reference, and leaves the frames raw."""
    from unidistill_amd.ops import input_prep as ip
    g = golden("image_affine")
    np.random.seed(SEED)
    t = ip.ImageAffineTransformation(True, **IDA_CONF)
    cams = [f"CAM_{k}" for k in range(6)]
    raw = {c: np.zeros((2, 2, 3), np.uint8) for c in cams}
    d = t.forward({"imgs": dict(raw)})
    want = unpack_augs(g, "train")
    for k, c in enumerate(cams):
        assert d["imgs"][c] is raw[c]
        a = d["ida_aug"][c]
        assert (a[0], tuple(a[1]), tuple(a[2]), bool(a[3]), float(a[4])) == want[k]
        np.testing.assert_array_equal(d["ida_mat"][c], g["train_ida_mat"][k])


@pytest.mark.parametrize("k", range(len(CASES)))
def test_tables_and_rotation_constants_reproduce_golden_cases(golden, k):
    g = golden("image_affine")
    out = emulate(frame(int(g["case_frame"][k])), case_augs(g, k))
    assert np.array_equal(out, g[f"case{k}_out"])


def test_tables_and_rotation_constants_reproduce_golden_digests(golden):
    """A few of the seeded training draws (the rest run on the GPU) through the same numpy evaluation."""
    g = golden("image_affine")
    augs = unpack_augs(g, "train")
    for i in (0, 7, 13):
        assert sha(emulate(frame(i), augs[i])) == str(g["train_out_sha256"][i]), i


def test_rotation_constants_and_tables_properties():
    from unidistill_amd.ops import input_prep as ip
    assert ip.rotate_constants(0, 704, 256) is None and ip.rotate_constants(360.0, 704, 256) is None
    assert ip.rotate_constants(180, 704, 256) == (-65536, 0, 703 << 16, 0, -65536, 255 << 16)
    a = ip.rotate_constants(5.4, 704, 256)
    assert all(isinstance(v, int) for v in a) and a[0] == a[4] and a[1] == -a[3]
    t = ip.resample_table(1600, 704)
    assert t.dtype == np.int32 and t.shape[0] == 704
    assert (t[:, 0] >= 0).all() and (t[:, 0] + t[:, 1] <= 1600).all()
    assert np.abs(t[:, 2:].sum(1) - (1 << 22)).max() <= t.shape[1]                 # normalised, then rounded per tap
    ident = ip.resample_table(37, 37)                                                # no resample: one unit tap
    assert all(ident[o, 2 + (o - ident[o, 0])] == 1 << 22 for o in range(37))


def test_bad_inputs_raise():
    from unidistill_amd.ops import image_affine, input_prep as ip
    good = (0.44, (704, 396), (0, 140, 704, 396), False, 0.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ip.image_affine(torch.zeros(900, 1600, 3, dtype=torch.uint8), [good])
    with pytest.raises(ValueError):                                                  # wrong crop size
        ip.plan_frames([(0.44, (704, 396), (0, 140, 700, 396), False, 0.0)], 900, 1600, (256, 704), torch.device("cpu"))
    with pytest.raises(ValueError):                                                  # not an augs tuple
        image_affine._flat_augs([1, 2, 3])
    with pytest.raises(ValueError):
        ip.resample_table(0, 5)
    with pytest.raises(ValueError):                                                  # host frames: dtype / shape
        ip.image_affine_host_frames(np.zeros((900, 1600, 3), np.float32), [good], "cuda")
    with pytest.raises(ValueError):
        ip.image_affine_host_frames(np.zeros((900, 1600, 4), np.uint8), [good], "cuda")
    with pytest.raises(ValueError):                                                  # augs count
        ip.image_affine_host_frames(np.zeros((2, 900, 1600, 3), np.uint8), [good], "cuda")
    with pytest.raises(RuntimeError, match="GPU only"):
        ip.image_affine_host_frames(np.zeros((900, 1600, 3), np.uint8), [good], "cpu")
    with pytest.raises(ValueError):
        ip.collate_fn([{"imgs_raw": np.zeros((1, 1, 900, 1600, 3), np.uint8)}], device="cuda")


def test_launcher_rejects_bad_records(hip_lib):
    """ud_image_affine's bounds check of the records is a pure host function (ud_image_affine_check, which the launcher
    runs before it launches anything): called here directly, so nothing can reach a kernel."""
    from unidistill_amd.ops import image_affine, input_prep as ip
    recs, bands, _ = ip.plan_frames([(0.44, (704, 396), (0, 140, 704, 396), False, 0.0)], 900, 1600, (256, 704),
                                    torch.device("cpu"))
    i = image_affine._FRAME_FIELDS.index
    recs[0, i("src_rows")] = 900
    ws_bytes = hip_lib.ud_image_affine_workspace_bytes(recs.ctypes.data, 1)
    assert ws_bytes >= bands[0][1] * 704 * 3 and ws_bytes == hip_lib.ud_image_affine_workspace_bytes(recs.ctypes.data, 1)

    def check(r, img_bytes=900 * 1600 * 3, ws=ws_bytes, fW=704):
        r = np.ascontiguousarray(r)
        return hip_lib.ud_image_affine_check(r.ctypes.data, 1, img_bytes, 900, 1600, 4800, 256, fW, ws)
    assert check(recs) == 0                                                          # the plan itself passes
    bad = recs.copy()
    bad[0, i("src_rows")] = 100                                                      # band not stored
    assert check(bad) == -1
    assert check(recs, img_bytes=1000) == -1                                         # rows beyond the input
    assert check(recs, ws=16) == -2                                                  # workspace too small
    bad = recs.copy()
    bad[0, i("col0")] = 700                                                          # crop columns past the image
    assert check(bad) == -1
    bad = recs.copy()
    bad[0, i("ws_off")] = 8                                                          # misaligned workspace region
    assert check(bad) == -1
    assert check(recs, fW=9000) == -1                                                # output too large for int32 maps
    # the launcher refuses null pointers before the check (nothing to launch with)
    assert hip_lib.ud_image_affine(None, 0, 900, 1600, 4800, recs.ctypes.data, None, 1, 256, 704, 0, None, None, None,
                                   1, None, 0, None) == -1


def test_loader_side_runs_in_reference_compose():
    """The loader-side transform binds where the reference's nn.Module sat: transforms3d.Compose runs
    ``data_dict = t(data_dict)`` for every transform.  Under the seed the draws are the reference's."""
    from unidistill_amd.ops import input_prep as ip
    g = np.load(os.path.join(HERE, "golden", "image_affine.npz"))
    np.random.seed(SEED)
    pipeline = [ip.ImageAffineTransformation(True, **IDA_CONF)]
    cams = [f"CAM_{k}" for k in range(6)]
    raw = {c: np.zeros((2, 2, 3), np.uint8) for c in cams}
    d = {"imgs": dict(raw)}
    for t in pipeline:                                                               # Compose.forward
        d = t(d)
    want = unpack_augs(g, "train")
    for k, c in enumerate(cams):
        assert d["imgs"][c] is raw[c]
        a = d["ida_aug"][c]
        assert (a[0], tuple(a[1]), tuple(a[2]), bool(a[3]), float(a[4])) == want[k]
        np.testing.assert_array_equal(d["ida_mat"][c], g["train_ida_mat"][k])
    assert pipeline[0]({"imgs": None}) == {"imgs": None}                            # no cameras: passed through


def write_golden(ref):
    """Reference side: ImageAffineTransformation.sample_augs + functional.img_transform on Pillow."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import _ref_import
    _ref_import.REF_ROOT = ref
    _ref_import.install()
    from PIL import Image
    from unidistill.data.multisensorfusion.transforms3d import ImageAffineTransformation
    from unidistill.data.multisensorfusion.functional import img_transform
    import PIL
    out = {"pillow_version": np.array(PIL.__version__)}
    n_frames = max(N_DRAWS, len(CASES))
    frames = [frame(i) for i in range(n_frames)]
    out["frame_sha256"] = np.array([sha(f) for f in frames])
    for mode in ("train", "eval"):
        augs = draws(ImageAffineTransformation, mode == "train", N_DRAWS)
        (out[mode + "_resize"], out[mode + "_dims"], out[mode + "_crop"], out[mode + "_flip"],
         out[mode + "_rotate"]) = pack_augs(augs)
        imgs, mats = zip(*[img_transform(Image.fromarray(frames[i]), *augs[i]) for i in range(N_DRAWS)])
        out[mode + "_ida_mat"] = np.stack(mats)
        out[mode + "_out_sha256"] = np.array([sha(np.asarray(im)) for im in imgs])
    eval_aug = draws(ImageAffineTransformation, False, 1)[0]
    case_list = [(i, eval_aug if a is None else a) for i, a in CASES]
    out["case_frame"] = np.array([i for i, _ in case_list])
    (out["case_resize"], out["case_dims"], out["case_crop"], out["case_flip"],
     out["case_rotate"]) = pack_augs([a for _, a in case_list])
    mats = []
    for k, (i, a) in enumerate(case_list):
        im, m = img_transform(Image.fromarray(frames[i]), *a)
        out[f"case{k}_out"] = np.asarray(im)
        mats.append(m)
    out["case_ida_mat"] = np.stack(mats)
    path = os.path.join(HERE, "golden", "image_affine.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    ROOT = os.path.dirname(HERE)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
    os.environ.setdefault("UD_RANDOM_INIT", "1")
    write_golden(os.environ["UNIDISTILL_REF"])
