"""CPU: the JPEG reference decoder (tests/jpeg_reference.py) against Pillow and the committed digests, its emulation of
the device's self-synchronising Huffman decode, ud_jpeg_parse through ctypes, and the host-side argument checks of
jpeg_decode / collate_fn / ImageAffineTransformation."""
import hashlib
import io
import json
import os

import numpy as np
import pytest

import jpeg_reference as jr
from conftest import GOLDEN

JDIR = os.path.join(GOLDEN, "jpeg")
MANIFEST = json.load(open(os.path.join(JDIR, "manifest.json")))
SUPPORTED = sorted(k for k, v in MANIFEST.items() if v["supported"])
SMALL = sorted(k for k in SUPPORTED if MANIFEST[k]["shape"][0] * MANIFEST[k]["shape"][1] <= 320 * 180)


def load(name):
    with open(os.path.join(JDIR, name + ".jpg"), "rb") as fh:
        return fh.read()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("name", SMALL)
def test_reference_equals_pillow_small(name):
    got = jr.decode(load(name))
    assert sha(got) == MANIFEST[name]["sha256"]
    small = np.load(os.path.join(JDIR, "small.npz"))
    if name in small.files:
        np.testing.assert_array_equal(got, small[name])


def test_reference_equals_pillow_full_size():
    """One 1600x900 frame (4:2:2, restart every 7 MCUs) and the 1601x899 odd-size one."""
    for name in ("s0_q90_422_rst_blocks", "s3_q75_420_odd"):
        assert sha(jr.decode(load(name))) == MANIFEST[name]["sha256"], name


def test_reference_equals_pillow_live_encodes():
    """Fresh encodes of every sampling mode, several qualities, optimised tables and restart settings, at sizes that
    are not MCU multiples (Pillow needed)."""
    Image = pytest.importorskip("PIL.Image")
    from test_image_affine_cpu import frame
    for H, W in ((9, 17), (2, 3), (5, 4), (33, 47)):
        a = frame(H + W, H, W)
        for q in (50, 95, 100):
            for ss in (0, 1, 2):
                for kw in ({}, {"optimize": True}, {"restart_marker_blocks": 1}):
                    b = io.BytesIO()
                    Image.fromarray(a).save(b, "JPEG", quality=q, subsampling=ss, **kw)
                    d = b.getvalue()
                    np.testing.assert_array_equal(jr.decode(d), np.asarray(Image.open(io.BytesIO(d)).convert("RGB")),
                                                  err_msg=f"{H}x{W} q{q} ss{ss} {kw}")


def test_sixteen_bit_quant_tables():
    data = load("f4_qt16_420")
    i = data.index(b"\xff\xdb")
    assert data[i + 4] >> 4 == 1                  # Pq = 1: 16-bit DQT
    assert b"\xff\xc1" in data[:i + 600]          # extended sequential frame
    assert jr.parse(data).qt.max() > 255


@pytest.mark.parametrize("sub_bits", [1, 7, 8, 13, 64, 1024])
@pytest.mark.parametrize("name", ["f3_q90_422_opt_rst", "f4_qt16_420", "f13_q90_422_33x47_rst", "f5_q50_420_17x9"])
def test_sync_decode_equals_serial(name, sub_bits):
    """The self-synchronising decode gives the serial decode's coefficients, for subsequence sizes down to 1 bit
    (every code and block boundary then falls on a subsequence boundary) and sizes that cut codes."""
    data = load(name)
    f = jr.parse(data)
    ref = jr.decode_coefficients(data, f)
    got, rounds = jr.sync_decode_coefficients(data, f, sub_bits)
    np.testing.assert_array_equal(got, ref)
    assert rounds >= 1


def test_sync_decode_boundaries_on_codes():
    """Subsequence sizes taken from the serial decode's own symbol and block boundaries, so a boundary falls exactly on
    the start of a code and exactly on the start of a block."""
    data = load("f2_q95_444_crop")
    f = jr.parse(data)
    seg = jr.destuff(data, f)[0]
    bits = jr.Bits(seg)
    st, starts, blocks = (0, 0, 0), [], []
    while len(blocks) < 40:
        st, ev = jr.step(bits, f, st)
        starts.append(st[0])
        if ev == "block":
            blocks.append(st[0])
    ref = jr.decode_coefficients(data, f)
    for s in (starts[5], starts[17], blocks[3], blocks[11]):
        assert s > 0
        got, _ = jr.sync_decode_coefficients(data, f, s)
        np.testing.assert_array_equal(got, ref, err_msg=f"sub_bits {s}")


# ---- ud_jpeg_parse -------------------------------------------------------------------------------------------
def _same_record(rec, f):
    geo = ("width", "height", "hmax", "vmax", "mcus_x", "mcus_y", "bpm", "restart", "nseg", "ecs_off", "ecs_bytes")
    for k in geo:
        assert getattr(rec, k) == getattr(f, k), k
    for k in ("h", "v", "cw", "ch", "comp_id"):
        assert list(getattr(rec, k)) == list(getattr(f, k)), k
    np.testing.assert_array_equal(np.ctypeslib.as_array(rec.qt), f.qt)
    for t in range(6):
        for k, v in zip(("look", "maxcode", "valoff", "vals"), f.huff[t]):
            np.testing.assert_array_equal(np.ctypeslib.as_array(getattr(rec.huff[t], k)), v, err_msg=f"{t} {k}")


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_parse_matches_reference(hip_lib, name):
    from unidistill_amd.ops import jpeg
    data = load(name)
    rc, rec = jpeg.parse(data)
    try:
        f, code = jr.parse(data), jr.OK
    except jr.JpegError as e:
        f, code = None, e.code
    assert rc == code
    assert (rc == jpeg.OK) == MANIFEST[name]["supported"]
    if f is not None:
        _same_record(rec, f)
        assert rec.total_blocks == rec.mcus_x * rec.mcus_y * rec.bpm


def _segment(data, marker):
    i = data.index(marker)
    return i, i + 2 + (data[i + 2] << 8 | data[i + 3])


def test_parse_return_codes(hip_lib):
    from unidistill_amd.ops import jpeg
    d = load("f8_q90_420_8x8")
    assert jpeg.parse(load("reject_progressive"))[0] == jpeg.UNSUPPORTED
    assert jpeg.parse(load("reject_gray"))[0] == jpeg.UNSUPPORTED
    s0, s1 = _segment(d, b"\xff\xc0")
    assert jpeg.parse(d[:s0 + 5])[0] == jpeg.TRUNCATED                  # ends inside SOF
    assert jpeg.parse(d[:s1])[0] == jpeg.TRUNCATED                      # ends before the scan
    assert jpeg.parse(d[:s0] + b"\xff\xd9")[0] == jpeg.TRUNCATED         # EOI before a scan
    assert jpeg.parse(b"\x00" + d[1:])[0] == jpeg.CORRUPT               # no SOI
    twelve = bytearray(d)
    twelve[s0 + 4] = 12
    assert jpeg.parse(bytes(twelve))[0] == jpeg.UNSUPPORTED             # 12-bit
    for marker in (b"\xc2", b"\xc3", b"\xc9"):                          # progressive, lossless, arithmetic
        m = bytearray(d)
        m[s0 + 1] = marker[0]
        assert jpeg.parse(bytes(m))[0] == jpeg.UNSUPPORTED, marker
    s440 = bytearray(d)                                                 # luma 1x2: 4:4:0
    s440[s0 + 11] = 0x12
    assert jpeg.parse(bytes(s440))[0] == jpeg.UNSUPPORTED
    rgb = bytearray(d.replace(b"JFIF\x00", b"JFXX\x00"))                # no JFIF, component ids R G B
    for c, v in enumerate(b"RGB"):
        rgb[s0 + 10 + 3 * c] = v
    sos = rgb.index(b"\xff\xda")
    for c, v in enumerate(b"RGB"):
        rgb[sos + 5 + 2 * c] = v
    assert jpeg.parse(bytes(rgb))[0] == jpeg.UNSUPPORTED
    adobe = d[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + d[2:]
    assert jpeg.parse(adobe)[0] == jpeg.UNSUPPORTED                     # Adobe transform 0: RGB
    noq = bytearray(d)
    noq[s0 + 12] = 3                                                    # quant table 3 never defined
    assert jpeg.parse(bytes(noq))[0] == jpeg.CORRUPT
    rc, rec = jpeg.parse(d[:-40])                                       # the scan cut short: the device reports it
    assert rc == jpeg.OK and rec.ecs_off + rec.ecs_bytes == len(d) - 40


def test_plan_and_launch_checks(hip_lib):
    import ctypes
    from unidistill_amd.ops import jpeg
    recs = (jpeg.UdJpegFrame * 2)(jpeg.parse(load("f0_q75_420"))[1], jpeg.parse(load("s3_q75_420_odd"))[1])
    n = hip_lib.ud_jpeg_plan(recs, 2)
    assert n > 2 * 1600 * 900 * 3
    assert recs[1].out_off == 1600 * 900 * 3 and recs[0].ws_coef == 0 and recs[1].ws_coef > 0
    assert all(getattr(recs[i], k) % 16 == 0 for i in range(2) for k in ("ws_ecs", "ws_seg", "ws_sub", "ws_state"))
    bad = (jpeg.UdJpegFrame * 1)(recs[0])
    bad[0].mcus_x += 1                                                  # geometry inconsistent with the size
    assert hip_lib.ud_jpeg_plan(bad, 1) == 0
    # the launcher checks before anything is launched (no device pointer is touched on these paths)
    src = ctypes.c_void_p(16)
    args = lambda N, src_bytes, out_bytes, ws: (src, src_bytes, recs, src, N, src, out_bytes, src, None, src, ws, None)
    assert hip_lib.ud_jpeg_decode(*args(0, 0, 0, 0)) == 0
    big = 1 << 40
    assert hip_lib.ud_jpeg_decode(*args(2, 10, big, n)) == -1           # the files are not inside src
    assert hip_lib.ud_jpeg_decode(*args(2, big, 100, n)) == -1          # out too small
    assert hip_lib.ud_jpeg_decode(*args(2, big, big, n - 16)) == -2     # workspace too small


# ---- host-side checks of the Python entry points -----------------------------------------------------------------
def test_jpeg_decode_argument_checks(hip_lib):
    from unidistill_amd.ops import jpeg
    with pytest.raises(RuntimeError, match="GPU only"):
        jpeg.jpeg_decode([load("f8_q90_420_8x8")], "cpu")
    with pytest.raises(ValueError, match="bytes"):
        jpeg.jpeg_decode([np.zeros((2, 2), np.uint8)], "cuda:0")
    with pytest.raises(ValueError, match="no JPEG"):
        jpeg.jpeg_decode([], "cuda:0")


def test_collate_jpeg_argument_checks():
    from unidistill_amd.ops import input_prep as ip
    f = load("f8_q90_420_8x8")
    aug = (0.5, (4, 4), (0, 0, 4, 4), False, 0.0)
    with pytest.raises(ValueError, match="ida_aug"):
        ip.collate_fn([{"imgs_jpeg": [[f, f]]}], device="cuda:0")
    with pytest.raises(ValueError, match="nesting"):
        ip.collate_fn([{"imgs_jpeg": [[f, f]], "ida_aug": [[aug, aug]]}, {"imgs_jpeg": [[f]]}], device="cuda:0")
    with pytest.raises(ValueError, match="augs for"):
        ip.collate_fn([{"imgs_jpeg": [[f, f]], "ida_aug": [[aug]]}], device="cuda:0")


def test_loader_side_draws_for_jpeg_bytes():
    """ImageAffineTransformation.forward draws per camera whether the values are frames or JPEG bytes (also under
    imgs_jpeg), in the same np.random order."""
    from unidistill_amd.ops import input_prep as ip
    conf = dict(resize_lim=(0.386, 0.55), final_dim=(256, 704), rot_lim=(-5.4, 5.4), H=900, W=1600, rand_flip=True,
                bot_pct_lim=(0.0, 0.0))
    cams = ["CAM_FRONT", "CAM_FRONT_LEFT", "CAM_BACK"]
    t = ip.ImageAffineTransformation(is_train=True, **conf)
    outs = []
    for d in ({"imgs": {c: np.zeros((900, 1600, 3), np.uint8) for c in cams}},
              {"imgs": {c: b"\xff\xd8" for c in cams}}, {"imgs_jpeg": {c: b"\xff\xd8" for c in cams}}):
        np.random.seed(42)
        outs.append(t(d))
    for o in outs[1:]:
        assert list(o["ida_aug"]) == cams
        for c in cams:
            assert o["ida_aug"][c] == outs[0]["ida_aug"][c]
            np.testing.assert_array_equal(o["ida_mat"][c], outs[0]["ida_mat"][c])


# ---- malformed Huffman tables, bytes after EOI, header errors -------------------------------------------------------
def _with_dht(d, counts, th=3):
    """d with one more DHT segment (AC table `th`) right after SOI: the given 16 counts, symbols 1, 2, ..."""
    counts = list(counts) + [0] * (16 - len(counts))
    vals = bytes((k % 255) + 1 for k in range(sum(counts)))
    body = bytes([0x10 | th]) + bytes(counts) + vals
    return d[:2] + b"\xff\xc4" + (2 + len(body)).to_bytes(2, "big") + body + d[2:]


@pytest.mark.parametrize("counts", [[40], [2, 1], [0, 4], [1, 1, 2], [0, 0, 9]])
def test_oversubscribed_huffman_table_is_corrupt(hip_lib, counts):
    """Tables whose codes do not fit their lengths (or use the all-ones code, which libjpeg refuses) are rejected
    before any lookup entry is written."""
    from unidistill_amd.ops import jpeg
    d = _with_dht(load("f8_q90_420_8x8"), counts)
    assert jpeg.parse(d)[0] == jpeg.CORRUPT
    with pytest.raises(jr.JpegError) as e:
        jr.parse(d)
    assert e.value.code == jr.CORRUPT


def test_full_huffman_table_without_all_ones_code_is_accepted(hip_lib):
    from unidistill_amd.ops import jpeg
    d = _with_dht(load("f8_q90_420_8x8"), [0, 3, 1, 1])          # 00 01 10 | 110 | 1110: 1111 stays free
    assert jpeg.parse(d)[0] == jpeg.OK
    assert sha(jr.decode(d)) == MANIFEST["f8_q90_420_8x8"]["sha256"]


@pytest.mark.parametrize("name", ["f13_q90_422_33x47_rst", "f5_q50_420_17x9"])
def test_bytes_after_eoi_are_ignored(hip_lib, name):
    """The scan ends at its first marker other than RSTn: padding and data after EOI do not change the decode."""
    from unidistill_amd.ops import jpeg
    d = load(name) + b"\x00" * 37 + b"\xff\xd9trailer\xff"
    rc, rec = jpeg.parse(d)
    assert rc == jpeg.OK and rec.ecs_off + rec.ecs_bytes == len(d)
    assert sha(jr.decode(d)) == MANIFEST[name]["sha256"]


def test_header_errors_raise_with_frame_index(hip_lib):
    """Truncated or corrupt headers are not handed to Pillow: ValueError with the frame's index, and collate_fn names
    sample, sweep and camera (raised on the host, before any device work)."""
    from unidistill_amd.ops import input_prep as ip
    from unidistill_amd.ops import jpeg
    f = load("f8_q90_420_8x8")
    s0, _ = _segment(f, b"\xff\xc0")
    short = f[:s0 + 5]
    with pytest.raises(jpeg.JpegFrameError, match="truncated") as e:
        jpeg.jpeg_decode([f, short], "cuda:0")
    assert e.value.index == 1 and isinstance(e.value, ValueError)
    with pytest.raises(jpeg.JpegFrameError, match="corrupt"):
        jpeg.jpeg_decode([_with_dht(f, [2, 1])], "cuda:0")
    aug = (0.5, (4, 4), (0, 0, 4, 4), False, 0.0)
    with pytest.raises(ValueError, match="sample 1 sweep 0 camera 0: truncated"):
        ip.collate_fn([{"imgs_jpeg": [[f]], "ida_aug": [[aug]]}, {"imgs_jpeg": [[short]], "ida_aug": [[aug]]}],
                      device="cuda:0")


def test_unsupported_file_pillow_cannot_decode_raises_with_index(hip_lib):
    pytest.importorskip("PIL.Image")
    from unidistill_amd.ops import jpeg
    prog = load("reject_progressive")
    with pytest.raises(jpeg.JpegFrameError, match="Pillow failed") as e:
        jpeg.jpeg_decode([load("f8_q90_420_8x8"), load("f8_q90_420_8x8"), prog[:len(prog) // 2]], "cuda:0")
    assert e.value.index == 2
