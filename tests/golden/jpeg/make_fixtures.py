"""Writes the JPEG fixtures of tests/test_jpeg_cpu.py / tests/test_jpeg_decode_gpu.py with Pillow (libjpeg-turbo) and
records the sha256 of Pillow's decoded RGB array for each (manifest.json); full arrays only for the small images
(small.npz).  Content: the frame(i) generator of tests/test_image_affine_cpu.py and a smooth gradient.
Run from the repository root: python tests/golden/jpeg/make_fixtures.py"""
import hashlib
import io
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from test_image_affine_cpu import frame  # noqa: E402


def smooth(H, W, i=0):
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    return np.stack([(x * 255) // max(W, 1), (y * 255) // max(H, 1), ((x + y + 37 * i) * 255) // (W + H + 37 * i)],
                    -1).astype(np.uint8)


# 16-bit DQT: entries above 255 (Pillow writes a 16-bit table and an SOF1 frame)
QT16 = [[min(999, 3 + 20 * i) for i in range(64)], [300 + i for i in range(64)]]

# name: (content, H, W, save options)
SUPPORTED = {
    "f0_q75_420": ("frame0", 900, 1600, dict(quality=75, subsampling=2)),
    "f1_q50_420_rst_rows": ("frame1", 900, 1600, dict(quality=50, subsampling=2, restart_marker_rows=1)),
    "s0_q90_422_rst_blocks": ("smooth0", 900, 1600, dict(quality=90, subsampling=1, restart_marker_blocks=7)),
    "s1_q95_444_opt": ("smooth1", 900, 1600, dict(quality=95, subsampling=0, optimize=True)),
    "s2_q100_420_opt_rst": ("smooth2", 900, 1600, dict(quality=100, subsampling=2, optimize=True,
                                                       restart_marker_blocks=64)),
    "s3_q75_420_odd": ("smooth3", 899, 1601, dict(quality=75, subsampling=2)),
    "f2_q95_444_crop": ("frame2", 180, 320, dict(quality=95, subsampling=0)),
    "f3_q90_422_opt_rst": ("frame3", 72, 120, dict(quality=90, subsampling=1, optimize=True, restart_marker_rows=2)),
    "f4_qt16_420": ("frame4", 64, 96, dict(qtables=QT16, subsampling=2)),
    "f5_q50_420_17x9": ("frame5", 9, 17, dict(quality=50, subsampling=2)),
    "f6_q100_422_17x9": ("frame6", 9, 17, dict(quality=100, subsampling=1)),
    "f7_q75_444_17x9_rst": ("frame7", 9, 17, dict(quality=75, subsampling=0, restart_marker_blocks=1)),
    "f8_q90_420_8x8": ("frame8", 8, 8, dict(quality=90, subsampling=2)),
    "f9_q95_422_8x8_opt": ("frame9", 8, 8, dict(quality=95, subsampling=1, optimize=True)),
    "f10_q75_420_1x1": ("frame10", 1, 1, dict(quality=75, subsampling=2)),
    "f11_q100_444_1x1": ("frame11", 1, 1, dict(quality=100, subsampling=0)),
    "f12_q75_420_3x5": ("frame12", 5, 3, dict(quality=75, subsampling=2)),
    "f13_q90_422_33x47_rst": ("frame13", 33, 47, dict(quality=90, subsampling=1, restart_marker_blocks=2)),
}
REJECTED = {
    "reject_progressive": ("frame14", 32, 48, dict(quality=75, progressive=True), "unsupported"),
    "reject_gray": ("frame15", 32, 48, dict(quality=75, mode="L"), "unsupported"),
}
SMALL = 100 * 100                 # store full arrays up to this many pixels


def content(name, H, W):
    if name.startswith("frame"):
        return frame(int(name[5:]), H, W)
    return smooth(H, W, int(name[6:]))


def encode(a, opts):
    opts = dict(opts)
    mode = opts.pop("mode", "RGB")
    im = Image.fromarray(a)
    if mode != "RGB":
        im = im.convert(mode)
    b = io.BytesIO()
    im.save(b, "JPEG", **opts)
    return b.getvalue()


def main():
    manifest, small = {}, {}
    for name, (c, H, W, opts) in list(SUPPORTED.items()) + [(k, v[:4]) for k, v in REJECTED.items()]:
        data = encode(content(c, H, W), opts)
        with open(os.path.join(HERE, name + ".jpg"), "wb") as fh:
            fh.write(data)
        dec = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        manifest[name] = {"shape": list(dec.shape), "sha256": hashlib.sha256(dec.tobytes()).hexdigest(),
                          "supported": name in SUPPORTED, "options": {k: v for k, v in opts.items() if k != "qtables"}}
        if dec.shape[0] * dec.shape[1] <= SMALL:
            small[name] = dec
    with open(os.path.join(HERE, "manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "small.npz"), **small)


if __name__ == "__main__":
    main()
