"""GPU timing of the camera augmentation (ud_image_affine) at production sizes: B = 4 x 6 cameras of
1600 x 900 uint8 frames -> 704 x 256, training-mode draws.  Prints the kernel time per batch (device events, after
warm-up) for the uint8 and the fused normalised float32 outputs, the algorithmic bytes and their share of the measured
6.3 TB/s copy rate, the pinned H2D copy of the crops' source row bands, and Pillow's time per frame on this host.
    python tools/time_image_affine.py            [B=4 NCAM=6 ITERS=50 PIL_FRAMES=12]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
import numpy as np
import torch

from unidistill_amd.ops import image_affine, input_prep as ip

COPY_TBS = 6.3                                   # measured device copy rate (DESIGN)
B, NCAM = int(os.environ.get("B", 4)), int(os.environ.get("NCAM", 6))
ITERS, PIL_FRAMES = int(os.environ.get("ITERS", 50)), int(os.environ.get("PIL_FRAMES", 12))
CONF = dict(resize_lim=(0.386, 0.55), final_dim=(256, 704), rot_lim=(-5.4, 5.4), H=900, W=1600, rand_flip=True,
            bot_pct_lim=(0.0, 0.0))
d = torch.device("cuda:0")
np.random.seed(0)
t = ip.ImageAffineTransformation(True, **CONF)
N = B * NCAM
augs = [t.sample_augs() for _ in range(N)]
host = np.random.default_rng(0).integers(0, 256, (N, 900, 1600, 3), dtype=np.uint8)
x = torch.from_numpy(host).to(d)


def timeit(fn, n=ITERS):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


recs, bands, _ = ip.plan_frames(augs, 900, 1600, (256, 704), d)
i = image_affine._FRAME_FIELDS.index
band_rows = sum(r for _, r in bands)
src_bytes = sum(int(r[i("band_rows")]) * 1600 * 3 for r in recs)              # source rows the kernel reads
mid_bytes = sum(int(r[i("band_rows")]) * int(r[i("ncols")]) * 3 for r in recs)  # uint8 intermediate, written + read
for name, kw, out_bytes in (("u8", dict(normalize=False), N * 256 * 704 * 3),
                            ("f32 NCHW", dict(normalize=True), N * 256 * 704 * 12),
                            ("f32 NHWC", dict(normalize=True, channels_last=True), N * 256 * 704 * 12)):
    us = timeit(lambda: ip.image_affine(x, augs, **kw))
    alg = src_bytes + 2 * mid_bytes + out_bytes
    print(f"image_affine {name:8s}: {us:7.1f} us / batch of {N}  bytes {alg / 1e6:.1f} MB (src {src_bytes / 1e6:.1f} "
          f"+ 2 x intermediate {mid_bytes / 1e6:.1f} + out {out_bytes / 1e6:.1f})  {alg / us / 1e6:.2f} TB/s "
          f"= {alg / us / 1e6 / COPY_TBS * 100:.0f}% of {COPY_TBS} TB/s")

# H2D of the raw row bands (pinned), as collate_fn ships them
pinned = torch.empty(band_rows * 1600 * 3, dtype=torch.uint8, pin_memory=True)
us = timeit(lambda: pinned.to(d, non_blocking=True), n=20)
print(f"H2D row bands: {band_rows} of {N * 900} rows, {pinned.numel() / 1e6:.1f} MB pinned -> {us / 1e3:.2f} ms "
      f"({pinned.numel() / us / 1e3:.1f} GB/s); whole frames would be {host.nbytes / 1e6:.1f} MB")
t0 = time.perf_counter()
for _ in range(3):
    ip.image_affine_host_frames(host, augs, d)
torch.cuda.synchronize()
print(f"collate path (band pack + pinned H2D + kernel, host wall): {(time.perf_counter() - t0) / 3 * 1e3:.2f} ms / batch")

try:
    from PIL import Image
except ImportError:
    print("PIL not importable: no host comparison")
else:
    t0 = time.perf_counter()
    for k in range(PIL_FRAMES):
        a = augs[k % N]
        img = Image.fromarray(host[k % N]).resize(a[1]).crop(a[2])
        if a[3]:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        img.rotate(a[4])
    ms = (time.perf_counter() - t0) / PIL_FRAMES * 1e3
    print(f"PIL on this host: {ms:.2f} ms / frame (one core) -> {ms * N:.0f} ms of CPU per batch of {N}")
