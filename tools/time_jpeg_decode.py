"""Times the JPEG decode after collate on 24 frames of 1600x900 (the committed 1600x900 fixtures of
tests/golden/jpeg/, mixed qualities, sampling modes and restart intervals), as one B = 4 x 6-camera batch:
  - jpeg_decode wall time and the synchronisation rounds the Huffman decode needed per frame;
  - Pillow's single-core decode time per file (when Pillow is importable);
  - collate_fn on the imgs_jpeg route against the imgs_raw route with Pillow's decode counted, and the H2D bytes of both.
Per-kernel device times: run under `rocprofv3 --kernel-trace --stats -- python tools/time_jpeg_decode.py --trace`.
Prints one JSON line."""
import argparse
import ctypes
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cvpr2023-unidistill_amd"))
JDIR = os.path.join(ROOT, "tests", "golden", "jpeg")
CONF = dict(resize_lim=(0.386, 0.55), final_dim=(256, 704), rot_lim=(-5.4, 5.4), H=900, W=1600, rand_flip=True,
            bot_pct_lim=(0.0, 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--trace", action="store_true", help="only a few decodes (for a rocprofv3 kernel trace)")
    a = ap.parse_args()
    from unidistill_amd.ops import input_prep as ip
    from unidistill_amd.ops import jpeg
    man = json.load(open(os.path.join(JDIR, "manifest.json")))
    big = sorted(k for k, v in man.items() if v["supported"] and v["shape"][:2] == [900, 1600])
    names = [big[(7 * i + i // len(big)) % len(big)] for i in range(24)]
    files = [open(os.path.join(JDIR, n + ".jpg"), "rb").read() for n in names]
    dev = torch.device("cuda:0")
    out, st = jpeg.jpeg_decode(files, dev)
    torch.cuda.synchronize()
    assert not st.cpu().any()
    res = {"frames": 24, "jpeg_bytes": sum(len(f) for f in files),
           "sync_rounds": jpeg.STATS["last_sync_iters"].cpu().tolist()}
    iters = 3 if a.trace else a.iters
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        jpeg.jpeg_decode(files, dev, out=out)
    torch.cuda.synchronize()
    res["jpeg_decode_ms"] = (time.perf_counter() - t0) / iters * 1e3
    if a.trace:
        print(json.dumps(res))
        return
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        per = {}
        for n, f in zip(names, files):
            if n in per:
                continue
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
                ts.append(time.perf_counter() - t0)
            per[n] = min(ts) * 1e3
        res["pillow_ms_per_file"] = per
        res["pillow_ms_batch_one_core"] = sum(per[n] for n in names)
    raw = out.cpu().numpy().reshape(4, 1, 6, 900, 1600, 3)
    t = ip.ImageAffineTransformation(is_train=True, **CONF)
    np.random.seed(0)
    augs = [[[t.sample_augs() for _ in range(6)]] for _ in range(4)]
    batch_j = [{"imgs_jpeg": [files[6 * b:6 * b + 6]], "ida_aug": augs[b]} for b in range(4)]
    batch_r = [{"imgs_raw": raw[b], "ida_aug": augs[b]} for b in range(4)]
    for name, batch in (("collate_jpeg_ms", batch_j), ("collate_raw_ms", batch_r)):
        ip.collate_fn(batch, device=dev, with_points=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            ip.collate_fn(batch, device=dev, with_points=False)
        torch.cuda.synchronize()
        res[name] = (time.perf_counter() - t0) / a.iters * 1e3
    if "pillow_ms_batch_one_core" in res:
        res["collate_raw_plus_pillow_ms"] = res["collate_raw_ms"] + res["pillow_ms_batch_one_core"]
    recs, bands, _ = ip.plan_frames([x for s in augs for c in s for x in c], 900, 1600, (256, 704), dev)
    res["h2d_bytes_raw_route"] = int(sum(r for _, r in bands) * 1600 * 3)
    res["h2d_bytes_jpeg_route"] = int(sum((len(f) + 15) // 16 * 16 for f in files)
                                      + 24 * ctypes.sizeof(jpeg.UdJpegFrame))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
