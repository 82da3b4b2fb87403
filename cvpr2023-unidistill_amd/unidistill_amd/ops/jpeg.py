"""JPEG decode after collate: camera frames travel as their JPEG bytes and are decoded on the device.

The reference reads every camera frame with skimage_io.imread (nuscenes_multimodal.py:171-177, :197), i.e. Pillow's
libjpeg-turbo, in the loader.  ``jpeg_decode`` parses each file on the host (ud_jpeg_parse: markers and tables only),
packs the compressed bytes and the per-frame records into one pinned buffer, makes one H2D copy and decodes the batch
in four launches on the input stream (csrc/jpeg_decode.hip), bit for bit as Pillow decodes it.  Files the parser does
not support (progressive, grayscale, CMYK, ...) are decoded by Pillow on the host when it is importable and counted in
``STATS``; without Pillow they raise.  Files with truncated or inconsistent headers raise JpegFrameError (a ValueError
carrying the frame's index), as does a fallback file Pillow cannot decode.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .staging import align16, device_index, staged_upload

OK, UNSUPPORTED, TRUNCATED, CORRUPT = 0, 1, 2, 3           # UD_JPEG_* (include/unidistill_hip.h)
ST_MARKER, ST_CODE, ST_LENGTH = 1, 2, 4                    # UD_JPEG_ST_* status bits
SUB_BITS = 1024                                            # UD_JPEG_SUB_BITS
PARSE_ERRORS = {UNSUPPORTED: "unsupported", TRUNCATED: "truncated", CORRUPT: "corrupt"}

# frames: decoded on the device; fallback: decoded by Pillow because the parser reported them unsupported;
# last_sync_iters: int32 [N] device tensor of the last call's synchronisation rounds (-1 for fallback frames)
STATS = {"frames": 0, "fallback": 0, "last_sync_iters": None}


class UdJpegHuff(ctypes.Structure):
    _fields_ = [("look", ctypes.c_uint16 * 512), ("maxcode", ctypes.c_int32 * 18), ("valoff", ctypes.c_int32 * 18),
                ("vals", ctypes.c_uint8 * 256)]


class UdJpegFrame(ctypes.Structure):
    """Mirror of include/unidistill_hip.h UdJpegFrame."""
    _fields_ = ([(k, ctypes.c_int32) for k in ("width", "height", "hmax", "vmax", "mcus_x", "mcus_y", "bpm", "restart",
                                                "nseg", "reserved0")]
                + [(k, ctypes.c_int32 * 3) for k in ("comp_id", "h", "v", "cw", "ch")] + [("reserved1", ctypes.c_int32)]
                + [(k, ctypes.c_int64) for k in ("ecs_off", "ecs_bytes", "src_off", "out_off", "ws_ecs", "ws_seg",
                                                 "ws_sub", "ws_state", "ws_scan", "ws_coef")]
                + [("ws_plane", ctypes.c_int64 * 3), ("nsub_max", ctypes.c_int64), ("total_blocks", ctypes.c_int64),
                   ("qt", (ctypes.c_uint16 * 64) * 3), ("huff", UdJpegHuff * 6)])


def _as_bytes(buf):
    if isinstance(buf, (bytes, bytearray, memoryview)):
        return bytes(buf)
    if isinstance(buf, np.ndarray) and buf.dtype == np.uint8 and buf.ndim == 1:
        return buf.tobytes()
    raise ValueError(f"a JPEG frame must be bytes or a 1-D uint8 numpy array, got {type(buf).__name__}")


def parse(buf):
    """ud_jpeg_parse on one file -> (code, UdJpegFrame); code is OK or one of UNSUPPORTED / TRUNCATED / CORRUPT."""
    data = _as_bytes(buf)
    rec = UdJpegFrame()
    rc = _lib.load().ud_jpeg_parse(data, len(data), ctypes.byref(rec))
    if rc < 0:
        _lib.check(rc, "ud_jpeg_parse")  # raw handle: the positive codes go back to the caller, only a negative one is an error
    return rc, rec


class JpegFrameError(ValueError):
    """A file of the batch cannot be decoded; ``index`` is its position in the buffers."""

    def __init__(self, index, msg):
        super().__init__(f"JPEG frame {index}: {msg}")
        self.index = index
        self.reason = msg


def _pillow_decode(index, data):
    """Host decode of a file the device parser does not support (UNSUPPORTED only)."""
    try:
        from PIL import Image
    except ImportError:
        raise JpegFrameError(index, "unsupported by the device decoder and Pillow is not importable") from None
    import io
    try:
        with Image.open(io.BytesIO(data)) as im:
            return np.asarray(im.convert("RGB"))
    except Exception as e:          # Pillow raises OSError / SyntaxError / ... on broken files
        raise JpegFrameError(index, f"unsupported by the device decoder and Pillow failed: {e}") from e


def jpeg_decode(buffers, device, out=None):
    """Decode host JPEG files (``bytes`` or 1-D uint8 arrays) on ``device`` -> (frames uint8 [N, H, W, 3], status
    int32 [N]), both on the device.  The frames must share H x W (ValueError otherwise).  A status word is 0 or the
    UD_JPEG_ST_* bits of a frame whose entropy-coded data failed (its pixels are zeros); the caller decides what to do
    with it.  Runs on input_stream(device); the caller's current stream waits on the result.  ``out``: an optional
    uint8 [N, H, W, 3] device tensor to decode into; the decode is ordered after the work already queued on the
    caller's current stream.  A file that cannot be decoded at all raises JpegFrameError (ValueError) with its index."""
    device = _lib.require_gpu_device(device)
    datas = [_as_bytes(b) for b in buffers]
    if not datas:
        raise ValueError("no JPEG frames")
    recs, host_frames = [], {}
    for i, d in enumerate(datas):
        rc, rec = parse(d)
        if rc == OK:
            recs.append((i, rec))
        elif rc == UNSUPPORTED:
            host_frames[i] = _pillow_decode(i, d)
        else:
            raise JpegFrameError(i, f"{PARSE_ERRORS[rc]} headers")
    sizes = {(r.height, r.width) for _, r in recs} | {a.shape[:2] for a in host_frames.values()}
    if len(sizes) != 1:
        raise ValueError(f"JPEG frames of one batch must share H x W, got {sorted(sizes)}")
    H, W = sizes.pop()
    N, fb = len(datas), H * W * 3
    if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != (N, H, W, 3) or not out.is_contiguous()
                            or out.device != torch.device("cuda", device_index(device))):
        raise ValueError(f"out must be a contiguous uint8 [{N}, {H}, {W}, 3] tensor on {device}")

    # host staging: files, then Pillow's frames for the fallback, then the records
    lib = _lib.load()
    off, file_off = 0, []
    for i, rec in recs:
        file_off.append(off)
        rec.src_off = off
        off = align16(off + len(datas[i]))
    src_bytes = off
    host_off = {}
    for i in host_frames:
        host_off[i] = off
        off = align16(off + fb)
    rec_arr = (UdJpegFrame * max(len(recs), 1))(*[r for _, r in recs])
    ws_bytes = int(lib.ud_jpeg_plan(rec_arr, len(recs))) if recs else 0
    if recs and ws_bytes == 0:
        raise RuntimeError("ud_jpeg_plan rejected a parsed record")
    for j, (i, _) in enumerate(recs):
        rec_arr[j].out_off = i * fb                        # the frame's slot in out
    rec_off = off
    rec_bytes = ctypes.sizeof(rec_arr) if recs else 0
    cur = None if out is None else torch.cuda.current_stream(device)

    def fill(hv, dev):
        for (i, _), o in zip(recs, file_off):
            hv[o:o + len(datas[i])] = np.frombuffer(datas[i], np.uint8)
        for i, a in host_frames.items():
            hv[host_off[i]:host_off[i] + fb] = np.ascontiguousarray(a, np.uint8).reshape(-1)
        if rec_bytes:
            ctypes.memmove(hv.ctypes.data + rec_off, rec_arr, rec_bytes)

    def run(dev, s, out=out):
        device = dev.device
        if out is None:
            out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=device)
        else:
            s.wait_stream(cur)      # earlier work of the caller's stream on out (reads or writes) comes first
            out.record_stream(s)
        status = torch.zeros(N, dtype=torch.int32, device=device)
        iters = torch.full((N,), -1, dtype=torch.int32, device=device)
        flat = out.view(N, fb)
        for i in host_frames:
            flat[i].copy_(dev[host_off[i]:host_off[i] + fb])
        if recs:
            ws = _lib.workspace(device, ws_bytes, slot="jpeg")
            ws.record_stream(s)
            st_d = torch.empty(2 * len(recs), dtype=torch.int32, device=device)
            _lib.ud.ud_jpeg_decode(dev.data_ptr(), src_bytes, rec_arr, dev.data_ptr() + rec_off, len(recs), out.data_ptr(),
                                   out.numel(), st_d.data_ptr(), st_d.data_ptr() + 4 * len(recs), ws.data_ptr(), ws.numel(),
                                   s.cuda_stream)
            idx = torch.tensor([i for i, _ in recs], dtype=torch.int64).to(device, non_blocking=True)
            status.index_copy_(0, idx, st_d[:len(recs)])
            iters.index_copy_(0, idx, st_d[len(recs):])
        return out, status, iters

    out, status, iters = staged_upload(device, rec_off + rec_bytes, fill, run)
    STATS["frames"] += len(recs)
    STATS["fallback"] += len(host_frames)
    STATS["last_sync_iters"] = iters
    return out, status
