"""Work lists of the frozen distillation teacher's head (csrc/head_sites.hip).  The teacher's head output is read by
ResponseDistillLoss only, which weights every site by the Gaussian box mask; ``build`` turns that mask, on the device and in one
launch, into the pixel units of the first head convolution and the strips (with their rows) of the grouped tail that hold a site.
Nothing is read back: the two kernels take the lists as they are (ops/conv2d_f32.py: conv3x3_units, ops/head_tail_f32.py:
bn_relu_group_tail_sites)."""
import torch

from .. import _lib
from . import conv2d_f32


class SiteLists:
    """mask f32[B, H, W]; conv_units i32[1 + blocks] (count, ascending block indices); tail_strips i32[1 + strips] likewise;
    tail_rows i32[strips, 2] (first, end) rows of each strip's sites; plus the geometry they were built for."""

    def __init__(self, mask, conv_units, tail_strips, tail_rows, block, strip):
        self.mask, self.conv_units, self.tail_strips, self.tail_rows = mask, conv_units, tail_strips, tail_rows
        self.block, self.strip = block, strip

    def fractions(self):
        """(units kept / all units, strips kept / all strips, tail rows walked / all rows) -- reads back: measurements only."""
        rows = (self.tail_rows[:, 1] - self.tail_rows[:, 0]).clamp_(min=0).sum().item()
        B, H, W = self.mask.shape
        cols = -(-W // self.strip[0])
        return (self.conv_units[0].item() / (self.conv_units.numel() - 1), self.tail_strips[0].item() / (self.tail_strips.numel() - 1),
                rows / float(B * H * cols))


def build(mask, G, KM):
    """mask: f32 [B, H, W] or [B, 1, H, W] on the device; G, KM: the tail's groups and outputs per group (they set its strips)."""
    _lib.require_gpu(mask)
    if mask.dim() == 4:
        mask = mask[:, 0]
    mask = mask.contiguous().float()
    B, H, W = mask.shape
    lib = _lib.load()
    bw, bh = conv2d_f32.unit_block_pixels(H, W)
    sw, sh = 16, lib.ud_head_tail_f32_strip_rows(B, H, W, G, KM)
    if sh <= 0:
        raise ValueError(f"no grouped-tail launch for B={B} H={H} W={W} G={G} KM={KM}")
    nb = B * (-(-W // bw)) * (-(-H // bh))
    ns = B * (-(-W // sw)) * (-(-H // sh))
    # one allocation: [conv_units | tail_strips | tail_rows | scratch (ticket + flags, zero on entry)]
    buf = torch.zeros(2 + nb + ns + 2 * ns + 1 + nb + ns, dtype=torch.int32, device=mask.device)
    conv_units, tail_strips = buf[:1 + nb], buf[1 + nb:2 + nb + ns]
    tail_rows = buf[2 + nb + ns:2 + nb + 3 * ns].view(ns, 2)
    scratch = buf[2 + nb + 3 * ns:]
    _lib.ud.ud_head_sites_build(mask, B, H, W, bw, bh, sw, sh, conv_units, tail_strips, tail_rows, scratch, _lib.stream_of(mask))
    return SiteLists(mask, conv_units, tail_strips, tail_rows, (bw, bh), (sw, sh))
