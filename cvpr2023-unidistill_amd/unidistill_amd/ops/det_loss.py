"""Fused detection-loss terms of the CenterPoint heads (ud_det_focal_*, ud_det_reg_*).

CenterHeadIouAware.get_loss (reference layers/head/det3d/center_head_iou_aware.py:55-298; FocalLoss and
CenterNetRegLoss of layers/losses/det3d.py:287-421) evaluates ~330 small tensor ops per step; here the
focal term over all heat maps and the gathered regression / IoU terms are one forward kernel each, with
the local derivatives kept for a scale-and-scatter backward.

``iou_mode="rotated3d"`` (opt-in) replaces the reference's axis-aligned IoU loss and nearest-BEV IoU-aware target by the
rotated 3-D IoU of the decoded boxes (ud_det_reg_*_rot); ``rotated_iou3d`` is that IoU as a pairwise op on plain boxes.
"""
import ctypes

import torch

from .. import _lib

HEADS = ("reg", "height", "dim", "rot", "vel", "iou")       # gathered order: 2+1+3+2+2+1 = 11 values
WIDTH = (2, 1, 3, 2, 2, 1)
IOU_MODES = ("reference", "rotated3d")


def check_iou_mode(iou_mode):
    if iou_mode not in IOU_MODES:
        raise ValueError(f"iou_mode must be one of {IOU_MODES}, got {iou_mode!r}")
    return iou_mode


def supported(preds, nb):
    """All head tensors fp32 CUDA [B, c, H, W] with contiguous H*W planes, nuScenes code size."""
    if nb != 10 or len(preds) > 8:
        return False
    for pd in preds:
        for name in ("hm",) + HEADS:
            t = pd.get(name)
            if t is None or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
                return False
            if t.stride(3) != 1 or t.stride(2) != t.shape[3] or t.stride(1) != t.shape[2] * t.shape[3]:
                return False
    return True


def _ptr_table(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


class _FocalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gt, alpha, gamma, *hms):
        lib = _lib.load()
        T = len(hms)
        B, _, H, W = hms[0].shape
        ncm = gt.shape[2]
        ncls = [int(h.shape[1]) for h in hms]
        gt = gt.contiguous().float()
        prob = torch.empty((T, B, ncm, H, W), dtype=torch.float32, device=gt.device)
        pos_neg = torch.empty((T, 2), dtype=torch.float32, device=gt.device)
        ws = _lib.workspace(gt.device, lib.ud_det_loss_workspace_bytes(T), "det_loss")
        _lib.ud.ud_det_focal_fwd(_ptr_table(hms), (ctypes.c_longlong * T)(*[h.stride(0) for h in hms]),
                                 (ctypes.c_int * T)(*ncls), T, B, ncm, H * W, gt, float(alpha), float(gamma), prob, pos_neg, ws,
                                 ws.numel(), _lib.stream_of(gt))
        ctx.save_for_backward(gt, prob)
        ctx.cfg = (ncls, float(alpha), float(gamma))
        return prob, pos_neg[:, 0], pos_neg[:, 1]

    @staticmethod
    def backward(ctx, g_prob, g_pos, g_neg):
        gt, prob = ctx.saved_tensors
        ncls, alpha, gamma = ctx.cfg
        T, B, ncm, H, W = prob.shape
        dl = torch.empty_like(prob)
        gp = None if g_prob is None else g_prob.contiguous().float()
        _lib.ud.ud_det_focal_bwd((ctypes.c_int * T)(*ncls), T, B, ncm, H * W, gt, prob, gp, g_pos.contiguous().float(),
                                 g_neg.contiguous().float(), alpha, gamma, dl, _lib.stream_of(prob))
        return (None, None, None) + tuple(dl[t, :, :ncls[t]] for t in range(T))


def focal_terms(hms, gt, alpha, gamma):
    """hms: T logits tensors [B, ncls_t, H, W]; gt [T, B, ncm, H, W]  ->  (prob [T,B,ncm,H,W], pos [T], neg [T])."""
    return _FocalFn.apply(gt, alpha, gamma, *hms)


class _RegFn(torch.autograd.Function):
    FWD, BWD, LOC = "ud_det_reg_fwd", "ud_det_reg_bwd", 17      # entry points and saved derivatives per slot

    @staticmethod
    def forward(ctx, ind, mask, tgt, num_obj, sx, sy, nb, *heads):
        """heads: T * 6 tensors in HEADS order per task."""
        lib = _lib.load()
        T = len(heads) // len(HEADS)
        B, _, H, W = heads[0].shape
        K = ind.shape[2]
        planes, strides = [], []
        for t in range(T):
            for h, wd in zip(heads[t * 6:(t + 1) * 6], WIDTH):
                assert h.shape[1] == wd
                for c in range(wd):
                    planes.append(h[:, c])
                    strides.append(h.stride(0))
        table = (ctypes.c_void_p * len(planes))(*[p.data_ptr() for p in planes])
        ind = ind.contiguous()
        mask_u8 = mask.to(torch.uint8).contiguous()
        tgt = tgt.contiguous().float()
        num_obj = num_obj.contiguous().float()
        dev = ind.device
        losses = torch.empty((T, 12), dtype=torch.float32, device=dev)
        loc = torch.empty((T, B, K, ctx._forward_cls.LOC), dtype=torch.float32, device=dev)
        ws = _lib.workspace(dev, lib.ud_det_loss_workspace_bytes(T), "det_loss")
        fwd = ctx._forward_cls.FWD
        getattr(_lib.ud, fwd)(table, (ctypes.c_longlong * len(strides))(*strides), T, B, K, H * W, nb, ind, mask_u8, tgt,
                              tgt.shape[-1], num_obj, float(sx), float(sy), losses, loc, ws, ws.numel(), _lib.stream_of(ind))
        ctx.save_for_backward(ind, mask_u8, loc)
        ctx.cfg = (T, B, K, H, W, nb)
        return losses[:, :10], losses[:, 10], losses[:, 11]

    @staticmethod
    def backward(ctx, g_box, g_iou, g_aw):
        ind, mask_u8, loc = ctx.saved_tensors
        T, B, K, H, W, nb = ctx.cfg
        dhead = torch.zeros((T, B, 11, H, W), dtype=torch.float32, device=ind.device)
        z = lambda g, shape: (torch.zeros(shape, device=ind.device) if g is None else g.contiguous().float())
        bwd = ctx._forward_cls.BWD
        getattr(_lib.ud, bwd)(T, B, K, H * W, nb, ind, mask_u8, loc, z(g_box, (T, 10)), z(g_iou, (T,)), z(g_aw, (T,)), dhead,
                              _lib.stream_of(ind))
        grads = []
        for t in range(T):
            c = 0
            for wd in WIDTH:
                grads.append(dhead[t, :, c:c + wd])
                c += wd
        return (None,) * 7 + tuple(grads)


class _RegRotFn(_RegFn):
    """The same terms with the rotated 3-D IoU (ud_det_reg_*_rot): 19 saved derivatives per slot, gradients reach rot too."""
    FWD, BWD, LOC = "ud_det_reg_fwd_rot", "ud_det_reg_bwd_rot", 19


def reg_terms(preds, ind, mask, tgt, num_obj, sx, sy, nb=10, iou_mode="reference"):
    """preds: per-task dicts of head tensors; ind/mask [T,B,K], tgt [T,B,K,>=nb], num_obj [T]
    -> (box_loss [T,10], iou_loss [T], iou_aware [T]) normalised like the reference.
    iou_mode "reference": the reference's axis-aligned IoU loss and nearest-BEV IoU-aware target; "rotated3d": both from the
    rotated 3-D IoU of the decoded prediction and target (box_loss is the same either way).  Gradients go to the heads only.
    Precondition: the positive (mask) slots of one (task, sample) name pairwise distinct pixels in ``ind``.  The backward stores a slot's
    gradient at its pixel and does not accumulate, so a second positive slot on the same pixel would silently lose one of the two.  The
    assigner's output satisfies it (one positive slot per anchor point; tests/test_dense_head.py, tests/test_det_loss_reference_gpu.py)."""
    heads = [pd[name] for pd in preds for name in HEADS]
    fn = _RegFn
    if check_iou_mode(iou_mode) == "rotated3d":
        _lib.require_gpu(ind, *heads)
        fn = _RegRotFn
    return fn.apply(ind, mask, tgt, num_obj, sx, sy, nb, *heads)


class _RotIou3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        n = a.shape[0]
        iou = torch.empty((n,), dtype=torch.float32, device=a.device)
        diou = torch.empty((n, 7), dtype=torch.float32, device=a.device) if ctx.needs_input_grad[0] else None
        _lib.ud.ud_rot_iou3d_pairs(a, b, n, iou, diou, _lib.stream_of(a))
        if diou is not None:
            ctx.save_for_backward(diou)
        return iou

    @staticmethod
    def backward(ctx, g):
        diou, = ctx.saved_tensors
        return g[:, None] * diou, None


def rotated_iou3d(a, b):
    """a, b: fp32 GPU boxes [N,7] (x, y, z, dx, dy, dz, yaw) -> IoU3D_rot(a[i], b[i]) [N]: area of the intersection of the
    two rotated rectangles x z-overlap, over the union (floor 1e-8).  Differentiable in a; b is a constant."""
    _lib.require_gpu(a, b)
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise TypeError(f"rotated_iou3d takes float32 boxes, got {a.dtype} and {b.dtype}")
    if a.dim() != 2 or a.shape[1] != 7 or a.shape != b.shape:
        raise ValueError(f"rotated_iou3d takes two [N, 7] box tensors, got {tuple(a.shape)} and {tuple(b.shape)}")
    return _RotIou3dFn.apply(a.contiguous(), b.detach().contiguous())
