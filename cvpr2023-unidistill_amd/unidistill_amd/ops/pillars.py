"""PointPillars encoder op: PillarVFE's feature augmentation + one PFNLayer (Linear, BatchNorm1d, ReLU, max over the rows)
+ PointPillarScatter as one autograd Function on csrc/pillars.hip.

Reference: unidistill/layers/blocks_3d/det3d/vfe/pillar_vfe.py:8-145,
unidistill/layers/blocks_2d/det3d/map_to_bev/pointpillar_scatter.py:5-40.
"""
import ctypes

import torch

from .. import _lib
from .spconv import folded_batchnorm

ABS_XYZ, DISTANCE = 1, 2


def feature_count(F, use_absolute_xyz=True, with_distance=False):
    """K, the PFNLayer's input width for F point features."""
    return F + (6 if use_absolute_xyz else 3) + (1 if with_distance else 0)


def cell_geometry(voxel_size, point_cloud_range):
    """(vx, vy, vz, x_offset, y_offset, z_offset): the offsets evaluated in double as PillarVFE.__init__ does
    (pillar_vfe.py:88-93), rounded to fp32 where they meet the fp32 coordinates."""
    v = [float(x) for x in voxel_size]
    return tuple(v) + tuple(v[i] / 2 + float(point_cloud_range[i]) for i in range(3))


def _geom(geometry):
    return (ctypes.c_float * 6)(*[float(x) for x in geometry])


class _PillarEncode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, gamma, beta, voxels, coords, num, bn_state, cfg):
        geometry, flags, B, ny, nx, return_pillars = cfg
        running_mean, running_var, eps, momentum, training, folded = bn_state
        M, P, F = voxels.shape
        C, K = weight.shape
        dev = voxels.device
        stream = _lib.stream_of(voxels)
        geom = _geom(geometry)
        w = weight.detach().float().contiguous()
        need = _lib.load().ud_pillar_workspace_bytes(M, P, F, C, flags)
        if need == 0:
            raise ValueError(f"pillar_encode: unsupported sizes M={M} P={P} F={F} C={C} (C % 32 == 0, C <= 256, 3 <= F <= 8, "
                             "P <= 64)")
        ws = _lib.workspace(dev, need, "pillars")
        stats = torch.empty((4, C), dtype=torch.float32, device=dev)
        if training:
            if M * P <= 1:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {(M * P, C)}")
            _lib.ud.ud_pillar_stats(voxels, coords, num, M, P, F, w, C, flags, geom, gamma.detach(), beta.detach(), float(eps),
                                    float(momentum), running_mean, running_var, stats, ws, ws.numel(), stream)
            if running_mean is not None:   # written through raw pointers: tell autograd's version counters
                torch.autograd.graph.increment_version(running_mean)
                torch.autograd.graph.increment_version(running_var)
        else:
            scale, shift = folded
            stats[0] = running_mean
            stats[1] = torch.rsqrt(running_var + eps)
            stats[2] = scale
            stats[3] = shift
        grad = any(ctx.needs_input_grad[:3])
        bev = torch.empty((B, ny, nx, C), dtype=torch.float32, device=dev)
        pillars = torch.empty((M, C), dtype=torch.float32, device=dev) if return_pillars else None
        argmax = torch.empty((M, C), dtype=torch.uint8, device=dev) if grad else None
        _lib.ud.ud_pillar_apply(voxels, coords, num, M, P, F, w, C, flags, geom, stats[2], stats[3], B, ny, nx, bev, pillars,
                                argmax, stream)
        if grad:
            ctx.save_for_backward(w, voxels, coords, num, stats, argmax)
            ctx.cfg = (geom, flags, B, ny, nx, not training)
        out = bev.permute(0, 3, 1, 2)
        return (out, pillars) if return_pillars else out

    @staticmethod
    def backward(ctx, gbev, gpillars=None):
        w, voxels, coords, num, stats, argmax = ctx.saved_tensors
        geom, flags, B, ny, nx, frozen = ctx.cfg
        M, P, F = voxels.shape
        C, K = w.shape
        if gbev is None:
            g = torch.zeros((B, ny, nx, C), dtype=torch.float32, device=voxels.device)
        else:
            g = gbev.float().permute(0, 2, 3, 1).contiguous()
        gp = None if gpillars is None else gpillars.float().contiguous()
        need_w, need_g, need_b = ctx.needs_input_grad[:3]
        dw = torch.empty((C, K), dtype=torch.float32, device=g.device) if need_w else None
        dg = torch.empty((C,), dtype=torch.float32, device=g.device) if need_g else None
        db = torch.empty((C,), dtype=torch.float32, device=g.device) if need_b else None
        ws = _lib.workspace(g.device, _lib.load().ud_pillar_workspace_bytes(M, P, F, C, flags), "pillars")
        _lib.ud.ud_pillar_bwd(voxels, coords, num, M, P, F, w, C, flags, geom, g, gp, B, ny, nx, argmax, stats,
                              1 if frozen else 0, dw, dg, db, ws, ws.numel(), _lib.stream_of(g))
        return dw, dg, db, None, None, None, None, None


def pillar_encode(voxels, coords, num, weight, bn, B, ny, nx, voxel_size, point_cloud_range, use_absolute_xyz=True,
                  with_distance=False, return_pillars=False):
    """voxels f32[M, P, F] (rows >= num zero), coords i32[M, 4] (b, z, y, x), num i32[M], weight f32[C, K], bn a BatchNorm1d(C)
    -> the BEV map [B, C, ny, nx] (channels-last memory, the layout LidarEncoder returns), and the [M, C] pillar features with
    return_pillars.  bn.training selects batch statistics (running statistics updated as torch does: unbiased variance,
    n = M * P, num_batches_tracked + 1) or the folded running statistics; both train weight, bn.weight and bn.bias.  Points carry
    no gradient."""
    _lib.require_gpu(voxels, coords, num, weight)
    if voxels.dtype != torch.float32 or voxels.dim() != 3:
        raise TypeError("voxels must be float32 [M, P, F]")
    M, P, F = voxels.shape
    C, K = weight.shape
    if K != feature_count(F, use_absolute_xyz, with_distance):
        raise ValueError(f"weight has {K} input features, the row features of F={F} points are "
                         f"{feature_count(F, use_absolute_xyz, with_distance)}")
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise NotImplementedError("pillar_encode: BatchNorm1d with affine parameters, running statistics and a fixed momentum")
    if M == 0:
        out = torch.zeros((B, ny, nx, C), dtype=torch.float32, device=voxels.device).permute(0, 3, 1, 2)
        return (out, voxels.new_zeros((0, C))) if return_pillars else out
    voxels = voxels.contiguous()
    coords = coords.int().contiguous()
    num = num.int().contiguous()
    flags = (ABS_XYZ if use_absolute_xyz else 0) | (DISTANCE if with_distance else 0)
    training = bn.training
    folded = None if training else folded_batchnorm(bn)
    bn_state = (bn.running_mean, bn.running_var, bn.eps, bn.momentum, training, folded)
    cfg = (cell_geometry(voxel_size, point_cloud_range), flags, int(B), int(ny), int(nx), bool(return_pillars))
    out = _PillarEncode.apply(weight, bn.weight, bn.bias, voxels, coords, num, bn_state, cfg)
    if training:
        with torch.no_grad():
            bn.num_batches_tracked += 1
    return out
