"""PointPillars LiDAR encoder at the workload's size: B = 4, the 30 k-point synthetic cloud, config.PILLAR_ENCODER (0.6 m pillars,
180 x 180 x 1 grid, 20 points per pillar, 256 channels).  Forward and forward + backward of PillarLidarEncoder (csrc/pillars.hip)
against the reference formulation written with PyTorch ops on the same device (same voxelizer output) and against LidarEncoder
(the sparse VoxelResBackBone8x) on the same clouds; HIP events, the paths alternated in one process, medians of 5.  Prints one
JSON line.  Run it under a time limit:  timeout -k 10 300 python tools/time_pillars.py"""
import os as _os; _os.environ.setdefault("UD_RANDOM_INIT", "1")
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
import torch
import torch.nn.functional as F
from unidistill_amd import config as C, synthetic as syn
from unidistill_amd.layers.lidar import LidarEncoder
from unidistill_amd.layers.pillars import PillarLidarEncoder

assert torch.cuda.is_available(), "time_pillars.py measures on the GPU only"
dev = torch.device("cuda:0")
B = 4
g = syn.rng(0)
points = [p for p in torch.from_numpy(syn.pad_clouds([syn.lidar_cloud(g, 30000, 1) for _ in range(B)])).to(dev)]
torch.manual_seed(0)
pillar = PillarLidarEncoder(C.PILLAR_ENCODER).to(dev).train()
sparse = LidarEncoder(C.LIDAR_ENCODER).to(dev).train()
pfn, sc = pillar.vfe.pfn_layers[0], pillar.map_to_bev
voxels, coords, num, _ = pillar.prepare(points)
M, P, Fp = voxels.shape
gy = torch.randn(B, 256, sc.ny, sc.nx, device=dev).contiguous(memory_format=torch.channels_last)


def torch_encoder(voxels, coords, num):
    """PillarVFE.forward + PFNLayer.forward + PointPillarScatter.forward as the reference writes them, on the device."""
    v = pillar.vfe
    xyz = voxels[:, :, :3]
    mean = xyz.sum(1, keepdim=True) / num.type_as(voxels).view(-1, 1, 1)
    centre = torch.stack([coords[:, 3].float() * v.voxel_x + v.x_offset, coords[:, 2].float() * v.voxel_y + v.y_offset,
                          coords[:, 1].float() * v.voxel_z + v.z_offset], 1)
    feats = torch.cat([voxels, xyz - mean, xyz - centre[:, None]], -1)
    feats = feats * (torch.arange(P, device=dev)[None] < num[:, None]).unsqueeze(-1).type_as(voxels)
    x = F.linear(feats, pfn.linear.weight)
    x = F.batch_norm(x.permute(0, 2, 1), None, None, pfn.norm.weight, pfn.norm.bias, True, 0.01, 1e-3).permute(0, 2, 1)
    x = torch.relu(x).max(1)[0]
    bev = torch.zeros(B, sc.ny * sc.nx, 256, device=dev)
    bev[coords[:, 0].long(), (coords[:, 2] * sc.nx + coords[:, 3]).long()] = x
    return bev.view(B, sc.ny, sc.nx, 256).permute(0, 3, 1, 2)


def fwd(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def fwd_bwd(fn, params):
    def run():
        for p in params:
            p.grad = None
        fn().backward(gy)
    return run


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


pp, sp_ = list(pillar.parameters()), list(sparse.parameters())
paths = {
    "pillar_op_fwd_ms": (fwd(lambda: pillar(points, (voxels, coords, num, B))), 50),
    "pillar_op_fwd_bwd_ms": (fwd_bwd(lambda: pillar(points, (voxels, coords, num, B)), pp), 50),
    "pillar_encoder_fwd_ms": (fwd(lambda: pillar(points)), 20),
    "pillar_encoder_fwd_bwd_ms": (fwd_bwd(lambda: pillar(points), pp), 20),
    "torch_ops_fwd_ms": (fwd(lambda: torch_encoder(voxels, coords, num)), 20),
    "torch_ops_fwd_bwd_ms": (fwd_bwd(lambda: torch_encoder(voxels, coords, num), pp), 20),
    "sparse_encoder_fwd_ms": (fwd(lambda: sparse(points)), 5),
    "sparse_encoder_fwd_bwd_ms": (fwd_bwd(lambda: sparse(points), sp_), 5),
}
for fn, _n in paths.values():
    for _ in range(3):
        fn()
res = {k: [] for k in paths}
for rep in range(5):                    # alternate the paths so that clock / neighbour drift hits all alike
    for k, (fn, n) in paths.items():
        res[k].append(timed(fn, n))
out = {"B": B, "pillars": int(M), "points_per_pillar": int(P), "point_features": int(Fp), "channels": 256,
       "voxels_mbytes": round(M * P * Fp * 4 / 1e6, 2), "bev_mbytes": round(B * 256 * sc.ny * sc.nx * 4 / 1e6, 2)}
out.update({k: round(sorted(v)[len(v) // 2], 4) for k, v in res.items()})
print(json.dumps(out))
