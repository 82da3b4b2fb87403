"""PointPillars LiDAR branch: pillar feature encoder + scatter to the BEV map.

Mirrors (state_dict-compatible) of
  PFNLayer / PillarVFE      unidistill/layers/blocks_3d/det3d/vfe/pillar_vfe.py:8-145
  PointPillarScatter        unidistill/layers/blocks_2d/det3d/map_to_bev/pointpillar_scatter.py:5-40
and PillarLidarEncoder, the cheap counterpart of layers.lidar.LidarEncoder: points -> voxelizer on a one-cell-high grid ->
PillarVFE + PointPillarScatter in one pass (ops/pillars.py, csrc/pillars.hip) -> [B, C, ny, nx].
"""
import torch
from torch import nn

from ..ops import pillars as P
from ..ops import spconv as sp
from ..ops.voxelize import Voxelization, voxelize_confirm, voxelize_deferred, voxelize_dirty
from .base import BaseEncoder


class PFNLayer(nn.Module):
    """Linear (no bias) + BatchNorm1d(eps 1e-3, momentum 0.01) + ReLU + max over the rows.  Only the layer the fused kernel
    implements exists: use_norm=True, last_layer=True."""

    def __init__(self, in_channels, out_channels, use_norm=True, last_layer=False):
        super().__init__()
        if not use_norm:
            raise NotImplementedError("PFNLayer: use_norm=False has no kernel (csrc/pillars.hip folds a BatchNorm1d)")
        if not last_layer:
            raise NotImplementedError("PFNLayer: only the last layer of a PillarVFE has a kernel; stacked PFN layers "
                                      "(len(num_filters) > 1) are not implemented")
        self.last_vfe = last_layer
        self.use_norm = use_norm
        self.linear = nn.Linear(in_channels, out_channels, bias=False)
        self.norm = nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01)


class PillarVFE(nn.Module):
    """forward(voxel_features [M, P, F], voxel_coords i32[M, 4] (b, z, y, x), voxel_num_points [M]) -> [M, C].

    ``fuse(scatter)`` ties a PointPillarScatter to this module: forward then writes the BEV map in the same pass and leaves it
    on the returned features, where that scatter's forward finds it (``batch_size=`` spares the host read that sizes the map)."""

    def __init__(self, use_norm, with_distance, use_absolute_xyz, num_filters, num_point_features, voxel_size,
                 point_cloud_range):
        super().__init__()
        self.use_norm = use_norm
        self.with_distance = with_distance
        self.use_absolute_xyz = use_absolute_xyz
        self.num_point_features = num_point_features
        self.num_filters = list(num_filters)
        assert len(self.num_filters) > 0
        if len(self.num_filters) > 1:
            raise NotImplementedError(f"PillarVFE: num_filters={self.num_filters} asks for stacked PFN layers; the fused kernel "
                                      "implements one PFN layer (len(num_filters) == 1), as every stock PointPillars config uses")
        k = P.feature_count(num_point_features, use_absolute_xyz, with_distance)
        self.pfn_layers = nn.ModuleList([PFNLayer(k, self.num_filters[0], self.use_norm, last_layer=True)])
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.voxel_x, self.voxel_y, self.voxel_z = self.voxel_size
        self.x_offset = self.voxel_x / 2 + self.point_cloud_range[0]
        self.y_offset = self.voxel_y / 2 + self.point_cloud_range[1]
        self.z_offset = self.voxel_z / 2 + self.point_cloud_range[2]
        self._scatter = None

    def get_output_feature_dim(self):
        return self.num_filters[-1]

    def fuse(self, scatter):
        object.__setattr__(self, "_scatter", scatter)      # not a sub-module: the state_dict keeps the reference's keys
        return self

    def encode(self, voxels, coords, num, batch_size, ny, nx, return_pillars=False):
        pfn = self.pfn_layers[0]
        return P.pillar_encode(voxels[:, :, :self.num_point_features] if voxels.shape[2] != self.num_point_features else voxels,
                               coords, num, pfn.linear.weight, pfn.norm, batch_size, ny, nx, self.voxel_size,
                               self.point_cloud_range, self.use_absolute_xyz, self.with_distance, return_pillars=return_pillars)

    def forward(self, voxel_features, voxel_coords, voxel_num_points, batch_size=None, **kwargs):
        sc = self._scatter
        if sc is None:      # the [M, C] features alone: a one-cell map takes the scatter's place
            _, feats = self.encode(voxel_features, voxel_coords, voxel_num_points, 1, 1, 1, return_pillars=True)
            return feats
        if batch_size is None:
            batch_size = int(voxel_coords[:, 0].max()) + 1      # pointpillar_scatter.py:15
        bev, feats = self.encode(voxel_features, voxel_coords, voxel_num_points, batch_size, sc.ny, sc.nx, return_pillars=True)
        feats._ud_pillar_bev = (bev, voxel_coords)
        return feats


class PointPillarScatter(nn.Module):
    """forward(pillar_features [M, C], voxel_coords i32[M, 4]) -> [B, C * nz, ny, nx] (nz == 1), zero where no pillar lies."""

    def __init__(self, num_bev_features, grid_size):
        super().__init__()
        self.num_bev_features = num_bev_features
        self.nx, self.ny, self.nz = [int(v) for v in grid_size]
        assert self.nz == 1

    def forward(self, pillar_features, voxel_coords, batch_size=None, **kwargs):
        fused = getattr(pillar_features, "_ud_pillar_bev", None)
        if fused is not None and fused[1] is voxel_coords:
            return fused[0]
        if batch_size is None:
            batch_size = int(voxel_coords[:, 0].max()) + 1
        x = sp.SparseConvTensor(pillar_features.contiguous(), voxel_coords.int(), (1, self.ny, self.nx), batch_size)
        return x.bev()


class PillarLidarEncoder(BaseEncoder):
    """points -> voxelize (one cell high) -> PillarVFE + PointPillarScatter (one pass) -> [B, C, ny, nx], channels-last memory.

    cfg needs: voxel_size, point_cloud_range, grid_size (nz == 1), max_num_points, max_voxels, src_num_point_features,
    use_num_point_features, num_filters; optional use_absolute_xyz (True), with_distance (False).
    frozen_encoder / frozen_bn: the reference's BaseEncoder switches (layers/base.py), applied by train().
    """

    def __init__(self, cfg, frozen_encoder=False, frozen_bn=False):
        super().__init__(frozen_encoder, frozen_bn)
        self.cfg = cfg
        g = (lambda k, *d: cfg.get(k, *d)) if isinstance(cfg, dict) else (lambda k, *d: getattr(cfg, k, *d))
        grid = [int(v) for v in g("grid_size")]
        self.voxelizer = Voxelization(voxel_size=g("voxel_size"), point_cloud_range=g("point_cloud_range"),
                                      max_num_points=g("max_num_points"), max_voxels=g("max_voxels"),
                                      num_point_features=g("src_num_point_features"), device=torch.device("cuda"))
        assert [int(v) for v in self.voxelizer.grid_size] == grid and grid[2] == 1, (self.voxelizer.grid_size, grid)
        self.vfe = PillarVFE(use_norm=True, with_distance=g("with_distance", False), use_absolute_xyz=g("use_absolute_xyz", True),
                             num_filters=g("num_filters"), num_point_features=g("use_num_point_features"),
                             voxel_size=g("voxel_size"), point_cloud_range=g("point_cloud_range"))
        self.map_to_bev = PointPillarScatter(num_bev_features=self.vfe.get_output_feature_dim(), grid_size=grid)
        self.vfe.fuse(self.map_to_bev)

    one_read = True        # False: voxelize_batch's own read per call (tests)

    def prepare(self, lidar_points):
        """Everything of a pass that sizes tensors from device-side counts: -> (voxels [M, P, F], coords, num, B).  Equal-length
        clouds (the collate_fn case) take ONE host read, for the voxel count and the voxelizer's overflow word."""
        pts = lidar_points if isinstance(lidar_points, (list, tuple)) else [lidar_points]
        vz = self.voxelizer
        overflowed = False
        if self.one_read and all(p.shape == pts[0].shape for p in pts):
            batch = torch.stack(list(pts), 0) if len(pts) > 1 else pts[0].unsqueeze(0)
            B = batch.shape[0]
            vox, coords, num, _, m_out, _ = voxelize_deferred(batch, vz.voxel_size, vz.point_cloud_range, vz.max_num_points,
                                                              vz.max_voxels, want_voxels=True, want_mean=False)
            host = m_out[B:B + 2].cpu()                                     # THE host read of this encoder pass
            if int(host[1]) == 0:
                voxelize_confirm(batch.device)
                M = int(host[0])
                return vox[:M], coords[:M], num[:M], B
            overflowed = True
            voxelize_dirty(batch.device)
        voxels, coords, num = vz(lidar_points, algo=1 if overflowed else None)
        return voxels, coords, num, len(pts)

    def forward(self, lidar_points, prepared=None):
        voxels, coords, num, B = prepared if prepared is not None else self.prepare(lidar_points)
        sc = self.map_to_bev
        return self.vfe.encode(voxels, coords, num, B, sc.ny, sc.nx)
