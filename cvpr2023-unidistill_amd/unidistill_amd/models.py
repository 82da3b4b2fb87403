"""BEVFusion detector (camera / LiDAR / fusion) with the CenterPoint IoU-aware head.

Mirrors, with state_dict-compatible sub-module names,
  BEVFusion / BEVFusionCenterHead / CameraEncoder / DetHead
      unidistill/exps/multisensor_fusion/nuscenes/BEVFusion/BEVFusion_nuscenes_base_exp.py:88-104,
      :164-259;  BEVFusion_nuscenes_centerhead_fusion_exp.py:44-171
  BaseMultiSensorFusion.with_* properties   unidistill/models/multisensor_fusion/base.py:12-40
"""
import torch
from torch import nn

from .layers.base import BaseEncoder
from .layers.bev import BevEncoder, FusionEncoder
from .layers.center_head import CenterHeadIouAware, FCOSAssigner
from .layers.gen_proposals import IouAwareGenProposals
from .layers.lidar import LidarEncoder
from .layers.pillars import PillarLidarEncoder
from .layers.lss_fpn import LSSFPN
from .ops.distill import feature_tap


class CameraEncoder(BaseEncoder):
    """frozen_encoder / frozen_bn: the reference's BaseEncoder switches (layers/base.py), applied by train(); the image
    backbone's own frozen_stages / norm_eval (layers/image.ResNet.train) compose with them."""

    def __init__(self, camera_encoder_cfg, frozen_encoder=False, frozen_bn=False, **kw):
        super().__init__(frozen_encoder, frozen_bn)
        self.backbone = LSSFPN(**camera_encoder_cfg, **kw)

    def forward(self, imgs, mats_dict, is_return_depth=False):
        return self.backbone(imgs, mats_dict, is_return_depth=is_return_depth)


class DetHead(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.det_head_cfg = cfg
        names = [n for t in cfg["tasks"] for n in t["class_names"]]
        assigner = FCOSAssigner(
            out_size_factor=cfg["out_size_factor"], tasks=cfg["tasks"], dense_reg=cfg["dense_reg"],
            gaussian_overlap=cfg["gaussian_overlap"], max_objs=cfg["max_objs"],
            min_radius=cfg["min_radius"], mapping={n: i + 1 for i, n in enumerate(names)},
            grid_size=cfg["grid_size"], pc_range=cfg["point_cloud_range"][0:2],
            voxel_size=cfg["voxel_size"][0:2], assign_topk=cfg["assign_topk"],
            with_velocity=cfg["with_velocity"])
        prop = cfg.get("proposal")
        proposal_layer = None
        if prop is not None:      # BEVFusion_nuscenes_centerhead_fusion_exp.py:67-84
            proposal_layer = IouAwareGenProposals(
                dataset_name="nuscenes", class_names=[t["class_names"] for t in cfg["tasks"]],
                post_center_limit_range=prop["post_center_limit_range"], score_threshold=prop["score_threshold"],
                pc_range=cfg["point_cloud_range"][0:2], out_size_factor=cfg["out_size_factor"],
                voxel_size=cfg["voxel_size"][0:2], no_log=prop["no_log"], iou_aware_list=prop["iou_aware_list"],
                nms_iou_threshold_train=prop["nms_iou_threshold_train"],
                nms_pre_max_size_train=prop["nms_pre_max_size_train"],
                nms_post_max_size_train=prop["nms_post_max_size_train"],
                nms_iou_threshold_test=prop["nms_iou_threshold_test"],
                nms_pre_max_size_test=prop["nms_pre_max_size_test"],
                nms_post_max_size_test=prop["nms_post_max_size_test"])
        self.dense_head = CenterHeadIouAware(
            dataset_name="nuscenes", tasks=cfg["tasks"], target_assigner=assigner, proposal_layer=proposal_layer,
            out_size_factor=cfg["out_size_factor"], input_channels=cfg["input_channels"],
            grid_size=cfg["grid_size"], point_cloud_range=cfg["point_cloud_range"],
            code_weights=cfg["code_weights"], loc_weight=cfg["loc_weight"], iou_weight=cfg["iou_weight"],
            share_conv_channel=cfg["share_conv_channel"], common_heads=cfg["common_heads"],
            init_bias=cfg["init_bias"], focal_alpha=cfg["focal_alpha"], focal_gamma=cfg["focal_gamma"],
            voxel_size_xy=cfg["voxel_size"][0:2], iou_mode=cfg.get("iou_mode", "reference"))

    def forward(self, x, gt_boxes, targets=None, response_mask=None):
        ret = (self.dense_head(x, gt_boxes, targets=targets) if response_mask is None else
               self.dense_head(x, gt_boxes, targets=targets, response_mask=response_mask))
        # precomputed targets are cleaned by whoever built them and say so (train.DistillStep.prep); anything else is cleaned here
        if self.training and "box_encoding" in ret and not (targets is not None and targets.get("box_encoding_clean")):
            for enc in ret["box_encoding"].values():
                enc[torch.isinf(enc)] = 0          # log(0) of zero-size boxes (fusion_exp.py:124-126)
        return ret


LIDAR_ENCODER_CLASSES = {"sparse": LidarEncoder, "pillars": PillarLidarEncoder}


def lidar_encoder_class(cfg):
    """The encoder class a lidar_encoder cfg asks for by its optional 'type' key; without one, LidarEncoder."""
    kind = (cfg.get("type", "sparse") if isinstance(cfg, dict) else getattr(cfg, "type", "sparse"))
    if kind not in LIDAR_ENCODER_CLASSES:
        raise ValueError(f"lidar_encoder type: expected one of {sorted(LIDAR_ENCODER_CLASSES)}, got {kind!r}")
    return LIDAR_ENCODER_CLASSES[kind]


class BEVFusionCenterHead(nn.Module):
    """forward(lidar_points, cameras_imgs, metas, gt_boxes, return_feature=False)

    training:            (ret_dict{'loss'}, tb_dict, bev_feat, trunk_out, multi_head_features, {})
    return_feature=True: (bev_feat, trunk_out, multi_head_features)
    eval:                the proposal layer's dict: pred_dicts (boxes / scores / labels per sample), rois,
                         roi_scores, roi_labels (layers/gen_proposals.py, rotated NMS on the HIP library)
    """

    def __init__(self, model_cfg, camera_kwargs=None, lidar_kwargs=None):
        """camera_kwargs / lidar_kwargs (and model_cfg["camera_encoder_kwargs"] / ["lidar_encoder_kwargs"], which they
        override): constructor arguments of the two encoders beyond their cfg, e.g. frozen_bn=True, frozen_encoder=True."""
        super().__init__()
        self.cfg = model_cfg
        self.class_names = model_cfg["class_names"]
        self.num_class = len(self.class_names)
        lidar_kwargs = {**(model_cfg.get("lidar_encoder_kwargs") or {}), **(lidar_kwargs or {})}
        camera_kwargs = {**(model_cfg.get("camera_encoder_kwargs") or {}), **(camera_kwargs or {})}
        self.lidar_encoder = (lidar_encoder_class(model_cfg["lidar_encoder"])(model_cfg["lidar_encoder"], **lidar_kwargs)
                              if model_cfg.get("lidar_encoder") else None)
        self.camera_encoder = (CameraEncoder(model_cfg["camera_encoder"], **camera_kwargs)
                               if model_cfg.get("camera_encoder") else None)
        both = self.lidar_encoder is not None and self.camera_encoder is not None
        self.fusion_encoder = FusionEncoder(use_elementwise=False) if both else None
        self.bev_encoder = BevEncoder(model_cfg["bev_encoder"])
        self.det_head = DetHead(model_cfg["det_head"])

    with_lidar_encoder = property(lambda self: self.lidar_encoder is not None)
    with_camera_encoder = property(lambda self: self.camera_encoder is not None)
    with_fusion_encoder = property(lambda self: self.fusion_encoder is not None)

    def extract_bev(self, lidar_points, cameras_imgs, metas, lidar_prepared=None, return_depth_logits=False):
        """return_depth_logits: -> (bev, the camera encoder's key-frame depth logits)."""
        lidar_out = camera_out = depth_logits = None
        if self.with_lidar_encoder:
            lidar_out = self.lidar_encoder(lidar_points, lidar_prepared)
        if self.with_camera_encoder and return_depth_logits:
            camera_out, depth_logits = self.camera_encoder(cameras_imgs, metas, is_return_depth="logits")
        elif self.with_camera_encoder:
            camera_out = self.camera_encoder(cameras_imgs, metas)
        if self.with_fusion_encoder:
            bev = self.fusion_encoder(lidar_out, camera_out)
        else:
            bev = camera_out if camera_out is not None else lidar_out
        return (bev, depth_logits) if return_depth_logits else bev

    def forward(self, lidar_points=None, cameras_imgs=None, metas=None, gt_boxes=None,
                return_feature=False, targets=None, loss_norm=None, lidar_prepared=None, depth_label=None,
                depth_weight=None, return_depth_logits=False, response_mask=None, **_):
        """targets / loss_norm: optional precomputed FCOS targets and globally reduced loss
        normalisers (train.py computes them up front so the network pass holds no collective);
        lidar_prepared: LidarEncoder.prepare(lidar_points), when the caller ran it ahead of time;
        depth_label / depth_weight: LiDAR depth-bin labels i32[B, ncam, fH, fW] (LSSFPN.lidar_depth_labels) and the weight
        of the depth loss (BEVDepth: 3.0).  With both, in training, on a model with a camera encoder,
        depth_weight * ops.depth_sup.depth_loss joins ret['loss'] and tb['loss_depth'] holds the unweighted term.
        return_depth_logits: in eval mode, on a model with a camera encoder, the returned dict also holds 'depth_logits',
        the key frame's depth logits [B * ncam, D, fH, fW] of this very forward (evaluation.DepthMetric reads them)."""
        depth_sup = (depth_label is not None and depth_weight is not None and self.training and not return_feature
                     and self.with_camera_encoder)
        eval_logits = return_depth_logits and not self.training and not return_feature and self.with_camera_encoder
        depth_logits = None
        if depth_sup or eval_logits:
            bev, depth_logits = self.extract_bev(lidar_points, cameras_imgs, metas, lidar_prepared, return_depth_logits=True)
        else:
            bev = self.extract_bev(lidar_points, cameras_imgs, metas, lidar_prepared)
        tapped = self.training and not return_feature
        # the two maps the box distillation losses read: their gradients join the network branch's inside one kernel (ops/distill.py)
        bev, bev_out = feature_tap(bev) if tapped else (bev, bev)
        trunk, _ = self.bev_encoder(bev)
        trunk, trunk_out = feature_tap(trunk) if tapped else (trunk, trunk)
        # response_mask (train.DistillStep.teacher): the head maps are read weighted by it only -- feature requests alone
        ret = self.det_head(trunk, gt_boxes, targets=targets, response_mask=response_mask if return_feature else None)
        if return_feature:
            return bev, trunk, ret["multi_head_features"]
        if self.training:
            loss, tb = self.det_head.dense_head.get_loss(ret, norm=loss_norm)
            tb["loss_rpn"] = loss.detach()
            if depth_sup:
                from .ops.depth_sup import depth_loss
                loss_depth = depth_loss(depth_logits, depth_label)
                loss = loss + depth_weight * loss_depth
                tb["loss_depth"] = loss_depth.detach()
            return {"loss": loss}, tb, bev_out, trunk_out, ret["multi_head_features"], {}
        if eval_logits:
            ret["depth_logits"] = depth_logits
        return ret
