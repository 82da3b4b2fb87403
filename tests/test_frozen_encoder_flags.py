"""CPU: the reference's BaseEncoder switches (unidistill/models/multisensor_fusion/base.py:50-67) on LidarEncoder / CameraEncoder:
frozen_bn keeps every BatchNorm under the encoder in eval through train(), frozen_encoder stops its parameter gradients; the
defaults change nothing, state_dict keys are the same, and train.build_model / the model config pass the flags through."""
import pytest
import torch
from torch.nn.modules.batchnorm import _BatchNorm

from unidistill_amd import config as C, train
from unidistill_amd.layers.lidar import LidarEncoder
from unidistill_amd.models import BEVFusionCenterHead, CameraEncoder


def _encoder(kind, **kw):
    cfg = C.model_cfg(lidar=kind == "lidar", camera=kind == "camera")
    return LidarEncoder(cfg["lidar_encoder"], **kw) if kind == "lidar" else CameraEncoder(cfg["camera_encoder"], **kw)


def _modes(enc):
    bns = [m.training for m in enc.modules() if isinstance(m, _BatchNorm)]
    rest = [m.training for m in enc.modules() if not isinstance(m, _BatchNorm)]
    assert bns and rest
    return bns, rest


def _default_bn_modes(kind):
    """What train() leaves without the flags (the image backbone freezes its stem's BatchNorm by itself)."""
    return [m.training for m in _encoder(kind).train().modules() if isinstance(m, _BatchNorm)]


@pytest.mark.parametrize("kind", ["lidar", "camera"])
def test_frozen_bn_keeps_every_batchnorm_in_eval_through_train(kind):
    enc = _encoder(kind, frozen_bn=True)
    assert enc.frozen_bn and not enc.frozen_encoder
    for _ in range(2):                                  # .train(), then .eval() -> .train(): the same state
        enc.train()
        bns, rest = _modes(enc)
        assert not any(bns) and all(rest)
        enc.eval()
        bns, rest = _modes(enc)
        assert not any(bns) and not any(rest)
    enc.train()
    # frozen_bn alone freezes no parameter beyond what the encoder freezes by itself
    assert [p.requires_grad for p in enc.parameters()] == [p.requires_grad for p in _encoder(kind).train().parameters()]
    assert any(p.requires_grad for p in enc.parameters())


@pytest.mark.parametrize("kind", ["lidar", "camera"])
def test_frozen_encoder_stops_every_parameter_gradient(kind):
    enc = _encoder(kind, frozen_encoder=True).train()
    assert enc.frozen_encoder and not enc.frozen_bn
    assert not any(p.requires_grad for p in enc.parameters())
    bns, rest = _modes(enc)
    assert bns == _default_bn_modes(kind) and all(rest)          # the BatchNorms keep training-mode statistics: not frozen_bn
    enc.eval().train()
    assert not any(p.requires_grad for p in enc.parameters())


@pytest.mark.parametrize("kind", ["lidar", "camera"])
def test_default_flags_change_nothing(kind):
    enc = _encoder(kind).train()
    assert not enc.frozen_bn and not enc.frozen_encoder
    bns, rest = _modes(enc)
    assert all(rest) and any(bns)
    if kind == "lidar":
        assert all(bns) and all(p.requires_grad for p in enc.parameters())
    else:
        # only the image backbone's own frozen stem (frozen_stages=0) is in eval / without gradient
        stem = enc.backbone.img_backbone
        frozen = {id(p) for m in (stem.conv1, stem.bn1) for p in m.parameters()}
        assert all(p.requires_grad == (id(p) not in frozen) for p in enc.parameters())
        assert [m for m in enc.modules() if isinstance(m, _BatchNorm) and not m.training] == [stem.bn1]


@pytest.mark.parametrize("kind", ["lidar", "camera"])
def test_state_dict_keys_do_not_depend_on_the_flags(kind):
    keys = list(_encoder(kind).state_dict().keys())
    assert list(_encoder(kind, frozen_bn=True, frozen_encoder=True).train().state_dict().keys()) == keys


def test_build_model_and_the_model_config_pass_the_flags_through():
    m = train.build_model("fusion", frozen_bn=True, frozen_encoder="lidar")
    assert m.lidar_encoder.frozen_bn and m.lidar_encoder.frozen_encoder
    assert m.camera_encoder.frozen_bn and not m.camera_encoder.frozen_encoder
    m.train()
    assert not any(p.requires_grad for p in m.lidar_encoder.parameters())
    assert any(p.requires_grad for p in m.camera_encoder.parameters())
    for enc in (m.lidar_encoder, m.camera_encoder):
        assert not any(b.training for b in enc.modules() if isinstance(b, _BatchNorm))
    # the trunk and the head are no encoders: their BatchNorms keep training
    assert all(b.training for b in m.bev_encoder.modules() if isinstance(b, _BatchNorm))
    plain = train.build_model("fusion")
    assert not (plain.lidar_encoder.frozen_bn or plain.lidar_encoder.frozen_encoder or plain.camera_encoder.frozen_bn
                or plain.camera_encoder.frozen_encoder)
    assert list(plain.state_dict().keys()) == list(m.state_dict().keys())
    cam = train.build_model("camera", frozen_bn=("camera",))
    assert cam.camera_encoder.frozen_bn and cam.lidar_encoder is None
    with pytest.raises(ValueError, match="frozen_bn"):
        train.build_model("camera", frozen_bn="radar")
    # the model config and the constructor arguments
    cfg = C.model_cfg(lidar=True, camera=True)
    cfg["lidar_encoder_kwargs"] = dict(frozen_encoder=True)
    m = BEVFusionCenterHead(cfg, camera_kwargs=dict(frozen_bn=True))
    assert m.lidar_encoder.frozen_encoder and not m.lidar_encoder.frozen_bn
    assert m.camera_encoder.frozen_bn and not m.camera_encoder.frozen_encoder
    m = BEVFusionCenterHead(cfg, lidar_kwargs=dict(frozen_encoder=False))
    assert not m.lidar_encoder.frozen_encoder
