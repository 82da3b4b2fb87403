"""CPU: with unidistill_amd.shims installed the UNMODIFIED reference modules import and construct on top of this library
(no kernels are launched).  The reference side is stored in tests/golden/shims_reference.npz: which extension module the
reference's lss_fpn binds, the classes its VoxelResBackBone8x / Voxelization were built from on the shims, the state-dict
shapes of its backbone and LSSFPN, and LSSFPN's frustum / voxel_coord.  Regenerate it where the reference tree is available:
    UNIDISTILL_REF=<reference checkout> python tests/test_shims_reference.py
which imports the reference modules on the shims exactly as a user of this library would and fails if they do not build."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _qualname(cls):
    return cls.__module__ + "." + cls.__qualname__


def _resolve(name):
    mod, _, attr = str(name).rpartition(".")
    return getattr(importlib.import_module(mod), attr)


def _shapes(module):
    keys = sorted(module.state_dict())
    return np.array(keys), np.array([",".join(map(str, module.state_dict()[k].shape)) for k in keys])


def _install_reference_side(ref):
    """shims.install() plus stand-ins for packages the reference imports for its data side only (not the hot path)."""
    from unidistill_amd import shims
    shims.install()
    for name in ("numba", "nuscenes", "pyquaternion", "skimage", "skimage.io", "cv2", "torchvision",
                 "torchvision.ops", "sklearn", "sklearn.datasets", "pytorch_lightning",
                 "pytorch_lightning.core"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
    sys.modules["numba"].jit = sys.modules["numba"].njit = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
    sys.modules["torchvision.ops"].roi_align = None
    sys.modules["sklearn.datasets"].load_sample_images = None
    sys.modules["pyquaternion"].Quaternion = object
    if ref not in sys.path:
        sys.path.insert(0, ref)
    sys.dont_write_bytecode = True


def write_golden(ref):
    """Build the reference modules on the shims and store what the test compares against."""
    _install_reference_side(ref)
    from unidistill.layers.blocks_3d.mmdet3d import lss_fpn
    from unidistill.layers.blocks_3d.det3d.spconv_backbone import VoxelResBackBone8x
    from unidistill.data.det3d.preprocess.voxelization import Voxelization
    from unidistill_amd import config as C
    bb = VoxelResBackBone8x(5, np.array(C.GRID_SIZE))
    vox = Voxelization(C.VOXEL_SIZE, C.POINT_CLOUD_RANGE, 10, (120000, 160000), 5, torch.device("cpu"))
    lss = lss_fpn.LSSFPN(**C.CAMERA_ENCODER)
    bb_keys, bb_shapes = _shapes(bb)
    lss_keys, lss_shapes = _shapes(lss)
    path = os.path.join(HERE, "golden", "shims_reference.npz")
    np.savez_compressed(path, voxel_pooling_module=np.array(lss_fpn.voxel_pooling_ext.__name__),
                        backbone_conv_input_cls=np.array(_qualname(type(bb.conv_input[0]))),
                        backbone_conv2_cls=np.array(_qualname(type(bb.conv2[0][0]))),
                        voxel_generator_cls=np.array(_qualname(type(vox.voxel_generator))),
                        backbone_keys=bb_keys, backbone_shapes=bb_shapes, lss_keys=lss_keys, lss_shapes=lss_shapes,
                        frustum=lss.frustum.numpy(), voxel_coord=lss.voxel_coord.numpy())
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


def test_reference_modules_build_on_the_shims(golden):
    g = golden("shims_reference")
    saved = dict(sys.modules)
    try:
        from unidistill_amd import shims
        shims.install()
        from unidistill_amd.ops import spconv as sp, bev_pool, voxelize
        from unidistill_amd import config as C
        # the extension module the reference's lss_fpn imports resolves to this library's bev_pool
        assert sys.modules[str(g["voxel_pooling_module"])].voxel_pooling_forward_wrapper is \
            bev_pool.voxel_pooling_forward_wrapper
        # the reference's backbone and voxelizer were built from this library's classes
        assert _resolve(g["backbone_conv_input_cls"]) is sp.SubMConv3d
        assert _resolve(g["backbone_conv2_cls"]) is sp.SparseConv3d
        assert _resolve(g["voxel_generator_cls"]) is voxelize.PointToVoxel
        assert sys.modules["spconv.pytorch"].SubMConv3d is sp.SubMConv3d
        assert sys.modules["spconv.pytorch"].SparseConv3d is sp.SparseConv3d
        assert sys.modules["spconv.pytorch.utils"].PointToVoxel is voxelize.PointToVoxel
        from unidistill_amd.layers.lidar import VoxelResBackBone8x as Mine
        keys, shapes = _shapes(Mine(5, C.GRID_SIZE))
        assert keys.tolist() == g["backbone_keys"].tolist() and shapes.tolist() == g["backbone_shapes"].tolist()
        from unidistill_amd.layers.lss_fpn import LSSFPN as MineLSS
        ours = MineLSS(**C.CAMERA_ENCODER)
        keys, shapes = _shapes(ours)
        assert keys.tolist() == g["lss_keys"].tolist() and shapes.tolist() == g["lss_shapes"].tolist()
        torch.testing.assert_close(ours.frustum, torch.from_numpy(g["frustum"]), rtol=0, atol=0)
        torch.testing.assert_close(ours.voxel_coord, torch.from_numpy(g["voxel_coord"]), rtol=0, atol=0)
    finally:          # drop the stand-in packages again (spconv, mmcv, ...); this library's own modules stay loaded
        for name in set(sys.modules) - set(saved):
            if not name.startswith("unidistill_amd"):
                del sys.modules[name]


if __name__ == "__main__":
    ROOT = os.path.dirname(HERE)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
    os.environ.setdefault("UD_RANDOM_INIT", "1")
    write_golden(os.environ["UNIDISTILL_REF"])
