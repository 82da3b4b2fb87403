"""CPU: the input chain's module layout -- every layer imports on its own in a fresh interpreter (a lower layer first is
the order that exposes an import cycle), and ops/input_prep.py still hands out every public name it used to define."""
import importlib
import os
import subprocess
import sys

from conftest import PKG

LAYERS = ("staging", "lidar_prep", "gt_paste", "image_affine", "jpeg", "collate", "input_prep")

# dir(input_prep) before the split (the names without a leading underscore that are not imported modules), by the module
# that holds each now
PUBLIC = {
    "config": ("IMG_DIM",),
    "ops.staging": ("input_stream",),
    "ops.lidar_prep": ("BevAffineTransformation", "CollectLidarSweeps", "ObjectRangeFilter", "bda_boxes", "bev_affine",
                       "bev_transform_matrix", "boxes_in_range_mask", "collect_lidar_sweeps", "points_range_filter",
                       "points_transform", "sweep_time_lag", "sweep_to_key_matrix"),
    "ops.gt_paste": ("GTSampling", "ObjectDatabase", "append_pasted", "gt_paste", "lidar_paste_host_clouds"),
    "ops.image_affine": ("IMG_MEAN", "IMG_STD", "ImageAffineTransformation", "TO_RGB", "ida_matrix", "image_affine",
                         "image_affine_host_frames", "image_normalize", "plan_frames", "resample_table",
                         "rotate_constants"),
    "ops.jpeg": ("JpegFrameError", "jpeg_decode"),
    "ops.collate": ("collate_fn", "lidar_prep_host_clouds"),
}


def test_every_layer_imports_first_in_a_fresh_process():
    env = dict(os.environ, PYTHONPATH=PKG)
    procs = [(name, subprocess.Popen([sys.executable, "-s", "-c", f"import unidistill_amd.ops.{name}"], env=env,
                                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for name in LAYERS]
    for name, p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, f"import unidistill_amd.ops.{name}:\n{out}"


def test_facade_hands_out_every_public_name_from_its_home_module():
    assert sum(len(names) for names in PUBLIC.values()) == 34
    facade = importlib.import_module("unidistill_amd.ops.input_prep")
    for home, names in PUBLIC.items():
        module = importlib.import_module("unidistill_amd." + home)
        for name in names:
            obj = getattr(module, name)
            assert getattr(facade, name) is obj, name
            assert getattr(obj, "__module__", module.__name__) == module.__name__, name      # defined there, not passed on
