"""The input chain's public names in one place.  The code lives in layers, each importing only from the
ones before it: staging -> lidar_prep -> gt_paste -> image_affine -> jpeg -> collate."""
from ..config import IMG_DIM                                                                        # noqa: F401
from .collate import collate_fn, lidar_prep_host_clouds                                             # noqa: F401
from .gt_paste import (GTSampling, ObjectDatabase, ObjectDatabaseBuilder, append_pasted, gt_paste,  # noqa: F401
                       lidar_paste_host_clouds, points_in_boxes)
from .image_affine import (IMG_MEAN, IMG_STD, TO_RGB, ImageAffineTransformation, ida_matrix,        # noqa: F401
                           image_affine, image_affine_host_frames, image_normalize, plan_frames, resample_table,
                           rotate_constants)
from .jpeg import JpegFrameError, jpeg_decode                                                       # noqa: F401
from .lidar_prep import (BevAffineTransformation, CollectLidarSweeps, ObjectRangeFilter, bda_boxes,  # noqa: F401
                         bev_affine, bev_transform_matrix, boxes_in_range_mask, collect_lidar_sweeps,
                         points_range_filter, points_transform, sweep_time_lag, sweep_to_key_matrix)
from .staging import input_stream                                                                   # noqa: F401
