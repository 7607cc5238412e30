"""GPU, two devices: an entry point of a stand-alone unit that works on another device than the caller's current one
puts the caller's device back before it returns (``CallerDevice`` / ``UnitCall`` of csrc/sc_unit.h)."""
import ctypes

import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import metrics, proc2d, proc3d

_RNG = np.random.default_rng(5)
_POINTS = _RNG.random((65, 3))
_VOLS = {"a": _RNG.random((3, 5, 6)).astype(np.float32), "b": _RNG.random((3, 5, 6)).astype(np.float32)}
_BALL = (((np.indices((12, 12, 12)) - 5.5) ** 2).sum(axis=0) < 16.0).astype(np.uint8)
_PICS = _RNG.integers(0, 2, (2, 9, 70), dtype=np.uint8)
_CAMERA = {"camera_model": {"params": [10.0, 10.0, 4.0, 4.0]}, "rotmat": np.eye(3), "tvec": [0.0, 0.0, 5.0]}

# one tiny call per unit (evaluate and nearest: per entry point), every input in host memory
CALLS = {
    "vol2pcd": lambda d: proc3d.vol2pcd(_BALL, (0, 0, 0), 1.0, device=d, as_open3d=False),
    "label_points": lambda d: proc3d.label_points(_POINTS, [_CAMERA], np.full((2, 1, 8, 8), 3, dtype=np.uint8), device=d),
    "masks_rgb": lambda d: proc2d.masks_from_images(_RNG.integers(0, 256, (2, 9, 70, 3), dtype=np.uint8), dilation=2, device=d),
    "dbscan": lambda d: proc3d.cluster_dbscan(_POINTS, 0.2, 3, device=d),
    "evaluate_voxels": lambda d: metrics.voxel_confusion(_VOLS, _VOLS, background=None, device=d),
    "evaluate_masks": lambda d: metrics.compare_mask_stacks(_PICS, _PICS[::-1].copy(), 2, device=d),
    "class_select": lambda d: proc3d.select_classes(_VOLS, background=None, device=d),
    "nearest": lambda d: proc3d.nearest_points(_POINTS, _POINTS[::2].copy(), device=d),
    "nearest_confusion": lambda d: proc3d.nearest_confusion(np.zeros(65, dtype=np.int32), np.zeros(65, dtype=np.int32),
                                                           np.zeros(33, dtype=np.int32), 2, device=d),
}


@pytest.mark.gpu
def test_every_unit_puts_the_callers_device_back(gpu_device):
    if nat.device_count() < 2:
        pytest.skip("needs two visible devices")
    hip = nat.hip_runtime()
    current = ctypes.c_int(-1)
    try:
        for name, call in CALLS.items():
            assert hip.hipSetDevice(0) == 0
            call(1)
            assert hip.hipGetDevice(ctypes.byref(current)) == 0
            assert current.value == 0, name
    finally:
        hip.hipSetDevice(0)
