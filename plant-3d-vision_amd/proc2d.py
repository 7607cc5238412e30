"""The geometric pipeline's picture stages on the device: the lens correction (``undistort``, below the masks) and
the mask producer, RGB pictures -> dilated binary masks.

Mirror of what ``Masks.f`` does to one picture (``plant3dvision/tasks/proc2d.py:224-249`` over
``plant3dvision/proc2d.py:69-220``) -- float64 copy, ``rescale_intensity(out_range=(0, 1))``, the ``linear`` or
``excess_green`` filter, ``> threshold``, ``binary_dilation`` with ``disk(n, decomposition='sequence')``,
``255 * mask`` as uint8 -- for a batch of pictures in one call of ``sc_masks_from_rgb`` (``csrc/masks_rgb.hip``).
The masks of a CUDA tensor stay in HBM, which is what ``masks2d.voxels_from_masks`` takes: no PNG, no host copy.

PARITY UNPINNED: skimage is not available here, so the range step restates
``skimage.exposure.rescale_intensity`` from its source; the dilation series is ``masks2d.disk_series``'s.
There is no CPU path: pictures that are not uint8 RGB are refused and the caller keeps the reference's route.
"""
import numpy as np

from . import _native as nat
from . import _operands as ops
from .masks2d import disk_series

#: filter names of ``Masks.type`` (tasks/proc2d.py:217-222) -> SC_FILTER_*
FILTERS = {"linear": nat.SC_FILTER_LINEAR, "excess_green": nat.SC_FILTER_EXCESS_GREEN}


def dilation_steps(n):
    """The 3x3 steps ``proc2d.dilation(img, n)`` amounts to, as SC_FOOT_* ids in the order they are applied:
    ``masks2d.disk_series(n)`` with its repetitions written out (at most 32 steps)."""
    steps = [nat.SC_FOOT[name] for name, reps in disk_series(n) for _ in range(reps)]
    return np.array(steps, dtype=np.uint8)


def masks_from_images(images, type="linear", parameters=(0, 1, 0), threshold=0.3, dilation=0, device=0):
    """``Masks`` on a batch of pictures.

    images : NumPy ``uint8 [V, H, W, 3]`` (or one picture ``[H, W, 3]``) -> NumPy ``uint8 [V, H, W]``
        (``[H, W]``); or a contiguous CUDA torch ``uint8`` tensor of that shape -> a CUDA torch tensor on the same
        device, produced on torch's current stream without a host wait.
    type, parameters, threshold, dilation : the task's parameters (tasks/proc2d.py:208-211); ``parameters`` are the
        ``linear`` coefficients.  Every picture is rescaled by its own range.
    """
    if type not in FILTERS:
        raise Exception(f"Unknown masking type '{type}'!")  # tasks/proc2d.py:222
    coefs = np.ascontiguousarray(np.asarray(list(parameters), dtype=np.float64).reshape(-1))
    if coefs.size != 3:
        raise ValueError("parameters must be the three linear coefficients")
    dilation = int(dilation)
    steps = dilation_steps(dilation) if dilation > 0 else np.zeros(0, dtype=np.uint8)
    nat.backend()
    p = ops.picture_batch(images, device)
    out = ops.empty_uint8(p.shape[:-1], p.tdevice)
    if 0 in p.shape:  # (an empty batch is refused once its output exists)
        raise ValueError("V, H and W must be at least 1")
    nat.unit_call("sc_masks_from_rgb", p.ptr, p.on_device, *p.vhw, FILTERS[type], nat.addr(coefs), float(threshold),
                  nat.addr(steps) if steps.size else 0, int(steps.size), p.device, p.stream, ops.ptr_of(out), p.on_device, 0)
    return out


def _camera_numbers(camera_mtx, distortion_vect):
    """``(K = fx fy cx cy, dist = k1 k2 p1 p2 k3)`` as float64 arrays, widened as cv2 widens its arguments."""
    mtx = np.asarray(camera_mtx, dtype=np.float64)
    if mtx.shape != (3, 3):
        raise ValueError("camera_mtx must be 3 x 3")
    if mtx[0, 1] != 0 or mtx[1, 0] != 0 or mtx[2].tolist() != [0, 0, 1]:
        raise ValueError("camera_mtx with a skew or a last row other than [0, 0, 1] takes the reference's CPU route")
    d = np.asarray(distortion_vect, dtype=np.float64).reshape(-1)
    if d.size < 4:
        raise ValueError("distortion_vect must hold k1, k2, p1, p2 and optionally k3")
    if np.any(d[5:] != 0):  # (a NaN there is refused as well)
        raise ValueError("distortion models beyond k1, k2, p1, p2, k3 take the reference's CPU route")
    dist = np.zeros(5, dtype=np.float64)
    dist[:min(5, d.size)] = d[:5]
    return np.array([mtx[0, 0], mtx[1, 1], mtx[0, 2], mtx[1, 2]], dtype=np.float64), dist


def undistort(img, camera_mtx, distortion_vect, device=0):
    """``plant3dvision.proc2d.undistort`` (:25-66), which is ``cv2.undistort(img, camera_mtx, distortion_vect, None)``,
    for one picture or a batch of pictures of one camera, in one call of ``sc_undistort_rgb`` (``csrc/undistort.hip``).

    img : NumPy ``uint8 [H, W, 3]`` or ``[V, H, W, 3]`` -> NumPy of the same shape; or a contiguous CUDA torch
        ``uint8`` tensor of that shape -> a CUDA torch tensor on the same device, produced on torch's current stream
        without a host wait (``masks_from_images`` takes it from there).
    camera_mtx : 3 x 3 of any dtype, widened to float64 as cv2 does -- the reference passes float32 arrays
        (``camera.camera_arrays_from_params``), so the values are the float32-rounded ones.  A skew or a last row other
        than ``[0, 0, 1]`` raises ``ValueError``: the caller keeps the reference's route.
    distortion_vect : ``k1, k2, p1, p2[, k3]``; longer vectors only if the further entries are zero.

    PARITY UNPINNED: OpenCV is not available here, so the kernels restate its published algorithm
    (``initUndistortRectifyMap``, ``CV_16SC2`` maps with 5 fraction bits, ``remap`` with ``INTER_LINEAR`` and a
    constant 0 border) with two documented deviations: the ray of a pixel is evaluated directly, and source positions
    beyond +-32768 lie outside.  There is no CPU path.
    """
    K, dist = _camera_numbers(camera_mtx, distortion_vect)
    nat.backend()
    p = ops.picture_batch(img, device)
    if 0 in p.shape:
        raise ValueError("V, H and W must be at least 1")
    out = ops.empty_uint8(p.shape, p.tdevice)
    nat.unit_call("sc_undistort_rgb", p.ptr, p.on_device, *p.vhw, nat.addr(K), nat.addr(dist), p.device, p.stream,
                  ops.ptr_of(out), p.on_device, 0)
    return out
