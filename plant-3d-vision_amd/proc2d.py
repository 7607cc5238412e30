"""The geometric pipeline's mask producer on the device: RGB pictures -> dilated binary masks.

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
    b = nat.backend()
    is_tensor = not isinstance(images, np.ndarray) and hasattr(images, "data_ptr")
    if is_tensor:
        import torch
        if images.dtype != torch.uint8 or not images.is_cuda or not images.is_contiguous():
            raise ValueError("a tensor of pictures must be a contiguous CUDA uint8 tensor")
        shape = tuple(int(s) for s in images.shape)
    else:
        images = np.asarray(images)
        if images.dtype != np.uint8:
            raise ValueError("pictures must be uint8 (float pictures take the reference's CPU route)")
        shape = images.shape
    single = len(shape) == 3
    if len(shape) not in (3, 4) or shape[-1] != 3:
        raise ValueError("pictures must be [V, H, W, 3] or [H, W, 3] (RGB; RGBA and grey pictures take the reference's CPU route)")
    V, H, W = (1,) + tuple(shape[:2]) if single else tuple(shape[:3])
    args = (int(V), int(H), int(W), FILTERS[type], nat.addr(coefs), float(threshold),
            nat.addr(steps) if steps.size else 0, int(steps.size))
    if is_tensor:
        import torch
        dev = images.device.index
        out = torch.empty((H, W) if single else (V, H, W), dtype=torch.uint8, device=images.device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        if images.numel() == 0:
            raise ValueError("V, H and W must be at least 1")
        nat.check(b.call("sc_masks_from_rgb", images.data_ptr(), 1, *args, int(dev), int(stream), out.data_ptr(), 1, 0),
                  "sc_masks_from_rgb", "sc_masks_last_error")
        return out
    images = np.ascontiguousarray(images)
    out = np.empty((H, W) if single else (V, H, W), dtype=np.uint8)
    if images.size == 0:
        raise ValueError("V, H and W must be at least 1")
    nat.check(b.call("sc_masks_from_rgb", nat.addr(images), 0, *args, int(device), 0, nat.addr(out), 0, 0),
              "sc_masks_from_rgb", "sc_masks_last_error")
    return out
