"""What the device units' Python wrappers (``proc2d``, ``proc3d``, ``metrics``) ask of their operands, judged in one
place: is it a tensor, a batch of pictures, a cloud ``[n, 3]``, a vector of ids, a stack of class volumes.  Host code
only; ``torch`` is imported when a tensor arrives and not before.

Every helper returns a plain record (``SimpleNamespace``) that holds what the foreign call needs -- the address, whether
it is device memory, the device, torch's current stream there -- and the converted array itself, which has to stay
referenced until the call has returned.  A helper reports the stream; the wrapper decides whether to pass it or to wait."""
from types import SimpleNamespace

import numpy as np

from . import _native as nat


def is_tensor(a):
    """A torch tensor (anything but an ndarray that carries ``data_ptr``)."""
    return not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")


def ptr_of(a):
    """Address of a tensor's or of a C-contiguous array's data."""
    return a.data_ptr() if is_tensor(a) else nat.addr(a)


def empty_uint8(shape, tdevice=None):
    """An uint8 output: a CUDA tensor on the torch device ``tdevice``, or without one a NumPy array."""
    if tdevice is None:
        return np.empty(shape, dtype=np.uint8)
    import torch
    return torch.empty(shape, dtype=torch.uint8, device=tdevice)


def tensor_place(t):
    """``(device index, torch's current stream there)`` of a CUDA tensor."""
    import torch
    return t.device.index, torch.cuda.current_stream(t.device.index).cuda_stream


def picture_batch(images, device=0):
    """uint8 RGB pictures ``[V, H, W, 3]`` or one picture ``[H, W, 3]``, a NumPy array or a contiguous CUDA tensor:
    ``vhw`` (``V`` is 1 for one picture), ``shape`` (the input's), ``data``, ``ptr``, ``on_device``, ``device``,
    ``stream`` and ``tdevice``, with which ``empty_uint8`` makes an output of the input's kind (on the input's device).
    An empty batch (a 0 in ``shape``) is not refused here: the wrapper does that in its own turn."""
    on_device = is_tensor(images)
    if on_device:
        import torch
        if images.dtype != torch.uint8 or not images.is_cuda or not images.is_contiguous():
            raise ValueError("a tensor of pictures must be a contiguous CUDA uint8 tensor")
    else:
        images = np.asarray(images)
        if images.dtype != np.uint8:
            raise ValueError("pictures must be uint8 (float pictures take the reference's CPU route)")
    shape = tuple(images.shape)
    if len(shape) not in (3, 4) or shape[-1] != 3:
        raise ValueError("pictures must be [V, H, W, 3] or [H, W, 3] (RGB; RGBA and grey pictures take the reference's CPU route)")
    if on_device:
        (dev, stream), ptr, tdev = tensor_place(images), images.data_ptr(), images.device
    else:
        images = np.ascontiguousarray(images)
        dev, stream, ptr, tdev = int(device), 0, nat.addr(images), None
    return SimpleNamespace(vhw=(1,) + shape[:2] if len(shape) == 3 else shape[:3], shape=shape, data=images, ptr=ptr,
                           on_device=int(on_device), device=dev, stream=stream, tdevice=tdev)


def points(cloud, what, dims="[n, 3]"):
    """A cloud as the point units take it -- array-like ``[n, 3]``, anything with ``.points``, or a contiguous float64
    CUDA tensor ``[n, 3]`` used in place: ``points`` (the tensor, or a C-contiguous float64 array, ``[0, 3]`` for any
    empty input), ``n``, ``on_device`` and ``ptr``, which for an empty array is the address of a ``[1, 3]`` zero array
    (``keep``, held by the record): the library is given a valid address whatever ``n`` is.  ``what`` and ``dims`` word the refusals."""
    if not isinstance(cloud, np.ndarray) and hasattr(cloud, "points"):
        cloud = cloud.points
    if is_tensor(cloud):
        import torch
        if (cloud.dtype != torch.float64 or not cloud.is_cuda or not cloud.is_contiguous() or cloud.dim() != 2
                or cloud.shape[1] != 3):
            raise ValueError(f"device {what} must be a contiguous float64 CUDA tensor {dims}")
        return SimpleNamespace(points=cloud, n=int(cloud.shape[0]), on_device=1, ptr=cloud.data_ptr())
    pts = np.ascontiguousarray(np.asarray(cloud, dtype=np.float64))
    if pts.ndim != 2 or pts.shape[1] != 3:
        if pts.size:
            raise ValueError(f"{what} must be {dims}")
        pts = pts.reshape(0, 3)
    keep = pts if pts.shape[0] else np.zeros((1, 3))
    return SimpleNamespace(points=pts, n=pts.shape[0], on_device=0, ptr=nat.addr(keep), keep=keep)


def ids(a, what):
    """A vector of int32 ids ``[n]``, array-like (converted) or a contiguous int32 CUDA tensor: ``data``, ``n``,
    ``on_device``, ``tdevice`` (``None`` for an array) and ``ptr``, 0 when empty."""
    if is_tensor(a):
        import torch
        if a.dtype != torch.int32 or not a.is_cuda or not a.is_contiguous() or a.dim() != 1:
            raise ValueError(f"device {what} must be a contiguous int32 CUDA tensor [n]")
        return SimpleNamespace(data=a, n=len(a), on_device=1, tdevice=a.device, ptr=a.data_ptr() if a.numel() else 0)
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))
    return SimpleNamespace(data=arr, n=len(arr), on_device=0, tdevice=None, ptr=nat.addr(arr) if arr.size else 0)


def graph_rows(rows, n=None, extra=None):
    """The rows of arcs the graph unit reads -- ``(index [N, k], d2 [N, k])`` as ``knn_points`` returns them or
    ``(offsets [N + 1], index [E], d2 [E])`` as ``radius_points`` does -- and the optional extra pairs ``(edges [M, 2],
    weights [M])``: all array-likes (converted to int64 offsets, int32 indices, float64 values) or all contiguous CUDA
    tensors of those dtypes on one device, used in place.  ``n``, when given, must be the rows' node count.

    Returns ``n``, ``E``, ``M``, ``row_len`` (0 for the CSR form), the addresses ``offsets`` (0 for the fixed form),
    ``index``, ``values``, ``extra``, ``extra_w`` (0 where empty), ``arcs`` (the index array or tensor), ``on_device``,
    ``tdevice`` (``None`` for arrays) and ``keep``, what the addresses point into."""
    rows = tuple(rows)
    if len(rows) not in (2, 3):
        raise ValueError("rows must be (index, d2) or (offsets, index, d2)")
    parts = list(rows) + (list(extra) if extra is not None else [])
    if extra is not None and len(parts) != len(rows) + 2:
        raise ValueError("extra must be (edges [M, 2], weights [M])")
    kinds = [is_tensor(a) for a in parts]
    if any(kinds) and not all(kinds):
        raise ValueError("rows and extra must be all arrays or all CUDA tensors")
    on_device = int(all(kinds))
    tdev = None
    if on_device:
        import torch
        want = [torch.int64] * (len(rows) - 2) + [torch.int32, torch.float64] + [torch.int32, torch.float64] * (extra is not None)
        for a, dt in zip(parts, want):
            if a.dtype != dt or not a.is_cuda or not a.is_contiguous():
                raise ValueError("device rows must be contiguous CUDA tensors: int64 offsets, int32 indices, float64 values")
        tdev = same([a.device for a in parts], "devices")
    else:
        want = [np.int64] * (len(rows) - 2) + [np.int32, np.float64] + [np.int32, np.float64] * (extra is not None)
        parts = [np.ascontiguousarray(np.asarray(a, dtype=dt)) for a, dt in zip(parts, want)]
    offsets = parts[0] if len(rows) == 3 else None
    index, values = parts[len(rows) - 2], parts[len(rows) - 1]
    if tuple(index.shape) != tuple(values.shape):
        raise ValueError("index and d2 must have one shape")
    if offsets is None:
        if len(index.shape) != 2 or index.shape[1] < 1:
            raise ValueError("rows of fixed length must be [N, k] with k at least 1")
        nodes, row_len = int(index.shape[0]), int(index.shape[1])
    else:
        if len(offsets.shape) != 1 or offsets.shape[0] < 1 or len(index.shape) != 1:
            raise ValueError("CSR rows must be offsets [N + 1], index [E], d2 [E]")
        nodes, row_len = int(offsets.shape[0]) - 1, 0
    if n is not None and int(n) != nodes:
        raise ValueError(f"n is {int(n)}, the rows hold {nodes} nodes")
    E = int(np.prod(index.shape))
    M = 0
    if extra is not None:
        edges, weights = parts[-2], parts[-1]
        M = int(weights.shape[0]) if len(weights.shape) == 1 else -1
        if M and (M < 0 or tuple(edges.shape) != (M, 2)):
            raise ValueError("extra must be (edges [M, 2], weights [M])")

    def at(a, count):
        return ptr_of(a) if count else 0

    return SimpleNamespace(n=nodes, E=E, M=M, row_len=row_len, offsets=0 if offsets is None else ptr_of(offsets), index=at(index, E),
                           values=at(values, E), extra=at(parts[-2], M) if M else 0, extra_w=at(parts[-1], M) if M else 0,
                           arcs=index, offsets_data=offsets, extra_data=parts[-2] if M else None, on_device=on_device,
                           tdevice=tdev, keep=parts)


def node_ids(g, a, what):
    """One int32 id per node of ``g`` (a ``graph_rows`` record), of the rows' kind and on their device: the ``ids`` record
    of ``a``.  ``what`` ("key", "labels") words the refusals."""
    if is_tensor(a) != bool(g.on_device):
        raise ValueError(f"rows and {what} must be all arrays or all CUDA tensors")
    k = ids(a, what)
    if k.n != g.n:
        raise ValueError(f"one {what.rstrip('s')} per node")
    if k.on_device and k.tdevice != g.tdevice:
        raise ValueError(f"rows and {what} must be on one device")
    return k


def same(things, what):
    """The one value all ``things`` share, or the refusal that lists the values they take."""
    if any(t != things[0] for t in things):
        raise ValueError(f"the {what} differ: {sorted(set(str(t) for t in things))}")
    return things[0]


_EVAL_CODES = {np.dtype(np.float32): nat.SC_EVAL_F32, np.dtype(np.float64): nat.SC_EVAL_F64, np.dtype(np.uint8): nat.SC_EVAL_U8,
               np.dtype(np.bool_): nat.SC_EVAL_U8}  # (bool is read as uint8)
_TORCH_CODES = {}  # the same for torch's dtypes, filled when the first tensor arrives


def class_stack(vols, noun, accept, refused, device=0):
    """A list of class volumes of one shape ``(nx, ny, nz)`` and dtype: all NumPy arrays, or all contiguous CUDA tensors
    of one device.  ``noun`` ("voxels", "ground truths") names them in the refusals.  ``accept``: the ``SC_EVAL_*``
    forms the library reads here; float32, float64 and uint8 volumes of an accepted form are read as they are, bool as
    uint8; an array of any other dtype is converted to float64, a tensor of any other dtype refused with the message
    ``refused``.

    Returns ``vols`` (the arrays or tensors the table points into), ``table`` (their addresses, ``uintp``), ``shape``,
    ``code`` (``SC_EVAL_*``), ``on_device``, ``tdevice`` (``None`` for arrays), ``device`` and ``stream``."""
    tensors = [is_tensor(v) for v in vols]
    if any(tensors) and not all(tensors):
        raise ValueError("volumes must be all NumPy arrays or all CUDA tensors")
    if all(tensors):
        if not _TORCH_CODES:
            import torch
            _TORCH_CODES.update({getattr(torch, d.name): code for d, code in _EVAL_CODES.items()})
        for t in vols:
            if not t.is_cuda or not t.is_contiguous() or t.dim() != 3:
                raise ValueError("device volumes must be contiguous 3-D CUDA tensors")
        tdev = same([t.device for t in vols], "devices")
        shape = same([tuple(t.shape) for t in vols], f"shapes of the {noun}")
        code = _TORCH_CODES.get(same([t.dtype for t in vols], f"dtypes of the {noun}"))
        if code not in accept:
            raise ValueError(refused)
        (dev, stream), on_device, ptrs = tensor_place(vols[0]), 1, [t.data_ptr() for t in vols]
    else:
        vols = [np.asarray(v) for v in vols]
        shape = same([v.shape for v in vols], f"shapes of the {noun}")
        dt = same([v.dtype for v in vols], f"dtypes of the {noun}")
        if len(shape) != 3:
            raise ValueError("volumes must be 3-D")
        code = _EVAL_CODES.get(dt)
        if code not in accept:
            vols, code = [v.astype(np.float64) for v in vols], nat.SC_EVAL_F64
        elif dt == np.bool_:
            vols = [v.view(np.uint8) for v in vols]
        vols = [np.ascontiguousarray(v) for v in vols]
        tdev, dev, stream, on_device, ptrs = None, int(device), 0, 0, [nat.addr(v) for v in vols]
    return SimpleNamespace(vols=vols, table=np.array(ptrs, dtype=np.uintp), shape=shape, code=code, on_device=on_device,
                           tdevice=tdev, device=dev, stream=stream)
