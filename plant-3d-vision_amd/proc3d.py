"""Voxel <-> world convention of the reference (``plant3dvision/proc3d.py:28-65``), pinned
by its ``tests/unit/test_proc3d.py:12-30``: voxel centres sit at ``origin + index *
voxel_size`` -- the same rule the kernels use (``kernels/backprojection.c:71-73``)."""
import math

import numpy as np


def index2point(indexes, origin, voxel_size):
    """Nxd indices -> Nxd points (proc3d.py:28-45)."""
    return voxel_size * np.asarray(indexes) + np.asarray(origin)[np.newaxis, :]


def point2index(points, origin, voxel_size):
    """Nxd points -> Nxd integer indices, rounded to nearest (proc3d.py:48-65)."""
    return np.array(np.round((np.asarray(points) - np.asarray(origin)[np.newaxis, :]) / voxel_size),
                    dtype=int)


class PointCloud:
    """What ``vol2pcd`` returns where open3d is absent: ``points`` and ``normals`` as float64
    ``[n, 3]`` arrays (the two attributes the reference's callers read from the open3d object); ``colors`` is
    ``None`` or a float64 ``[n, 3]`` array (what ``tasks/proc3d.py::point_cloud_run`` sets, tasks/proc3d.py:118-124)."""

    def __init__(self, points, normals, colors=None):
        self.points = points
        self.normals = normals
        self.colors = colors

    def __len__(self):
        return len(self.points)


def gaussian_weights(sigma=1.0, truncate=4.0):
    """The weights ``scipy.ndimage.gaussian_filter`` uses (``_gaussian_kernel1d``): radius
    ``int(truncate*sigma + 0.5)``, ``exp(-0.5/sigma^2 * x^2)`` normalised by its sum.  Returns
    the distinct half, centre first."""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:], dtype=np.float64)


#: what ``release_device_buffers`` calls, in this order
RELEASES = ("sc_vol2pcd_release", "sc_dbscan_release", "sc_eval_release", "sc_select_release", "sc_nearest_release")


def release_device_buffers():
    """Give back the device work buffers ``vol2pcd`` keeps between calls (``sc_vol2pcd_release``; it keeps them
    only while they are at most 1 GiB), those of ``cluster_dbscan`` (``sc_dbscan_release``), those of the
    evaluation counts of ``metrics`` (``sc_eval_release``), those of ``select_classes`` (``sc_select_release``) and
    those of ``nearest_points`` and the cloud metrics (``sc_nearest_release``).  ``Backprojection.close`` calls this."""
    from . import _native as nat
    for entry in RELEASES:
        nat.backend().call(entry)


def release_graph_buffers():
    """Give back the device work buffers ``graph_distances``, ``graph_components`` and ``graph_quotient`` keep between calls
    (``sc_graph_release``; they are kept only while they are at most 1 GiB).  It stands beside
    ``release_device_buffers``, whose five entries in ``RELEASES`` stay what they are: call both to give everything back."""
    from . import _native as nat
    nat.backend().call("sc_graph_release")


def set_scratch_limit(nbytes):
    """Largest device work buffers a ``vol2pcd`` call may take (default 8 GiB; 0 = no limit): a volume that needs
    more -- 49 bytes per voxel -- goes through in x-slabs with a halo, same points in the same order."""
    from . import _native as nat
    nat.backend().call("sc_vol2pcd_set_scratch_limit", int(nbytes))


def _make_cloud(points, normals, colors=None, as_open3d=True):
    """An ``open3d.geometry.PointCloud`` when open3d is importable (and ``as_open3d``), else a :class:`PointCloud`."""
    if as_open3d:
        try:
            import open3d as o3d  # type: ignore
        except ImportError:
            o3d = None
        if o3d is not None:
            pcd = o3d.geometry.PointCloud()
            pcd.points = o3d.utility.Vector3dVector(points)
            pcd.normals = o3d.utility.Vector3dVector(normals)
            if colors is not None:
                pcd.colors = o3d.utility.Vector3dVector(colors)
            return pcd
    return PointCloud(points, normals, colors)


def _adopt_cloud(b, out, cnt, as_open3d):
    """The tail ``vol2pcd`` and ``vol2pcd_class`` share: the library's two buffers (``out``: their addresses, ``cnt``:
    the point count) become the arrays, points without a normal are dropped, the cloud object is made."""
    import ctypes

    n = int(cnt[0])
    if n:
        # the library's buffers become the arrays (no copy); they are released with the last view
        import weakref

        def adopt(address):
            owner = (ctypes.c_double * (3 * n)).from_address(address)
            weakref.finalize(owner, b.call, "sc_free_host", address)
            return np.frombuffer(owner, dtype=np.float64).reshape(n, 3)

        pts, nrm = adopt(int(out[0])), adopt(int(out[1]))
    else:
        pts = np.zeros((0, 3))
        nrm = np.zeros((0, 3))
    ok = ~np.isnan(nrm).any(axis=1)  # proc3d.py:559-561: keep points with a positive gradient norm
    if not ok.all():
        pts, nrm = pts[ok], nrm[ok]
    return _make_cloud(pts, nrm, None, as_open3d)


def vol2pcd(volume, origin, voxel_size, level_set_value=0, device=0, as_open3d=True):
    """Converts a volume into a point-cloud with normals, on the GPU
    (``plant3dvision/proc3d.py:490-570``; same signature, ``device`` / ``as_open3d`` added).

    ``volume`` may be a NumPy array (int32 / float32 / float64 / uint8, C-order), a
    ``Backprojection`` whose device-resident volume is used in place -- the 4N-byte grid then
    never crosses PCIe, only the shell's points and normals come back -- or the ``PackedGrid`` of a
    sharded run (``ShardedBackprojection.all_gather(compress="1bit" | "2bit", unpack=False)``): the
    ranks' packed planes are read as they are and the full-size grid is never written; or its ``SparseGrid``
    (``compress="sparse"``): the uint8 occupancy ``label == 1`` is written on the device from the codes and the mixed
    bricks (1 byte per voxel) and read in place.
    Returns an ``open3d.geometry.PointCloud`` when open3d is importable (and ``as_open3d``),
    else a :class:`PointCloud` with the same ``points`` / ``normals``.

    Deviation: a volume of one class -- nothing above 0.5, or nothing at or below it -- yields an empty
    cloud at every ``level_set_value``; the reference returns up to 5 points at corner (0, 0, 0) there, an artefact of
    SciPy's distance transform on an input without a site.
    """
    from . import _native as nat

    nat.backend()
    codes = {np.dtype(np.int32): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2, np.dtype(np.uint8): 3}
    origin64 = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))  # judged before the volume
    tail = (origin64, voxel_size, level_set_value, as_open3d)
    if hasattr(volume, "occupancy_device"):  # a sharded run's SparseGrid: its occupancy (label == 1) on the device
        sg = volume
        ptr, keep = sg.occupancy_device()
        return _vol2pcd_call("sc_vol2pcd", (ptr, 1, codes[np.dtype(np.uint8)]), sg.shape, sg.device, *tail)
    if hasattr(volume, "recv") and hasattr(volume, "rank_bytes"):  # a sharded run's PackedGrid: read as it is
        import torch
        pg = volume
        torch.cuda.synchronize(pg.recv.device)  # the collective that filled it
        head = (int(pg.recv.data_ptr()), int(pg.rank_bytes), int(pg.world), 0 if pg.partition == "cyclic" else 1, int(pg.bits))
        return _vol2pcd_call("sc_vol2pcd_packed", head, pg.shape, pg.device, *tail, what="sc_vol2pcd")
    if hasattr(volume, "_engine") and hasattr(volume, "shape"):  # a Backprojection: use its state in place
        bp = volume
        ptr = bp._engine.values_device_ptr()
        bp._engine.synchronize()
        shape = [int(s) for s in bp.shape]
        code, on_device, device = codes[np.dtype(bp.dtype)], 1, bp.device
    else:
        vol = np.asarray(volume)
        if vol.ndim != 3:
            raise ValueError("volume must be 3-D")
        if vol.dtype == np.bool_:
            vol = vol.view(np.uint8)
        if vol.dtype not in codes:
            vol = vol.astype(np.float64)
        keep = np.ascontiguousarray(vol)
        ptr, shape, code, on_device = nat.addr(keep), list(keep.shape), codes[keep.dtype], 0
    return _vol2pcd_call("sc_vol2pcd", (ptr, on_device, code), shape, device, *tail)


def _vol2pcd_call(entry, head, shape, device, origin64, voxel_size, level_set_value, as_open3d, what=None):
    """What the ``sc_vol2pcd*`` calls of ``vol2pcd`` and ``vol2pcd_class`` share: the arguments that follow an entry's own
    (``head``: its input), the call, its check (reported as ``what``, the entry unless given) and the cloud."""
    from . import _native as nat

    b = nat.backend()
    gw = gaussian_weights(1.0)
    assert gw.size == 5
    out = np.zeros(2, dtype=np.uintp)
    cnt = np.zeros(1, dtype=np.int64)
    nat.unit_call(entry, *head, shape[0], shape[1], shape[2], nat.addr(origin64), float(voxel_size), float(level_set_value),
                  nat.addr(gw), int(device), nat.addr(out), nat.addr(out) + 8, nat.addr(cnt), what=what)
    return _adopt_cloud(b, out, cnt, as_open3d)


def set_select_chunk_bytes(nbytes):
    """Largest device work buffer a ``select_classes`` call on host arrays may take (``sc_select_set_chunk_bytes``;
    default 256 MiB, 0 restores it): larger stacks go through in x-slabs of whole planes, same winners."""
    from . import _native as nat
    nat.backend().call("sc_select_set_chunk_bytes", int(nbytes))


def select_classes(voxels, background_prior=1.0, min_contrast=10.0, min_score=0.2, background="background", device=0):
    """The decision step of the multiclass ``PointCloud.run`` (``tasks/proc3d.py:84-115``) on the GPU
    (``sc_select_classes``, ``csrc/class_select.hip``; the rule is the contract in ``include/spacecarve.h``).

    voxels : dict ``{label: volume}`` of at least two and at most 32 classes, in the reference's key order.  All
        volumes are NumPy arrays of one shape ``(nx, ny, nz)`` and dtype, or all contiguous CUDA torch tensors of one
        device, shape and dtype (read in place on torch's current stream).  float32, float64 and uint8 are read as they
        are; bool is viewed as uint8; NumPy arrays of other dtypes are converted to float64 on the host.  Comparisons
        are in float64.
    background : the label whose value is multiplied by ``background_prior`` and that owns no voxel, or ``None``.

    Returns ``(winner, labels, counts)``: ``winner`` uint8 ``[nx, ny, nz]`` -- the index into ``labels`` of the class
    the voxel belongs to, 255 for none; the reference's volume of class ``c`` is ``winner == c`` -- a NumPy array, or a
    CUDA tensor on the inputs' device; ``labels = list(voxels.keys())``; ``counts`` int64 ``[L]``, the voxels of each
    class (0 for the background)."""
    from . import _native as nat, _operands as ops

    labels = list(voxels.keys())
    L = len(labels)
    if L < 2:
        raise ValueError("at least two classes are needed (with one key the reference takes its single-volume branch)")
    if L > 32:
        raise ValueError("at most 32 classes")
    s = ops.class_stack([voxels[label] for label in labels], "voxels", (nat.SC_EVAL_F32, nat.SC_EVAL_F64, nat.SC_EVAL_U8),
                        "device volumes must be float32, float64, uint8 or bool", device)
    if min(s.shape) < 1:
        raise ValueError("volumes must not be empty")
    bg = labels.index(background) if background in labels else -1
    winner = ops.empty_uint8(s.shape, s.tdevice)
    counts = np.zeros(L, dtype=np.int64)
    nat.unit_call("sc_select_classes", nat.addr(s.table), s.code, L, bg, s.shape[0], s.shape[1], s.shape[2], float(background_prior),
                  float(min_contrast), float(min_score), s.on_device, s.device, s.stream, ops.ptr_of(winner), nat.addr(counts))
    return winner, labels, counts


def vol2pcd_class(winner, index, origin, voxel_size, level_set_value=0, device=0, as_open3d=True):
    """``vol2pcd`` of one class of a winner volume: the cloud of ``winner == index`` (``sc_vol2pcd_class``), bit for bit
    what ``vol2pcd((winner == index).astype(np.uint8), ...)`` returns -- without that volume being made.

    winner : uint8 ``[nx, ny, nz]``, what ``select_classes`` returns: a NumPy array, or a contiguous CUDA torch tensor
        read in place (it never leaves the device; only points and normals come back).
    index : the class, 0..255 (255: the voxels of no class)."""
    from . import _native as nat, _operands as ops

    nat.backend()
    origin64 = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))  # judged before the volume
    if ops.is_tensor(winner):
        import torch
        if winner.dtype != torch.uint8 or winner.dim() != 3 or not winner.is_contiguous() or not winner.is_cuda:
            raise ValueError("a device winner volume must be a contiguous uint8 CUDA tensor [nx, ny, nz]")
        torch.cuda.current_stream(winner.device.index).synchronize()  # sc_vol2pcd_class runs on the default stream
        keep, shape = winner, [int(s) for s in winner.shape]
        ptr, on_device, device = winner.data_ptr(), 1, winner.device.index
    else:
        keep = np.asarray(winner)
        if keep.ndim != 3 or keep.dtype != np.uint8:
            raise ValueError("the winner volume must be uint8 [nx, ny, nz]")
        keep = np.ascontiguousarray(keep)
        ptr, shape, on_device = nat.addr(keep), list(keep.shape), 0
    return _vol2pcd_call("sc_vol2pcd_class", (ptr, on_device, int(index)), shape, device, origin64, voxel_size, level_set_value, as_open3d)


def backproject_points(points, K, rot, tvec):
    """``plant3dvision/proc3d.py:655-659`` (host, NumPy): pixel coordinates of 3-D points."""
    x = rot @ points.transpose() + tvec[:, np.newaxis]
    x = K @ x
    x = x / x[2, :][np.newaxis, :]
    return x[:2, :].transpose()


def label_points(points, cameras, masks, device=0):
    """The scoring loop of ``SegmentedPointCloud.run`` (``tasks/proc3d.py:203-232``) on the GPU.

    points  : ``[P, 3]`` float64 (``np.asarray(pcd.points)``)
    cameras : list of V camera dicts (``colmap_camera`` / ``camera`` metadata schema)
    masks   : uint8 ``[L, V, H, W]`` -- NumPy array, or a CUDA torch tensor (e.g. stacked
              ``masks2d.masks_from_predictions`` output) used in place
    Returns ``(labels int32 [P], scores float64 [L, P])``; ``labels[i]`` indexes the L labels in
    the order given (the reference iterates a Python ``set``; fix the order yourself).
    """
    from . import _native as nat, _operands as ops

    nat.backend()
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    P = pts.shape[0]
    V = len(cameras)
    K = np.ascontiguousarray(np.array([c["camera_model"]["params"][0:4] for c in cameras], dtype=np.float64).reshape(V, 4))
    R = np.ascontiguousarray(np.array([c["rotmat"] for c in cameras], dtype=np.float64).reshape(V, 9))
    t = np.ascontiguousarray(np.array([c["tvec"] for c in cameras], dtype=np.float64).reshape(V, 3))
    if ops.is_tensor(masks):  # torch tensor on the device
        import torch
        if masks.dtype != torch.uint8 or masks.dim() != 4 or not masks.is_contiguous() or not masks.is_cuda:
            raise ValueError("device masks must be a contiguous uint8 CUDA tensor [L, V, H, W]")
        torch.cuda.current_stream(masks.device.index).synchronize()
        L, Vm, H, W = (int(s) for s in masks.shape)
        mptr, on_dev, device = masks.data_ptr(), 1, masks.device.index
    else:
        m = np.ascontiguousarray(np.asarray(masks))
        if m.dtype != np.uint8 or m.ndim != 4:
            raise ValueError("masks must be uint8 [L, V, H, W]")
        L, Vm, H, W = m.shape
        mptr, on_dev = nat.addr(m), 0
    if Vm != V:
        raise ValueError("one camera per view")
    scores = np.zeros((L, P), dtype=np.float64)
    labels = np.zeros(P, dtype=np.int32)
    nat.unit_call("sc_label_points", nat.addr(pts), P, L, V, nat.addr(K), nat.addr(R), nat.addr(t), mptr, on_dev,
                  H, W, int(device), nat.addr(scores), nat.addr(labels))
    return labels, scores


def cluster_dbscan(points, eps, min_points, device=0):
    """open3d's ``PointCloud.cluster_dbscan(eps, min_points)`` -- what ``OrganSegmentation.run`` calls per label
    (``tasks/proc3d.py:507-508``) -- on the GPU (``sc_dbscan``, ``csrc/dbscan.hip``).

    points : array-like ``[P, 3]``, a :class:`PointCloud` or anything with ``.points`` -> ``np.int32 [P]``; or a
        contiguous float64 CUDA torch tensor ``[P, 3]``, read in place on torch's current stream -> a CUDA int32 tensor
        on the same device.
    Labels: cluster ids from 0 in the order of each cluster's smallest point index, ``-1`` for noise.

    PARITY UNPINNED: open3d is not available here.  The rules restate its sequential loop in an
    order-free form: ``d2 = ((dx dx) + (dy dy)) + (dz dz)`` in float64, neighbours iff ``d2 < eps * eps`` (strict: a
    pair at exactly ``eps`` is not; a point is its own neighbour), core iff at least ``min_points`` neighbours,
    clusters = connected components of the core points, a border point joins the smallest id among its core
    neighbours.  Deviation: non-finite coordinates (and ``eps`` that is not finite and positive) raise ``ValueError``.
    """
    from . import _native as nat, _operands as ops

    nat.backend()
    p = ops.points(points, "points", "[P, 3]")
    P = p.n
    if p.on_device:
        import torch
        out = torch.empty((P,), dtype=torch.int32, device=p.points.device)
        if P:
            dev, stream = ops.tensor_place(p.points)
            nat.unit_call("sc_dbscan", p.ptr, 1, P, float(eps), int(min_points), int(dev), out.data_ptr(), 1, 0, int(stream))
        return out
    labels = np.full(max(P, 1), -1, dtype=np.int32)
    nat.unit_call("sc_dbscan", p.ptr, 0, P, float(eps), int(min_points), int(device), nat.addr(labels), 0, 0, 0)
    return labels[:P]


def _max_distance_arg(max_distance):
    """``None`` -> 0.0 (unbounded, rule N3); anything else must be positive and finite (rule N5)."""
    if max_distance is None:
        return 0.0
    md = float(max_distance)
    if not (md > 0.0 and md != float("inf")):
        raise ValueError("max_distance must be positive and finite (None: unbounded)")
    return md


def _nearest_call(queries, targets, max_distance, device, want_points, want_sums):
    """One ``sc_nearest`` call: ``(index, d2, sums)``; ``index`` / ``d2`` are ``None`` without ``want_points``,
    ``sums`` (NumPy float64 ``[3]``: n, sum d2, sum sqrt d2) is ``None`` without ``want_sums``."""
    from . import _native as nat, _operands as ops

    md = _max_distance_arg(max_distance)
    q, t = ops.points(queries, "queries"), ops.points(targets, "targets")
    if q.on_device != t.on_device:
        raise ValueError("queries and targets must both be arrays (or clouds) or both CUDA tensors")
    Q, P = q.n, t.n
    sums = np.zeros(3, dtype=np.float64) if want_sums else None
    sptr = nat.addr(sums) if want_sums else 0
    if q.on_device:
        import torch
        if q.points.device != t.points.device:
            raise ValueError("queries and targets must be on one device")
        index = d2 = None
        if want_points:
            index = torch.full((Q,), -1, dtype=torch.int32, device=q.points.device)
            d2 = torch.full((Q,), float("inf"), dtype=torch.float64, device=q.points.device)
        if Q and P:  # rule N4 otherwise: the outputs are filled already
            dev, stream = ops.tensor_place(q.points)
            nat.unit_call("sc_nearest", q.ptr, 1, Q, t.ptr, 1, P, md, int(dev), index.data_ptr() if want_points else 0,
                          d2.data_ptr() if want_points else 0, 1, sptr, int(stream))
        return index, d2, sums
    index = np.full(max(Q, 1), -1, dtype=np.int32)
    d2 = np.full(max(Q, 1), np.inf, dtype=np.float64)
    nat.unit_call("sc_nearest", q.ptr, 0, Q, t.ptr, 0, P, md, int(device), nat.addr(index), nat.addr(d2), 0, sptr, 0)
    return (index[:Q], d2[:Q], sums) if want_points else (None, None, sums)


def nearest_points(queries, targets, max_distance=None, device=0):
    """For every query the nearest point of ``targets`` and its squared distance, on the GPU (``sc_nearest``,
    ``csrc/nearest.hip``): the primitive under open3d's ``compute_point_cloud_distance``,
    ``evaluate_registration`` and the ``KDTreeFlann`` loop of ``CompareSegmentedPointClouds``.

    queries, targets : array-likes ``[n, 3]``, :class:`PointCloud` objects or anything with ``.points`` -> NumPy
        ``(index int32 [Q], d2 float64 [Q])``; or two contiguous float64 CUDA torch tensors ``[n, 3]`` on one device,
        read in place on torch's current stream -> CUDA tensors on that device.  Mixed kinds raise ``ValueError``.
    max_distance : ``None`` (unbounded) or a positive finite number.

    PARITY UNPINNED: open3d is not available here.  The rules restate nanoflann's search in an
    order-free form: N1 ``d2 = ((dx dx) + (dy dy)) + (dz dz)`` in float64; N2 the least ``d2`` wins, among equal ``d2``
    the smallest target index; N3 with ``max_distance`` a query is matched iff ``d2 < max_distance * max_distance``
    (strict; at exactly ``max_distance`` it is not), an unmatched query reports ``-1`` and ``+inf``; N4 no target: all
    ``-1`` / ``+inf``.  Deviation (N5): non-finite coordinates, and a ``max_distance`` that is not positive and finite,
    raise ``ValueError``.  There is no CPU fallback."""
    index, d2, _ = _nearest_call(queries, targets, max_distance, device, True, False)
    return index, d2


def nearest_sums(queries, targets, max_distance=None, device=0):
    """``(n, sum d2, sum sqrt(d2))`` over the matched queries (rule N6: added in an order fixed by the number of
    queries alone, so two calls give the same bits); no per-query array leaves the device."""
    _, _, sums = _nearest_call(queries, targets, max_distance, device, False, True)
    return int(sums[0]), float(sums[1]), float(sums[2])


def nearest_confusion(index, query_labels, target_labels, n_labels, device=0):
    """``counts[a, b]`` = queries of label id ``a`` whose nearest target has label id ``b`` (``sc_nearest_confusion``):
    NumPy int64 ``[L, L]``.  ``index`` / ``query_labels`` are both int32 NumPy arrays or both int32 CUDA tensors,
    ``target_labels`` either; queries with index -1 are not counted; ids outside ``0..L-1`` raise ``ValueError``."""
    from . import _native as nat, _operands as ops

    L = int(n_labels)
    if ops.is_tensor(index) != ops.is_tensor(query_labels):
        raise ValueError("index and query_labels must both be arrays or both CUDA tensors")
    i, q, t = ops.ids(index, "index"), ops.ids(query_labels, "query_labels"), ops.ids(target_labels, "target_labels")
    if i.n != q.n:
        raise ValueError("one label per query")
    devs = [a.tdevice for a in (i, q, t) if a.on_device]
    if len(set(devs)) > 1:
        raise ValueError("the device arrays must be on one device")
    stream = 0
    if devs:
        import torch
        device = devs[0].index
        stream = torch.cuda.current_stream(device).cuda_stream
    counts = np.zeros((max(L, 1), max(L, 1)), dtype=np.int64)
    nat.unit_call("sc_nearest_confusion", i.ptr, q.ptr, i.on_device, i.n, t.ptr, t.on_device, t.n, L, int(device), nat.addr(counts),
                  int(stream))
    return counts


def knn_points(queries, targets, k, max_distance=None, device=0, return_far=False):
    """For every query its ``k`` nearest points of ``targets`` and their squared distances, on the GPU (``sc_knn``,
    ``csrc/nearest.hip``): open3d's ``KDTreeFlann.search_knn_vector_3d(p, k)`` for all queries at once.

    queries, targets : as for :func:`nearest_points` -- array-likes ``[n, 3]``, :class:`PointCloud` objects or anything
        with ``.points`` -> NumPy ``(index int32 [Q, k], d2 float64 [Q, k])``; or two contiguous float64 CUDA torch
        tensors ``[n, 3]`` on one device, read in place on torch's current stream -> CUDA tensors on that device.  Mixed
        kinds raise ``ValueError``.
    k : 1 .. ``SC_KNN_MAX`` (512); ``Q * k`` must be below 2^31.
    max_distance : ``None`` (unbounded) or a positive finite number.
    return_far : also return the number of queries the pass over all targets took (the call then waits at its end).

    PARITY UNPINNED: open3d is not available here.  The rules restate nanoflann's search in an
    order-free form: K1 ``d2`` is N1's ``((dx dx) + (dy dy)) + (dz dz)`` in float64; K2 a target's key is ``(d2, index)``,
    compared lexicographically, and row ``q`` holds the ``min(k, matched targets)`` smallest keys in rising key order -- a
    tie at the k-th place goes to the smaller index; K3 with ``max_distance`` only targets with
    ``d2 < max_distance * max_distance`` count (strict); K4 unused places, after the used ones, hold ``-1`` and ``+inf``
    (no target: every place); K5 non-finite coordinates, a bad ``max_distance``, ``k`` outside ``1..SC_KNN_MAX`` and
    ``Q * k >= 2^31`` raise ``ValueError``; K6 ``k = 1`` gives exactly ``nearest_points``' answer.  No CPU fallback."""
    from . import _native as nat, _operands as ops

    md = _max_distance_arg(max_distance)
    k = int(k)
    if not 1 <= k <= nat.SC_KNN_MAX:
        raise ValueError(f"k must be 1 .. {nat.SC_KNN_MAX}")
    q, t = ops.points(queries, "queries"), ops.points(targets, "targets")
    if q.on_device != t.on_device:
        raise ValueError("queries and targets must both be arrays (or clouds) or both CUDA tensors")
    Q, P = q.n, t.n
    if Q * k >= 2 ** 31:
        raise ValueError("Q * k must be below 2^31")
    far = np.zeros(1, dtype=np.int64)
    fptr = nat.addr(far) if return_far else 0

    def call(*args):  # sc_knn is an entry of the nearest unit: its errors are read with that unit's getter
        nat.check(nat.backend().call("sc_knn", *args), "sc_knn", "sc_nearest_last_error")

    if q.on_device:
        import torch
        if q.points.device != t.points.device:
            raise ValueError("queries and targets must be on one device")
        index = torch.full((Q, k), -1, dtype=torch.int32, device=q.points.device)
        d2 = torch.full((Q, k), float("inf"), dtype=torch.float64, device=q.points.device)
        if Q and P:  # rule K4 otherwise: the outputs are filled already
            dev, stream = ops.tensor_place(q.points)
            call(q.ptr, 1, Q, t.ptr, 1, P, k, md, int(dev), index.data_ptr(), d2.data_ptr(), 1, fptr, int(stream))
    else:
        index = np.full((max(Q, 1), k), -1, dtype=np.int32)
        d2 = np.full((max(Q, 1), k), np.inf, dtype=np.float64)
        call(q.ptr, 0, Q, t.ptr, 0, P, k, md, int(device), nat.addr(index), nat.addr(d2), 0, fptr, 0)
        index, d2 = index[:Q], d2[:Q]
    return (index, d2, int(far[0])) if return_far else (index, d2)


def knn_edges(points, k, device=0, knn_fn=None):
    """The edge set of the reference's ``knn_graph`` (``plant3dvision/proc3d.py:160-183``): for every point ``i`` of the
    cloud and each of its ``k`` nearest points ``j`` of the same cloud -- ``i`` itself among them, as in the reference,
    which adds the self-loop ``i-i`` of weight 0 -- the pair ``(min(i, j), max(i, j))``.

    Returns ``(edges int32 [E, 2], weights float64 [E])``: the pairs deduplicated and sorted lexicographically, the
    weight ``sqrt(d2)`` (``d2`` is bitwise symmetric under rule N1, so both directions of an edge carry one weight).
    The search is :func:`knn_points` on the GPU (``knn_fn(points, points, k)`` replaces it in tests); removing the
    duplicates is host NumPy."""
    from . import _operands as ops

    if knn_fn is None:
        def knn_fn(a, b, kk):
            return knn_points(a, b, kk, device=device)
    p = ops.points(points, "points")
    if p.on_device:
        raise ValueError("knn_edges takes host points (the edges are deduplicated on the host)")
    index, d2 = knn_fn(p.points, p.points, int(k))
    index, d2 = np.asarray(index), np.asarray(d2)
    i = np.broadcast_to(np.arange(p.n, dtype=np.int64)[:, None], index.shape)
    used = index >= 0
    return _fold_edges(i[used], index[used], d2[used], p.n)


def _fold_edges(i, j, d2, n):
    """The tail ``knn_edges`` and ``radius_edges`` share: the directed pairs ``i -> j`` (flat arrays, ``d2`` beside them)
    of a cloud of ``n`` points become ``(edges int32 [E, 2], weights float64 [E])`` -- ``(min, max)``, deduplicated,
    sorted lexicographically, weight ``sqrt(d2)`` of the first pair of each edge (``d2`` is bitwise symmetric)."""
    i, j, w = np.asarray(i, dtype=np.int64), np.asarray(j).astype(np.int64), np.sqrt(d2)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    key, first = np.unique(lo * max(n, 1) + hi, return_index=True)  # rising key: lexicographic in (lo, hi)
    edges = np.stack([key // max(n, 1), key % max(n, 1)], axis=1).astype(np.int32).reshape(-1, 2)
    return edges, np.ascontiguousarray(w[first])


def knn_graph(pcd, k, device=0, knn_fn=None):
    """``plant3dvision/proc3d.py:160-183``: the weighted undirected ``networkx.Graph`` that connects every point to its
    ``k`` nearest neighbours (itself included: a self-loop of weight 0).  Node ``i`` carries ``center`` (the point),
    an edge ``weight`` (the distance).  Built from :func:`knn_edges`; raises ``ImportError`` without networkx."""
    try:
        import networkx as nx
    except ImportError as e:
        raise ImportError("knn_graph needs networkx (knn_edges returns the same edges as arrays without it)") from e
    from . import _operands as ops

    pts = ops.points(pcd, "points").points
    edges, weights = knn_edges(pts, k, device=device, knn_fn=knn_fn)
    g = nx.Graph()
    for i in range(len(pts)):
        g.add_node(i, center=pts[i])
    g.add_weighted_edges_from((int(a), int(b), float(w)) for (a, b), w in zip(edges.tolist(), weights.tolist()))
    return g


def _radius_operands(queries, targets, radius):
    """What ``radius_counts`` and ``radius_points`` share: the radius judged (rule R5), the two clouds through
    ``_operands.points``, their kinds and devices compared.  ``(q, t, radius, place)``; ``place`` is ``None`` for host
    arrays, else ``(device index, torch's current stream there)``."""
    from . import _operands as ops

    r = float(radius)
    if not (r > 0.0 and r != float("inf")):
        raise ValueError("radius must be positive and finite")
    q, t = ops.points(queries, "queries"), ops.points(targets, "targets")
    if q.on_device != t.on_device:
        raise ValueError("queries and targets must both be arrays (or clouds) or both CUDA tensors")
    if q.on_device and q.points.device != t.points.device:
        raise ValueError("queries and targets must be on one device")
    return q, t, r, (ops.tensor_place(q.points) if q.on_device else None)


def _radius_call(q, t, r, place, device, counts=None, offsets=None, index=None, d2=None, want_long=False):
    """One ``sc_radius`` call on non-empty clouds: ``(E, rows the long-row launch sorted)``.  The outputs given are
    filled; ``index`` / ``d2`` hold ``capacity = len(index)`` places."""
    from . import _native as nat, _operands as ops

    out = np.zeros(2, dtype=np.int64)  # total_out, long_out
    dev, stream = place if place is not None else (int(device), 0)
    ptr = [0 if a is None else ops.ptr_of(a) for a in (counts, offsets, index, d2)]
    # sc_radius is an entry of the nearest unit: its errors are read with that unit's getter
    nat.check(nat.backend().call("sc_radius", q.ptr, q.on_device, q.n, t.ptr, t.on_device, t.n, r, int(dev), ptr[0], ptr[1], ptr[2], ptr[3],
                                 0 if index is None else int(index.shape[0]), q.on_device, nat.addr(out),
                                 nat.addr(out) + 8 if want_long else 0, int(stream)), "sc_radius", "sc_nearest_last_error")
    return int(out[0]), int(out[1])


def _radius_array(q, n, dtype, zero=False):
    """An output of ``n`` places of the queries' kind: a CUDA tensor on their device, or a NumPy array."""
    if q.on_device:
        import torch
        make = torch.zeros if zero else torch.empty
        return make((n,), dtype=getattr(torch, np.dtype(dtype).name), device=q.points.device)
    return (np.zeros if zero else np.empty)(n, dtype=dtype)


def radius_counts(queries, targets, radius, device=0):
    """For every query the number of points of ``targets`` within ``radius`` (rule R2: ``d2 < radius * radius``,
    strict), on the GPU: one ``sc_radius`` call without row outputs.  int32 ``[Q]``, a NumPy array or a
    CUDA tensor as the inputs are (see :func:`radius_points`).  On one cloud searched against itself
    ``radius_counts(p, p, eps) >= min_points`` is exactly ``cluster_dbscan``'s core test (rule R7)."""
    q, t, r, place = _radius_operands(queries, targets, radius)
    counts = _radius_array(q, q.n, np.int32, zero=True)
    if q.n and t.n:  # rule R4 otherwise: no device call, the zeros stand
        _radius_call(q, t, r, place, device, counts=counts)
    return counts


def radius_points(queries, targets, radius, device=0, return_long=False):
    """For every query ALL points of ``targets`` within ``radius``, nearest first, on the GPU (``sc_radius``,
    ``csrc/nearest.hip``): open3d's ``KDTreeFlann.search_radius_vector_3d(p, radius)`` for all queries
    at once.  (``search_hybrid_vector_3d(p, radius, max_nn)`` is ``knn_points(..., k=max_nn, max_distance=radius)``.)

    queries, targets : as for :func:`nearest_points` -- array-likes ``[n, 3]``, :class:`PointCloud` objects or anything
        with ``.points`` -> NumPy arrays; or two contiguous float64 CUDA torch tensors ``[n, 3]`` on one device, read in
        place on torch's current stream -> CUDA tensors on that device.  Mixed kinds raise ``ValueError``.
    radius : positive and finite.
    return_long : also return the number of rows longer than ``SC_RADIUS_LDS_ROW``, which the long-row launch sorted.

    Returns ``(offsets int64 [Q + 1], index int32 [E], d2 float64 [E])``, the rows in CSR form: row ``q`` is
    ``index[offsets[q]:offsets[q + 1]]``, ``E = offsets[Q]``.  Two calls are made: one for ``E``, one that fills arrays
    of exactly ``E`` places; inputs changed in between (another total) raise ``RuntimeError``.

    PARITY UNPINNED: open3d is not available here.  The rules restate nanoflann's search in an
    order-free form: R1 ``d2`` is N1's ``((dx dx) + (dy dy)) + (dz dz)`` in float64; R2 a target is a neighbour iff
    ``d2 < radius * radius`` (strict, the product rounded once: a target at exactly ``radius`` is not); R3 a row holds
    all neighbours in rising ``(d2, index)``; R4 no query: ``offsets = [0]``, no target: empty rows; R5 non-finite
    coordinates and a ``radius`` that is not positive and finite raise ``ValueError``.  No CPU fallback."""
    q, t, r, place = _radius_operands(queries, targets, radius)
    total = nlong = 0
    if q.n and t.n:
        total, _ = _radius_call(q, t, r, place, device)
    offsets = _radius_array(q, q.n + 1, np.int64, zero=True)
    index, d2 = _radius_array(q, total, np.int32), _radius_array(q, total, np.float64)
    if total:  # otherwise every row is empty and the zeros stand: no zero-length array goes to the library
        again, nlong = _radius_call(q, t, r, place, device, offsets=offsets, index=index, d2=d2, want_long=return_long)
        if again != total:
            raise RuntimeError(f"radius_points: {total} neighbours on the first call, {again} on the second: the inputs were changed in between")
    return (offsets, index, d2, nlong) if return_long else (offsets, index, d2)


def radius_edges(points, r, device=0, radius_fn=None):
    """The edge set of the reference's ``radius_graph`` (``plant3dvision/proc3d.py:186-209``): for every point ``i`` of
    the cloud and every point ``j`` of the same cloud within ``r`` of it -- ``i`` itself among them (``d2 = 0 < r * r``),
    as the reference's loop adds the self-loop ``i-i`` -- the pair ``(min(i, j), max(i, j))``.

    Returns ``(edges int32 [E', 2], weights float64 [E'])`` as :func:`knn_edges` does: deduplicated, sorted
    lexicographically, weight ``sqrt(d2)``.  The search is :func:`radius_points` on the GPU (``radius_fn(points, points,
    r)`` replaces it in tests); removing the duplicates is host NumPy."""
    from . import _operands as ops

    if radius_fn is None:
        def radius_fn(a, b, rr):
            return radius_points(a, b, rr, device=device)
    p = ops.points(points, "points")
    if p.on_device:
        raise ValueError("radius_edges takes host points (the edges are deduplicated on the host)")
    offsets, index, d2 = radius_fn(p.points, p.points, float(r))
    offsets, index, d2 = np.asarray(offsets), np.asarray(index), np.asarray(d2)
    i = np.repeat(np.arange(p.n, dtype=np.int64), np.diff(offsets))
    return _fold_edges(i, index, d2, p.n)


def radius_graph(pcd, r, device=0, radius_fn=None):
    """``plant3dvision/proc3d.py:186-209``: the weighted undirected ``networkx.Graph`` that connects every point to all
    points within ``r`` of it (itself included: a self-loop of weight 0).  Nodes are ``0..n-1`` and carry no attribute
    (the reference's ``radius_graph`` sets no ``center``), an edge carries ``weight`` (the distance).  Built from
    :func:`radius_edges`; raises ``ImportError`` without networkx."""
    try:
        import networkx as nx
    except ImportError as e:
        raise ImportError("radius_graph needs networkx (radius_edges returns the same edges as arrays without it)") from e
    from . import _operands as ops

    pts = ops.points(pcd, "points").points
    edges, weights = radius_edges(pts, r, device=device, radius_fn=radius_fn)
    g = nx.Graph()
    g.add_nodes_from(range(len(pts)))
    g.add_weighted_edges_from((int(a), int(b), float(w)) for (a, b), w in zip(edges.tolist(), weights.tolist()))
    return g


# ---- the graph steps of the XU skeleton (plant3dvision/proc3d.py:212-426) ---------------------------------
def _graph_call(entry, *args):
    """One call of the graph unit; its errors are read with the unit's own getter, ``sc_graph_error``."""
    from . import _native as nat
    nat.check(nat.backend().call(entry, *args), entry, "sc_graph_error")


def _graph_place(g, device):
    """``(device index, stream)`` of a graph call: the tensors' device and torch's current stream there, or ``device``."""
    from . import _operands as ops
    return ops.tensor_place(g.arcs) if g.on_device else (int(device), 0)


def graph_distances(rows, root, n=None, extra=None, device=0, return_rounds=False):
    """Shortest-path distances from node ``root`` to every node of the graph the rows span, on the GPU
    (``sc_graph_distances``, ``csrc/graph.hip``): the distances of
    ``nx.dijkstra_predecessor_and_distance(g, root)`` over ``knn_graph`` / ``radius_graph`` (``proc3d.py:287``), without
    the ``networkx.Graph``.

    rows : ``(index [N, k], d2 [N, k])`` as :func:`knn_points` ``(p, p, k)`` returns them (``-1`` in unused places) or
        ``(offsets, index, d2)`` as :func:`radius_points` ``(p, p, r)`` does: NumPy arrays -> a NumPy float64 ``[N]``; or
        contiguous CUDA tensors on one device, read in place on torch's current stream -> a CUDA tensor there.  Mixed
        kinds raise ``ValueError``.  The values are SQUARED distances; an arc's weight is their square root (rule G1).
    extra : ``None`` or ``(edges int32 [M, 2], weights float64 [M])``, more edges with plain weights: what
        :func:`connect_edges` returns.
    n : the node count, when given checked against the rows.
    return_rounds : also return the number of frontier rounds the device ran.

    PINNED: rule G2 -- ``d[root] = 0``, ``d[v]`` the least left-to-right float64 sum over all walks, every
    arc usable in both directions, ``+inf`` where no walk exists -- is what Dijkstra with a float64 accumulator returns,
    bit for bit; ``tests/test_graph_host.py`` compares the checker with networkx and scipy.  Rule G4: an index out of
    range, offsets that do not rise from 0 to E, a NaN, negative or infinite value and a bad root raise ``ValueError``.
    No nodes: an empty result, no native call.  There is no CPU fallback."""
    from . import _native as nat, _operands as ops

    g = ops.graph_rows(rows, n, extra)
    root = int(root)
    if g.n and not 0 <= root < g.n:
        raise ValueError(f"root must be 0 .. {g.n - 1}")
    rounds = np.zeros(1, dtype=np.int64)
    if g.on_device:
        import torch
        out = torch.empty((g.n,), dtype=torch.float64, device=g.tdevice)
    else:
        out = np.empty(g.n, dtype=np.float64)
    if g.n:
        dev, stream = _graph_place(g, device)
        _graph_call("sc_graph_distances", g.n, g.offsets, g.row_len, g.index, g.values, g.E, 1, g.extra, g.extra_w, g.M, g.on_device,
                    root, int(dev), ops.ptr_of(out), nat.addr(rounds) if return_rounds else 0, int(stream))
    return (out, int(rounds[0])) if return_rounds else out


def graph_components(rows, key=None, n=None, extra=None, device=0):
    """Connected components of the graph the rows span, on the GPU (``sc_graph_components``, ``csrc/graph.hip``):
    ``nx.connected_components`` of ``knn_graph`` / ``radius_graph`` (``proc3d.py:229``), or with ``key`` the components
    of every ``g.subgraph(nodes of one key)`` at once (``proc3d.py:307-308``).

    rows, extra, n : as for :func:`graph_distances` (the values are judged for shape only).
    key : ``None`` or int32 ``[N]`` of the rows' kind: an edge joins its ends only where ``key[i] == key[j] >= 0``.

    Returns ``(labels int32 [N], components)``: ``labels[v]`` is the rank of ``v``'s component when components are
    ordered by their smallest member (``cluster_dbscan``'s numbering), ``-1`` for nodes whose key is negative (rule G3)."""
    from . import _native as nat, _operands as ops

    g = ops.graph_rows(rows, n, extra)
    k = None if key is None else ops.node_ids(g, key, "key")
    kptr = 0 if k is None else k.ptr
    count = np.zeros(1, dtype=np.int32)
    if g.on_device:
        import torch
        labels = torch.empty((g.n,), dtype=torch.int32, device=g.tdevice)
    else:
        labels = np.empty(g.n, dtype=np.int32)
    if g.n:
        dev, stream = _graph_place(g, device)
        _graph_call("sc_graph_components", g.n, g.offsets, g.row_len, g.index, g.E, g.extra, g.M, kptr, g.on_device, int(dev),
                    ops.ptr_of(labels), nat.addr(count), int(stream))
    return labels, int(count[0])


def connect_edges(points, labels, root_index, device=0, n_labels=None):
    """The edges the reference's ``connect_graph`` (``proc3d.py:212-263``) adds to make a graph connected, in an
    order-free form, on the GPU (``sc_graph_connect``, ``csrc/graph_connect.inl``).  ``labels``: the
    component of every point (:func:`graph_components`), or any other labelling.  While a point lies outside the root's
    label ``R``: among all pairs ``(i not in R, j in R)`` the one with the least key ``(d2, i, j)`` becomes an edge of
    weight ``sqrt(d2)``, and every point with ``i``'s label joins ``R`` (rules C1, C2 of ``include/spacecarve.h``; ``d2``
    is rule N1's).

    points, labels : an array-like ``[n, 3]`` (or a :class:`PointCloud`) and any integers ``[n]`` -- they are compacted to
        ``0 .. L - 1`` on the host before the call -- -> NumPy results; or a contiguous float64 CUDA tensor ``[n, 3]`` and
        a contiguous int32 CUDA tensor ``[n]`` of labels ``0 .. n_labels - 1`` on one device, read in place on torch's
        current stream -> CUDA tensors on that device.  Mixed kinds raise ``ValueError``.
    n_labels : the label bound of tensor labels, :func:`graph_components`' count; ``None`` asks the device for
        ``labels.max() + 1``, which costs one wait.  With arrays it is ignored (the compaction gives it).

    Returns ``(edges int32 [M, 2], weights float64 [M])``, ``M = (labels with members) - 1``, each edge as ``(i, j)``:
    feed them to :func:`graph_distances` / :func:`graph_components` / :func:`graph_quotient` as ``extra``.  No points, one
    label (``n_labels <= 1``, or host labels that are all the root's): empty results, no native call.  A label outside
    ``0 .. n_labels - 1`` and a non-finite coordinate raise ``ValueError`` (rule C3).  There is no CPU fallback.

    Deviation: the reference stores ``nnorm``, the norm of the LAST point its loop visited, as the new edge's weight where
    it means ``minnorm`` (``proc3d.py:262-263``); ours is the minimum, the length of the edge."""
    from . import _native as nat, _operands as ops

    p = ops.points(points, "points")
    if ops.is_tensor(labels) != bool(p.on_device):
        raise ValueError("points and labels must be both arrays (or a cloud) or both CUDA tensors")
    lab = ops.ids(labels, "labels").data if p.on_device else np.asarray(labels).reshape(-1)
    if len(lab) != p.n:
        raise ValueError("one label per point")
    if p.on_device and lab.device != p.points.device:
        raise ValueError("points and labels must be on one device")
    root = int(root_index)
    if p.n and not 0 <= root < p.n:
        raise ValueError(f"root_index must be 0 .. {p.n - 1}")
    if p.on_device:
        import torch

        def empty(shape, dtype):
            return torch.empty(shape, dtype=getattr(torch, dtype), device=p.points.device)
        L = 0 if not p.n else int(n_labels) if n_labels is not None else int(lab.max()) + 1
    else:
        def empty(shape, dtype):
            return np.empty(shape, dtype=dtype)
        values, lab = np.unique(lab, return_inverse=True)  # any integers -> 0 .. L - 1
        lab = np.ascontiguousarray(lab.reshape(-1), dtype=np.int32)
        L = len(values)
    if p.n == 0 or L <= 1:
        return empty((0, 2), "int32"), empty((0,), "float64")
    dev, stream = ops.tensor_place(p.points) if p.on_device else (int(device), 0)
    edges, weights = empty((L - 1, 2), "int32"), empty((L - 1,), "float64")
    count = np.zeros(1, dtype=np.int64)
    _graph_call("sc_graph_connect", p.n, p.ptr, ops.ptr_of(lab), L, root, p.on_device, int(dev), ops.ptr_of(edges), ops.ptr_of(weights), nat.addr(count),
                int(stream))
    m = int(count[0])
    return edges[:m], weights[:m]


def _host(a):
    from . import _operands as ops
    return a.cpu().numpy() if ops.is_tensor(a) else np.asarray(a)


QUOTIENT_FIRST_EDGES = 4096  # places for cluster edges in graph_quotient's first ask; a second ask follows when there are more


def graph_quotient(rows, labels, n_labels, points=None, key=None, extra=None, weights=False, device=0):
    """The quotient of the graph the rows span under a labelling, on the GPU (``sc_graph_quotient``,
    ``csrc/graph_quotient.inl``): the clusters renumbered, their member counts and centres, and the edges
    of ``nx.quotient_graph`` with their weights -- everything :func:`distance_to_root_clusters` does behind its
    components.

    rows, extra : as for :func:`graph_distances`.
    labels : int32 ``[N]`` of the rows' kind, each below ``n_labels``; a negative label puts the node outside.
    key : ``None`` or int32 ``[N]``; points : ``None`` or float64 ``[N, 3]``; both of the rows' kind.
    weights : also sum the edge weights (the rows' values are then judged as :func:`graph_distances` judges them).

    Returns ``(cluster int32 [N], counts int32 [C], centers float64 [C, 3] | None, edges int32 [K, 2], edge_weights
    float64 [K] | None)``, NumPy arrays for arrays and CUDA tensors for tensors, by the rules Q1..Q4 of
    ``include/spacecarve.h``: labels with members are ranked by ``(least key of the members, smallest member)``;
    ``centers[c]`` is ``np.bincount(cluster, weights=coordinate) / count`` bit for bit; ``edges`` are the sorted pairs
    ``(a < b)`` of clusters joined by an arc; an edge's weight is the sum, in rising ``(i, j)``, over the undirected node
    pairs ``{i < j}`` that join the two clusters of the least weight of the pair's arcs -- ``nx.quotient_graph``'s
    ``weight`` up to summation order.  The first ask has room for ``QUOTIENT_FIRST_EDGES`` edges; when there are more the
    function asks a second time (rule Q5).  No nodes: empty results, no native call.  There is no CPU fallback."""
    from . import _native as nat, _operands as ops

    g = ops.graph_rows(rows, None, extra)
    lab = ops.node_ids(g, labels, "labels")
    n_labels = int(n_labels)
    if not 0 <= n_labels <= g.n:
        raise ValueError(f"n_labels must be 0 .. {g.n}, the node count")
    k = None if key is None else ops.node_ids(g, key, "key")
    pts = None
    if points is not None:
        if ops.is_tensor(points) != bool(g.on_device):
            raise ValueError("rows and points must be all arrays or all CUDA tensors")
        pts = ops.points(points, "points")
        if pts.n != g.n:
            raise ValueError("one point per node")
        if pts.on_device and pts.points.device != g.tdevice:
            raise ValueError("rows and points must be on one device")
    want_w = bool(weights)
    if g.on_device:
        import torch

        def empty(shape, dtype):
            return torch.empty(shape, dtype=getattr(torch, dtype), device=g.tdevice)
    else:
        def empty(shape, dtype):
            return np.empty(shape, dtype=dtype)
    cluster, counts = empty((g.n,), "int32"), empty((n_labels,), "int32")
    centers = None if pts is None else empty((n_labels, 3), "float64")
    nclusters, nedges = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    edges, edge_w = empty((0, 2), "int32"), empty((0,), "float64") if want_w else None
    if g.n:
        dev, stream = _graph_place(g, device)
        capacity = max(0, int(QUOTIENT_FIRST_EDGES))
        for _ in range(2):
            edges, edge_w = empty((capacity, 2), "int32"), empty((capacity,), "float64") if want_w else None
            _graph_call("sc_graph_quotient", g.n, g.offsets, g.row_len, g.index, g.values if want_w else 0, g.E, 1, g.extra,
                        g.extra_w if want_w else 0, g.M, lab.ptr, n_labels, 0 if k is None else k.ptr, 0 if pts is None else pts.ptr,
                        g.on_device, int(dev), ops.ptr_of(cluster), ops.ptr_of(counts) if n_labels else 0,
                        0 if centers is None or not n_labels else ops.ptr_of(centers), ops.ptr_of(edges) if capacity else 0,
                        ops.ptr_of(edge_w) if want_w and capacity else 0, capacity, nat.addr(nclusters), nat.addr(nedges), int(stream))
            if int(nedges[0]) <= capacity:
                break
            capacity = int(nedges[0])
    c, e = int(nclusters[0]), int(nedges[0])
    return cluster, counts[:c], None if centers is None else centers[:c], edges[:e], edge_w[:e] if want_w else None


def _bin_count(largest, bin_size):
    """``max(1, ceil(largest / bin_size))`` of the float64 quotient, refused where the bins, int32 keys, could not hold it."""
    top = float(largest) / bin_size  # an overflow gives inf
    if not math.isfinite(top) or math.ceil(top) - 1 > 2 ** 31 - 1:
        raise ValueError(f"bin_size {bin_size!r} is too small for distances up to {float(largest)!r}: the last bin's number must fit int32")
    return max(1, math.ceil(top))


def distance_to_root_clusters(points, rows, root_index, bin_size, extra=None, device=0, weights=False):
    """The clusters of the reference's ``distance_to_root_clusters`` (``proc3d.py:266-329``) as arrays: the nodes are cut
    into bins of their distance to the root, a cluster is a connected component of one bin, and two clusters are joined
    where an arc joins their nodes.  Everything but the bins is computed on the GPU: the distances
    (:func:`graph_distances`), the components (:func:`graph_components` with the bins as keys) and, in one call, the
    renumbering, the centres and the cluster edges (:func:`graph_quotient`); the bins are NumPy expressions (torch's for
    tensors).  With tensors nothing of the size of the nodes or the arcs crosses the bus: host points are uploaded once,
    device points are read in place.

    Returns ``(cluster, centers float64 [C, 3], cluster_edges int32 [K, 2], distances)``, with ``weights=True`` also
    ``edge_weights float64 [K]``; ``cluster`` (int32 ``[N]``) and ``distances`` (float64 ``[N]``) are NumPy arrays or CUDA
    tensors as the rows are, the others NumPy arrays:
      * ``n_bins = max(1, ceil(max finite d / bin_size))``, ``bin = min(floor(d / bin_size), n_bins - 1)``, ``-1`` for
        unreached nodes; a ``bin_size`` so small that the quotient overflows or ``n_bins - 1`` does not fit int32 raises
        ``ValueError``;
      * clusters are numbered by ``(bin, smallest member)``; unreached nodes have cluster ``-1``;
      * ``centers[c]`` is ``np.bincount(cluster, weights=coordinate) / count``;
      * ``cluster_edges`` are the unique pairs ``(a < b)`` of distinct clusters joined by an arc, sorted;
      * ``edge_weights[e]`` is the ``weight`` ``nx.quotient_graph`` gives the edge, up to summation order (rule Q4).

    Deviations: the reference function cannot be executed -- ``n = c[0]`` on a set raises ``TypeError`` on
    the first component (``proc3d.py:320``); its ``bisect`` cut is shifted by one sorted place (the first node of a bin
    falls into the bin before); it numbers components in set-iteration order.  Ours are the rules above."""
    from . import _operands as ops

    pts = ops.points(points, "points")
    g = ops.graph_rows(rows, pts.n, extra)
    bin_size = float(bin_size)
    if not (bin_size > 0.0 and bin_size != float("inf")):
        raise ValueError("bin_size must be positive and finite")
    d = graph_distances(rows, root_index, extra=extra, device=device)
    if g.on_device:
        import torch
        finite = torch.isfinite(d)
        n_bins = _bin_count(d[finite].max().item(), bin_size) if g.n else 1
        bins = torch.clamp(torch.floor(torch.where(finite, d, torch.zeros_like(d)) / bin_size), max=n_bins - 1).to(torch.int32)
        bins = torch.where(finite, bins, torch.full_like(bins, -1)).contiguous()
        xyz = pts.points if pts.on_device else torch.from_numpy(pts.points).to(g.tdevice)
    else:
        finite = np.isfinite(d)
        n_bins = _bin_count(d[finite].max(), bin_size) if g.n else 1
        bins = np.minimum(np.floor(np.where(finite, d, 0.0) / bin_size), n_bins - 1).astype(np.int32)
        bins = np.where(finite, bins, np.int32(-1)).astype(np.int32)
        xyz = _host(pts.points)
    labels, count = graph_components(rows, key=bins, extra=extra, device=device)
    cluster, _, centers, cluster_edges, edge_w = graph_quotient(rows, labels, count, points=xyz, key=bins, extra=extra, weights=weights,
                                                                device=device)
    out = (cluster, _host(centers), _host(cluster_edges), d)
    return out + (_host(edge_w),) if weights else out


def skeleton_from_distance_to_root_clusters(pcd, root_index, binsize, k, connect_all_points=True, device=0, weighted=False):
    """The XU method (``proc3d.py:392-426``; same signature, ``device`` and ``weighted`` added): the k-nearest-neighbour graph of the cloud
    (:func:`knn_points`), connected when ``connect_all_points`` (:func:`graph_components`, :func:`connect_edges`), its
    nodes clustered by distance to ``root_index`` (:func:`distance_to_root_clusters`), and the minimum spanning tree of
    the cluster graph.

    pcd : an array-like ``[n, 3]`` or a :class:`PointCloud`, uploaded once to ``device``; or a contiguous float64 CUDA
        tensor ``[n, 3]``, taken in place (``device`` is then the tensor's).  Every step runs device to device on torch's
        current stream; what comes home is ``cluster [n]``, the centres, the cluster edges and their weights.

    Returns ``(tree, cluster_values)``: ``tree`` is ``nx.minimum_spanning_tree`` of the ``networkx.Graph`` whose nodes
    ``0..C-1`` carry ``center`` and whose edges are the cluster edges in sorted order; ``cluster_values`` is the dict
    ``{node: cluster}``, unreached nodes absent as in the reference.  Raises ``ImportError`` without networkx.

    weighted : give every cluster edge its ``weight``, the sum of the weights of the node edges between the two clusters
        (:func:`graph_quotient`, rule Q4), before ``nx.minimum_spanning_tree``: the reference's tree.

    Deviation, for the default only: the reference's ``quotient_graph`` weights a cluster edge with the sum of the edge
    weights between the two clusters, added in set-iteration order; without ``weighted`` ours carry no weight (every edge
    counts 1), so the tree is Kruskal's over the sorted pairs.  With ``weighted`` the weights are the reference's up to
    summation order.  The deviations of :func:`distance_to_root_clusters` and :func:`connect_edges` hold here too."""
    try:
        import networkx as nx
    except ImportError as e:
        raise ImportError("skeleton_from_distance_to_root_clusters needs networkx (distance_to_root_clusters returns the clusters as "
                          "arrays without it)") from e
    from . import _operands as ops

    pts = ops.points(pcd, "points")
    if pts.on_device:
        xyz = pts.points
    else:  # the one upload: every step below reads and writes device memory
        import torch
        xyz = torch.from_numpy(pts.points).to(f"cuda:{int(device)}")
    rows = knn_points(xyz, xyz, int(k))
    extra = None
    if connect_all_points and pts.n:
        labels, count = graph_components(rows)
        if count > 1:
            extra = connect_edges(xyz, labels, root_index, n_labels=count)
    got = distance_to_root_clusters(xyz, rows, root_index, binsize, extra=extra, weights=bool(weighted))
    cluster, centers, cluster_edges, edge_w = _host(got[0]), got[1], got[2], got[4] if weighted else None
    g = nx.Graph()
    for c in range(len(centers)):
        g.add_node(c, center=centers[c])
    if weighted:
        g.add_weighted_edges_from((int(a), int(b), float(w)) for (a, b), w in zip(cluster_edges.tolist(), edge_w.tolist()))
    else:
        g.add_edges_from((int(a), int(b)) for a, b in cluster_edges.tolist())
    return nx.minimum_spanning_tree(g), {int(v): int(c) for v, c in enumerate(cluster.tolist()) if c >= 0}
