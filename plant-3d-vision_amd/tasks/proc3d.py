"""The ``PointCloud`` task logic of the reference (``plant3dvision/tasks/proc3d.py:66-136``) around the device
class selection and ``vol2pcd`` (``proc3d.select_classes``, ``proc3d.vol2pcd_class``; ``point_cloud_run``, at the end
of this file), and the ``OrganSegmentation`` task logic (``plant3dvision/tasks/proc3d.py:419-521``) around the
device clustering (``proc3d.cluster_dbscan``).

As with ``tasks/proc2d.py::masks_run``, the task's *logic* -- one cloud per label, the stem kept whole, every other
label split into its DBSCAN clusters, the noise dropped, the file names -- is a plain function,
``organ_segmentation_run``, without luigi / plantdb.  INTEGRATION.md has the lines a maintainer of the reference puts
into ``OrganSegmentation.run``.

PARITY UNPINNED: open3d's ``cluster_dbscan`` is not available here; ``proc3d.cluster_dbscan``
restates it.
"""
import logging

import numpy as np

logger = logging.getLogger(__name__)

#: parameter defaults of the reference task (tasks/proc3d.py:458-459)
ORGAN_SEGMENTATION_DEFAULTS = dict(eps=2.0, min_points=5)


def organ_segmentation_run(points, labels, eps=2.0, min_points=5, cluster_fn=None):
    """The loop of ``OrganSegmentation.run`` without luigi / plantdb (tasks/proc3d.py:489-521).

    points : ``[P, 3]`` array-like, a ``proc3d.PointCloud`` or anything with ``.points`` (the labelled cloud).
    labels : the P semantic labels (the ``labels`` metadata of the ``SegmentedPointCloud`` file).
    cluster_fn : ``proc3d.cluster_dbscan`` by default; an argument only, the CPU tests pass a function of theirs.
        Called as ``cluster_fn(points_of_the_label, eps, min_points)``; returns one id per point, ``-1`` for noise.

    Returns ``[(name, indices, {"label": label}), ...]``: ``name`` the file the reference creates
    (``"%s_%03d" % (label, i)``, :502 and :519), ``indices`` the points of that part as indices into the INPUT cloud
    (ascending), the dictionary the metadata it sets (:504, :521).  Labels come in the order of their first appearance
    -- the reference iterates a Python ``set`` (:496-498), whose order is arbitrary; clusters in the order of their ids.
    ``stem`` is one part, ``stem_000``, made of all its points (:501-505); noise is dropped (:516-517).
    """
    if cluster_fn is None:  # the product: the HIP kernels
        from ..proc3d import cluster_dbscan as cluster_fn
    if not isinstance(points, np.ndarray) and hasattr(points, "points"):
        points = points.points
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    labels = list(labels)
    if len(labels) != pts.shape[0]:
        raise ValueError("one label per point")
    members = {}  # label -> indices, labels in order of first appearance
    for q, label in enumerate(labels):
        members.setdefault(label, []).append(q)
    parts = []
    for label, idx in members.items():
        idx = np.asarray(idx, dtype=np.int64)
        logger.info(f"Found {idx.size} point for, label '{label}'.")
        if label == "stem":  # excluded from the clustering: one organ
            parts.append(("%s_%03d" % (label, 0), idx, {"label": label}))
            continue
        clustered = np.asarray(cluster_fn(np.ascontiguousarray(pts[idx]), eps, min_points))
        ids = np.unique(clustered)
        logger.info(f"Found {len(ids)} clusters in the point cloud!")
        for i in ids:
            if i == -1:  # outliers
                continue
            parts.append(("%s_%03d" % (label, i), idx[clustered == i], {"label": label}))
    return parts


#: parameter defaults of the reference task (tasks/proc3d.py:60-64)
POINT_CLOUD_DEFAULTS = dict(level_set_value=1.0, background_prior=1.0, min_contrast=10.0, min_score=0.2)

#: the label colours of the reference (tasks/config.py:7-13)
POINT_CLOUD_COLORS = {
    "stem": [1.0, 0.0, 0.0],
    "flower": [1.0, 1.0, 0.0],
    "fruit": [1.0, 0.0, 1.0],
    "pedicel": [1.0, 1.0, 1.0],
    "leaf": [0.0, 1.0, 0.0],
}


def point_cloud_run(voxels, origin, voxel_size, level_set_value=1.0, background_prior=1.0, min_contrast=10.0, min_score=0.2,
                    colors=None, random_color=None, select_fn=None, vol2pcd_fn=None, device=0):
    """Both branches of ``PointCloud.run`` without luigi / plantdb (tasks/proc3d.py:80-136).

    voxels : a dict ``{label: volume}`` -- what ``io.read_npz`` gives the task -- or a single volume.  A dict of more
        than one key is the multiclass branch (:80-129); a single array or a dict of one key the single-volume branch
        (:131-136).  The volumes of the multiclass branch are NumPy arrays, or CUDA torch tensors (``proc3d.
        select_classes``): the winner volume then stays on the device and only points and normals come back.
    origin, voxel_size : the ``origin`` and ``voxel_size`` metadata of the input file.
    colors : ``{label: [r, g, b]}``, ``POINT_CLOUD_COLORS`` by default (``PointCloudColorConfig().colors``, :104).
    random_color : called without arguments once per label that ``colors`` lacks, ``np.random.rand(3)`` by default
        (:122).
    select_fn, vol2pcd_fn : ``proc3d.select_classes`` and ``proc3d.vol2pcd`` / ``proc3d.vol2pcd_class`` by default;
        arguments only, the CPU tests pass functions of theirs.  Called as ``select_fn(voxels, background_prior,
        min_contrast, min_score)`` -> ``(winner, labels, counts)`` and ``vol2pcd_fn(volume, origin, voxel_size,
        level_set_value, index)`` -> an object with ``points`` and ``normals``: ``index`` is ``None`` for a plain
        volume, else ``volume`` is the winner volume and the cloud is that of ``winner == index``.

    Returns ``(cloud, metadata)``.  Multiclass: the clouds of the classes other than ``'background'`` in key order, one
    after the other (:125), each point coloured as its class (:118-124); ``metadata = {"labels": point_labels}``, one
    label per point (:126, :129).  A class that owns no voxel contributes nothing (``vol2pcd`` of an empty
    volume is an empty cloud here).  Single volume: ``vol2pcd``'s cloud, ``metadata = {"voxel_size": voxel_size}``
    (:134-136).
    """
    from .. import proc3d

    if vol2pcd_fn is None:  # the product: the HIP kernels
        def vol2pcd_fn(volume, origin, voxel_size, level_set_value, index):
            if index is None:
                return proc3d.vol2pcd(volume, origin, voxel_size, level_set_value, device=device)
            return proc3d.vol2pcd_class(volume, index, origin, voxel_size, level_set_value, device=device, as_open3d=False)
    if isinstance(voxels, dict) and len(voxels) == 1:  # :71-73
        voxels = voxels[list(voxels.keys())[0]]
    if not isinstance(voxels, dict):
        voxel_size = float(voxel_size)
        return vol2pcd_fn(voxels, origin, voxel_size, level_set_value, None), {"voxel_size": voxel_size}

    if select_fn is None:
        def select_fn(voxels, background_prior, min_contrast, min_score):
            return proc3d.select_classes(voxels, background_prior, min_contrast, min_score, device=device)
    if colors is None:
        colors = POINT_CLOUD_COLORS
    if random_color is None:
        def random_color():
            return np.random.rand(3)
    origin = np.array(origin)
    voxel_size = float(voxel_size)
    winner, labels, counts = select_fn(voxels, background_prior, min_contrast, min_score)
    points, normals, cols, point_labels = [], [], [], []
    for i, label in enumerate(labels):
        logger.debug(f"label = {label}")
        if label == "background":
            continue
        rgb = np.asarray(colors[label] if label in colors else random_color(), dtype=np.float64).reshape(3)
        if int(counts[i]) == 0:
            continue
        out = vol2pcd_fn(winner, origin, voxel_size, level_set_value, i)
        n = len(out.points)
        points.append(np.asarray(out.points, dtype=np.float64).reshape(n, 3))
        normals.append(np.asarray(out.normals, dtype=np.float64).reshape(n, 3))
        cols.append(np.tile(rgb, (n, 1)))
        point_labels = point_labels + [label] * n
    empty = np.zeros((0, 3))
    cloud = proc3d._make_cloud(np.concatenate(points + [empty]), np.concatenate(normals + [empty]), np.concatenate(cols + [empty]))
    return cloud, {"labels": point_labels}
