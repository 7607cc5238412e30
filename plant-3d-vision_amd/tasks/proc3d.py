"""The ``OrganSegmentation`` task logic of the reference (``plant3dvision/tasks/proc3d.py:419-521``) around the
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
