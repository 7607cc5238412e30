"""The ``VoxelsEvaluation`` and ``Segmentation2DEvaluation`` task logic of the reference
(``plant3dvision/tasks/evaluation.py:356-477``, ``plant3dvision/metrics.py:275-381``) around the device counting
passes (``metrics.voxel_confusion``, ``metrics.compare_mask_stacks``), and the ``PointCloudEvaluation`` and
``SegmentedPointCloudEvaluation`` logic (``tasks/evaluation.py:278-353``) around the device's nearest-point search
(``metrics.point_cloud_registration_fitness``, ``metrics.CompareSegmentedPointClouds``).

As with ``tasks/proc2d.py::masks_run`` and ``tasks/proc3d.py::organ_segmentation_run``, the tasks' *logic* is plain
functions without luigi / plantdb.  The ground-truth producers and the matplotlib figures of the reference stay where
they are; INTEGRATION.md has the lines a maintainer of the reference puts into the two tasks.
"""
import logging

import numpy as np

logger = logging.getLogger(__name__)


def voxels_evaluation_run(voxels, groundtruths, confusion_fn=None):
    """The ``histograms`` of ``VoxelsEvaluation.evaluate`` (tasks/evaluation.py:428-477).

    voxels, groundtruths : ``{label: volume}`` as ``read_npz`` gives them (:425-426); the classes are the ground
        truth's keys, ``"background"`` takes part in the arg-max and is not evaluated (:438-439).
    confusion_fn : ``metrics.voxel_confusion`` by default; an argument only, the CPU tests pass a function of theirs.

    Returns ``{label: {"tp", "fp", "tn", "fn"}}``."""
    if confusion_fn is None:  # the product: the HIP kernel
        from ..metrics import voxel_confusion as confusion_fn
    return confusion_fn(voxels, groundtruths)


def _matching(files, label, shot_id):
    return [f for f in files if f.get_metadata("channel") == label and f.get_metadata("shot_id") == shot_id]


def segmentation2d_evaluation_run(groundtruth_files, prediction_files, labels, dilation_amount=0, compare_fn=None):
    """``Segmentation2DEvaluation.evaluate`` (tasks/evaluation.py:386-396) over ``CompareMaskFilesets``
    (metrics.py:275-381) without luigi / plantdb.

    groundtruth_files, prediction_files : lists of file-like objects (``.id``, ``.get_metadata(key)`` with
        ``channel`` and ``shot_id``; pixels via ``cl.read_image``): what the two filesets' ``get_files()`` return.
    labels : the channels to evaluate; must not be empty (:389-391).
    compare_fn : ``metrics.compare_mask_stacks`` by default; an argument only, the CPU tests pass a function of theirs.
        Called once per label and picture size as ``compare_fn(groundtruth_stack, prediction_stack, dilation_amount)``.

    Returns ``CompareMaskFilesets.results``: ``{"evaluation-results": {prediction file id: metrics}, label: metrics}``,
    ``metrics`` the ``SetMetrics.as_dict()`` of the file or, summed over its files, of the label.  A labelled file
    without exactly one partner on the other side raises the reference's ``ValueError`` (:317-339)."""
    from ..cl import read_image
    from ..metrics import MaskEvaluator, SetMetrics

    labels = list(labels)
    if len(labels) == 0:
        raise ValueError("The labels parameter is empty. Not continuing because the results may not be what you expected. "
                         "Please add 'labels = ['...', '...']' to the Segmentation2DEvaluation section in the config file.")
    if compare_fn is None:  # the product: the HIP kernels
        from ..metrics import compare_mask_stacks as compare_fn
    groundtruth_files, prediction_files = list(groundtruth_files), list(prediction_files)
    for mine, others, what in ((groundtruth_files, prediction_files, "Missing file in predictions"),
                               (prediction_files, groundtruth_files, "Missing file in groundtruth")):
        for fi in mine:
            label, shot_id = fi.get_metadata("channel"), fi.get_metadata("shot_id")
            if label in labels and len(_matching(others, label, shot_id)) != 1:
                logger.warning(f"{what}: label '{label}', shot_id '{shot_id}'")
                raise ValueError(what)
    results = {"evaluation-results": {}}
    for label in labels:
        preds = [f for f in prediction_files if f.get_metadata("channel") == label]
        pairs = []
        for pf in preds:
            gf = _matching(groundtruth_files, label, pf.get_metadata("shot_id"))[0]  # exactly one: checked above
            g, p = np.asarray(read_image(gf)), np.asarray(read_image(pf))
            if g.shape != p.shape:
                raise ValueError("The groundtruth and prediction are different in size: %s vs %s" % (str(g.shape), str(p.shape)))
            if g.ndim != 2 or p.ndim != 2:
                raise ValueError(f"masks must be 2-D pictures (file '{pf.id}' has shape {p.shape})")
            pairs.append((g, p))
        groups = {}  # pictures of one size make one device call, in file order
        for q, (g, p) in enumerate(pairs):
            groups.setdefault(g.shape, []).append(q)
        counts = [None] * len(pairs)
        for members in groups.values():
            got = np.asarray(compare_fn(np.stack([pairs[q][0] for q in members]), np.stack([pairs[q][1] for q in members]),
                                        dilation_amount))
            for k, q in enumerate(members):
                counts[q] = [int(x) for x in got[k]]
        metrics_label = SetMetrics(MaskEvaluator(dilation_amount))
        for pf, (tp, fn, tn, fp) in zip(preds, counts):
            metrics_file = SetMetrics(MaskEvaluator(dilation_amount))
            metrics_file._update_metrics(tp, fn, tn, fp)
            results["evaluation-results"][pf.id] = metrics_file.as_dict()
            metrics_label += metrics_file
        results[label] = metrics_label.as_dict()
    return results


def _points_of(cloud):
    return cloud.points if not isinstance(cloud, np.ndarray) and hasattr(cloud, "points") else cloud


def _subset(points, idx):
    """The rows ``idx`` of a NumPy array or of a CUDA tensor (which stays on its device)."""
    from .._operands import is_tensor
    if is_tensor(points):
        import torch
        return points[torch.as_tensor(idx, dtype=torch.long, device=points.device)].contiguous()
    return np.asarray(points, dtype=np.float64).reshape(-1, 3)[idx]


def point_cloud_evaluation_run(source, target, labels=None, labels_gt=None, max_distance=2, task_id=None, registration_fn=None):
    """``PointCloudEvaluation.evaluate`` (tasks/evaluation.py:319-353) without luigi / plantdb.

    source, target : the evaluated cloud and the ground truth, as ``proc3d.nearest_points`` takes them.
    labels, labels_gt : one name per point of ``source`` / ``target``, or ``labels = None`` for the whole clouds only.
    registration_fn : ``metrics.point_cloud_registration_fitness`` by default; an argument only, the CPU tests pass a
        function of theirs.  Called as ``registration_fn(source, target, max_distance)`` -> ``(fitness, inlier_rmse)``.

    Returns ``{"id": task_id, "all": {...}, label: {"fitness", "inlier_rmse"}}``: a label per name of
    ``set(labels_gt)``; a name without a ground-truth point is skipped (:341-342), one without a source point gives
    0.0 / 0.0 (what open3d returns for an empty source)."""
    if registration_fn is None:  # the product: the HIP kernels
        from ..metrics import point_cloud_registration_fitness as registration_fn
    fitness, rmse = registration_fn(source, target, max_distance)
    out = {"id": task_id, "all": {"fitness": fitness, "inlier_rmse": rmse}}
    if labels is not None:
        src, tgt = _points_of(source), _points_of(target)
        for name in set(labels_gt):
            idx = [i for i in range(len(labels)) if labels[i] == name]
            idx_gt = [i for i in range(len(labels_gt)) if labels_gt[i] == name]
            if len(idx_gt) == 0:
                continue
            logger.debug("label : %s, gt points: %i, pcd points: %i", name, len(idx_gt), len(idx))
            fitness, rmse = registration_fn(_subset(src, idx), _subset(tgt, idx_gt), max_distance) if idx else (0.0, 0.0)
            out[name] = {"fitness": fitness, "inlier_rmse": rmse}
    return out


def segmented_point_cloud_evaluation_run(prediction, labels, groundtruth, labels_gt, compare_fn=None):
    """``SegmentedPointCloudEvaluation.evaluate`` (tasks/evaluation.py:278-290) without luigi / plantdb: the
    ``results`` of ``CompareSegmentedPointClouds(groundtruth, labels_gt, prediction, labels)``.  Empty ``labels``
    raise the reference's ``ValueError`` (:284-286).

    compare_fn : ``metrics.CompareSegmentedPointClouds`` by default; an argument only, the CPU tests pass a function
        of theirs.  Called as ``compare_fn(groundtruth, labels_gt, prediction, labels)``; its ``.results`` is returned."""
    if len(labels) == 0:
        raise ValueError("The labels parameter is empty. No continuing because the results may not be what expected.")
    if compare_fn is None:  # the product: the HIP kernels
        from ..metrics import CompareSegmentedPointClouds as compare_fn
    return compare_fn(groundtruth, labels_gt, prediction, labels).results
