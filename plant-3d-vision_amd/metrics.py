"""The set metrics of the reference (``plant3dvision/metrics.py:98-272``) over the device counting passes
(``sc_eval_masks`` / ``sc_eval_voxels``, ``csrc/evaluate.hip``).

``SetEvaluator``, ``SetMetrics``, ``MaskEvaluator`` and ``CompareMasks`` keep the reference's names, signatures and
results; ``MaskEvaluator.evaluate`` counts on the GPU.  ``compare_mask_stacks`` is the batched form a fileset
comparison calls once per label, ``voxel_confusion`` the counting of ``VoxelsEvaluation.evaluate``
(``tasks/evaluation.py:421-477``).

``chamfer_distance``, ``point_cloud_registration_fitness`` (metrics.py:16-95) and ``CompareSegmentedPointClouds``
(:384-519) rest on the nearest-point search of ``csrc/nearest.hip`` (``proc3d.nearest_points``; parity
with open3d unpinned).  The mesh metrics of the reference's module are not here.
There is no CPU fallback: without the library or a gfx950 device the calls raise.
"""
from abc import ABC, abstractmethod

import numpy as np


class SetEvaluator(ABC):
    """Domain-specific comparison of a ground truth with a prediction: ``evaluate`` returns ``(tp, fn, tn, fp)``."""

    @abstractmethod
    def evaluate(self, groundtruth, prediction):
        pass


class SetMetrics(ABC):
    """Confusion counts of arrays compared as sets, summed over ``add`` / ``+``; precision, recall and the mean of the
    per-comparison IoUs (metrics.py:105-204).  A ratio whose denominator is zero is ``None``."""

    def __init__(self, evaluator, groundtruth=None, prediction=None):
        self.evaluator = evaluator
        self.tp = 0
        self.fn = 0
        self.tn = 0
        self.fp = 0
        self._miou = 0
        self._miou_count = 0
        if groundtruth is not None and prediction is not None:
            self._compare(groundtruth, prediction)

    def __add__(self, other):
        self._update_metrics(other.tp, other.fn, other.tn, other.fp)  # (the other's totals count as ONE comparison)
        return self

    def add(self, groundtruth, prediction):
        self._compare(groundtruth, prediction)

    def __str__(self):
        return str(self.as_dict())

    def as_dict(self):
        return {"tp": self.tp, "fn": self.fn, "tn": self.tn, "fp": self.fp, "precision": self.precision(),
                "recall": self.recall(), "miou": self.miou()}

    def _compare(self, groundtruth, prediction):
        tp, fn, tn, fp = self.evaluator.evaluate(groundtruth, prediction)
        self._update_metrics(tp, fn, tn, fp)

    def _update_metrics(self, tp, fn, tn, fp):
        self.tp += tp
        self.fn += fn
        self.tn += tn
        self.fp += fp
        if (tp + fp + fn) != 0:
            self._miou += tp / (tp + fp + fn)
            self._miou_count += 1

    def precision(self):
        return self.tp / (self.tp + self.fp) if (self.tp + self.fp) != 0 else None

    def recall(self):
        return self.tp / (self.tp + self.fn) if (self.tp + self.fn) != 0 else None

    def miou(self):
        return self._miou / self._miou_count if self._miou_count > 0 else None


def _picture(a, what):
    a = np.asarray(a)
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError(f"{what} must be a 2-D uint8 picture (got {a.dtype}, shape {a.shape}): the device route "
                         f"takes masks only")
    return a


class MaskEvaluator(SetEvaluator):
    """``MaskEvaluator`` of the reference (metrics.py:242-272) on the GPU: the prediction's non-zero pixels, dilated
    ``dilation_amount`` times by ``scipy.ndimage.binary_dilation``'s default cross, against the ground truth's
    non-zero pixels.  Pictures are 2-D uint8 (or bool); anything else -- the reference would dilate a colour picture
    across its channels -- raises ``ValueError``."""

    def __init__(self, dilation_amount=0, device=0):
        self.dilation_amount = dilation_amount
        self.device = device

    def evaluate(self, groundtruth, prediction):
        self._assert_same_size(groundtruth, prediction)
        gt, pr = _picture(groundtruth, "groundtruth"), _picture(prediction, "prediction")
        c = compare_mask_stacks(gt[None], pr[None], self.dilation_amount, device=self.device)[0]
        return int(c[0]), int(c[1]), int(c[2]), int(c[3])

    def _assert_same_size(self, groundtruth, prediction):
        if np.shape(groundtruth) != np.shape(prediction):
            raise ValueError("The groundtruth and prediction are different in size: %s vs %s"
                             % (str(np.shape(groundtruth)), str(np.shape(prediction))))


class CompareMasks(SetMetrics):
    """The metrics of one ground-truth mask against one predicted mask (metrics.py:207-239)."""

    def __init__(self, groundtruth, prediction, dilation_amount=0):
        super(CompareMasks, self).__init__(MaskEvaluator(dilation_amount), groundtruth, prediction)


def compare_mask_stacks(groundtruths, predictions, dilation_amount=0, device=0):
    """``MaskEvaluator.evaluate`` for ``n`` pictures in one call (``sc_eval_masks``).

    groundtruths, predictions : uint8 (or bool) ``[n, H, W]``, both NumPy arrays or both contiguous CUDA torch tensors
        of one device; tensors are read in place on torch's current stream.
    Returns the NumPy int64 array ``[n, 4]`` of ``tp, fn, tn, fp`` (the reference's order)."""
    from . import _native as nat
    from ._operands import is_tensor

    k = int(dilation_amount)
    if k < 0:
        raise ValueError("dilation_amount must not be negative")
    if is_tensor(groundtruths) != is_tensor(predictions):
        raise ValueError("ground truths and predictions must both be NumPy arrays or both CUDA tensors")
    nat.backend()
    if is_tensor(groundtruths):
        import torch
        gt, pr = groundtruths, predictions
        for t in (gt, pr):
            if t.dtype not in (torch.uint8, torch.bool) or t.dim() != 3 or not t.is_cuda or not t.is_contiguous():
                raise ValueError("device masks must be contiguous uint8 CUDA tensors [n, H, W]")
        if tuple(gt.shape) != tuple(pr.shape) or gt.device != pr.device:
            raise ValueError("The groundtruth and prediction are different in size: %s vs %s"
                             % (str(tuple(gt.shape)), str(tuple(pr.shape))))
        n, H, W = (int(s) for s in gt.shape)
        dev = gt.device.index
        gptr, pptr, on_dev, stream = gt.data_ptr(), pr.data_ptr(), 1, torch.cuda.current_stream(dev).cuda_stream
    else:
        gt, pr = np.asarray(groundtruths), np.asarray(predictions)
        if gt.shape != pr.shape:
            raise ValueError("The groundtruth and prediction are different in size: %s vs %s" % (str(gt.shape), str(pr.shape)))
        keep = []
        for a in (gt, pr):
            if a.dtype == np.bool_:
                a = a.view(np.uint8)
            if a.ndim != 3 or a.dtype != np.uint8:
                raise ValueError("masks must be uint8 [n, H, W]")
            keep.append(np.ascontiguousarray(a))
        n, H, W = keep[0].shape
        dev, gptr, pptr, on_dev, stream = int(device), nat.addr(keep[0]), nat.addr(keep[1]), 0, 0
    counts = np.zeros((max(n, 1), 4), dtype=np.int64)
    if n == 0:
        return counts[:0]
    if H == 0 or W == 0:
        raise ValueError("pictures must not be empty")
    nat.unit_call("sc_eval_masks", gptr, pptr, on_dev, n, H, W, min(k, 2 ** 31 - 1), dev, int(stream), nat.addr(counts))
    return counts


def set_chunk_bytes(nbytes):
    """Largest device work buffer a call with host volumes or host pictures may take (``sc_eval_set_chunk_bytes``;
    default 256 MiB, ``0`` restores it): larger inputs go through in x-slabs / batches of pictures, same counts."""
    from . import _native as nat
    nat.backend().call("sc_eval_set_chunk_bytes", int(nbytes))


def voxel_confusion(voxels, groundtruths, background="background", min_contrast=10.0, projections=False, device=0):
    """The counting of ``VoxelsEvaluation.evaluate`` (tasks/evaluation.py:428-477) on the GPU (``sc_eval_voxels``).

    voxels, groundtruths : dicts ``{label: volume}``.  The classes are the ground truth's keys in their order, as in
        the reference; every one of them must be in ``voxels``.  Predictions share one shape ``(nx, ny, nz)``, ground
        truths one shape with every axis at least as long (only their corner ``[0:nx, 0:ny, 0:nz]`` is read).  All
        volumes are NumPy arrays or all contiguous CUDA torch tensors of one device (read in place on torch's current
        stream).  Predictions are float32 or float64, ground truths float32, float64 or uint8; bool is viewed as
        uint8; NumPy arrays of other dtypes are converted to float64 on the host.  Comparisons are in float64.
    background : the label that is not evaluated (it still takes part in the arg-max), or ``None``.
    min_contrast : a voxel predicts its arg-max class only if that value exceeds ``min_contrast`` times the greatest
        other one; the reference hard-codes 10.

    Returns ``{label: {"tp", "fp", "tn", "fn"}}`` (Python ints) for every label but the background -- the reference's
    ``histograms`` -- and with ``projections=True`` the pair ``(that, {label: uint8 [ny, nz]})``: 1 where some x of
    the column predicts the label (``prediction_c.max(0)``, :455)."""
    from . import _native as nat, _operands as ops

    labels = list(groundtruths.keys())
    L = len(labels)
    if L < 2:
        raise ValueError("at least two classes are needed (the reference fails with one: its max runs over nothing)")
    if L > 32:
        raise ValueError("at most 32 classes")
    for label in labels:
        if label not in voxels:
            raise ValueError(f"label '{label}' of the ground truth is missing from the voxels")
    refused = "device voxels must be float32 or float64, device ground truths float32, float64, uint8 or bool"
    floats = (nat.SC_EVAL_F32, nat.SC_EVAL_F64)
    pred, gt = [voxels[label] for label in labels], [groundtruths[label] for label in labels]
    if len({ops.is_tensor(v) for v in pred + gt}) > 1:  # (across both stacks, before either is judged)
        raise ValueError("volumes must be all NumPy arrays or all CUDA tensors")
    p = ops.class_stack(pred, "voxels", floats, refused, device)
    g = ops.class_stack(gt, "ground truths", floats + (nat.SC_EVAL_U8,), refused, device)
    ops.same([p.tdevice, g.tdevice], "devices")
    bg = labels.index(background) if background in labels else -1
    pshape, gshape = p.shape, g.shape
    if any(gs < ps for gs, ps in zip(gshape, pshape)):
        raise ValueError(f"ground truth {gshape} smaller than the prediction {pshape}")
    if min(pshape) < 1:
        raise ValueError("volumes must not be empty")
    counts = np.zeros((L, 4), dtype=np.int64)
    proj = np.zeros((L, pshape[1], pshape[2]), dtype=np.uint8) if projections else None
    nat.unit_call("sc_eval_voxels", nat.addr(p.table), p.code, nat.addr(g.table), g.code, L, pshape[0], pshape[1], pshape[2],
                  gshape[0], gshape[1], gshape[2], bg, float(min_contrast), p.on_device, p.device, p.stream,
                  nat.addr(counts), nat.addr(proj) if projections else 0)
    out = {label: {"tp": int(counts[q, 0]), "fp": int(counts[q, 1]), "tn": int(counts[q, 2]), "fn": int(counts[q, 3])}
           for q, label in enumerate(labels) if q != bg}
    if projections:
        return out, {label: proj[q] for q, label in enumerate(labels) if q != bg}
    return out


# ---- the cloud metrics ---------------------------------------------------------------------------------
def _n_points(cloud):
    if not isinstance(cloud, np.ndarray) and hasattr(cloud, "points"):
        cloud = cloud.points
    return int(cloud.shape[0]) if hasattr(cloud, "shape") else len(cloud)


def chamfer_distance(ref_pcd, flo_pcd, device=0):
    """The symmetric chamfer distance of the reference (metrics.py:16-55): the mean distance from every point of
    ``ref_pcd`` to its nearest point of ``flo_pcd`` plus the same the other way.  Clouds as ``proc3d.nearest_points``
    takes them; only the sums leave the device (rule N6 of DESIGN.md 16).  An empty cloud raises ``ValueError`` (the
    reference divides by zero)."""
    from .proc3d import nearest_sums

    na, nb = _n_points(ref_pcd), _n_points(flo_pcd)
    if na == 0 or nb == 0:
        raise ValueError("chamfer_distance needs two clouds that are not empty")
    _, _, sa = nearest_sums(ref_pcd, flo_pcd, None, device=device)
    _, _, sb = nearest_sums(flo_pcd, ref_pcd, None, device=device)
    return sa / na + sb / nb


def point_cloud_registration_fitness(ref_pcd, flo_pcd, max_distance=2, device=0):
    """``(fitness, inlier_rmse)`` of open3d's ``evaluate_registration(ref_pcd, flo_pcd, max_distance)``
    (metrics.py:58-95): every point of ``ref_pcd`` -- the source -- searches ``flo_pcd``; a point is matched iff its
    nearest target is closer than ``max_distance`` (strict, rule N3); ``fitness`` = matched / points of the source,
    ``inlier_rmse`` = sqrt(sum d2 / matched); both 0.0 when nothing is matched or the source is empty, which is what
    open3d returns without correspondences."""
    from .proc3d import nearest_sums

    Q = _n_points(ref_pcd)
    n, s2, _ = nearest_sums(ref_pcd, flo_pcd, max_distance, device=device)
    if Q == 0 or n == 0:
        return 0.0, 0.0
    return n / Q, float(np.sqrt(s2 / n))


def _device_tables(source, source_ids, target, target_ids, n_labels, device=0):
    """The product's table function: ``counts[a, b]`` = source points of label id ``a`` whose nearest target point has
    label id ``b``, by ``sc_nearest`` and ``sc_nearest_confusion``.  With CUDA tensors as points the indices stay on
    the device and the label ids are sent there."""
    from ._operands import is_tensor
    from .proc3d import nearest_confusion, nearest_points

    index, _ = nearest_points(source, target, None, device=device)
    if is_tensor(index):
        import torch
        source_ids = torch.from_numpy(np.ascontiguousarray(source_ids, dtype=np.int32)).to(index.device)
        target_ids = torch.from_numpy(np.ascontiguousarray(target_ids, dtype=np.int32)).to(index.device)
    return nearest_confusion(index, source_ids, target_ids, n_labels, device=device)


class CompareSegmentedPointClouds:
    """``CompareSegmentedPointClouds`` of the reference (metrics.py:384-519): ``results`` holds, for each direction
    (``'groundtruth-to-prediction'``, ``'prediction-to-groundtruth'``) and each label of ``set(groundtruth_labels)``,
    ``tp, fp, tn, fn, precision, recall, iou``, and ``'miou'``: per label the mean of the two directions' IoUs or
    ``None``.  The reference's naming is kept: ``fp`` = the source point has the label and its nearest target point
    has not, ``fn`` the reverse.  A label only the prediction has counts as "other".  A ratio with a zero denominator
    is ``None``.

    The reference asks a ``KDTreeFlann`` once per point; here each direction is one nearest-point search and one
    ``L x L`` table on the GPU, and everything else follows from the two tables with the reference's expressions.
    ``tables_fn(source, source_ids, target, target_ids, L)`` is an argument only: the CPU tests pass the checker's."""

    def __init__(self, groundtruth, groundtruth_labels, prediction, prediction_labels, device=0, tables_fn=None):
        self.groundtruth = groundtruth
        self.prediction = prediction
        self.groundtruth_labels = groundtruth_labels
        self.prediction_labels = prediction_labels
        self.unique_labels = set(groundtruth_labels)
        self.device = device
        self.results = {}
        self._assure_sizes()
        if tables_fn is None:  # the product: the HIP kernels
            def tables_fn(*args):
                return _device_tables(*args, device=device)
        self._tables_fn = tables_fn
        self._evaluate()

    def _assure_sizes(self):
        self.assure_size(self.groundtruth, self.groundtruth_labels)
        self.assure_size(self.prediction, self.prediction_labels)

    def assure_size(self, pointcloud, labels):
        num_points = _n_points(pointcloud)
        if num_points != len(labels):
            raise ValueError("The number of points should be the same as the number of "
                             f"labels (#points({num_points}) != #labels({len(labels)}))")

    def _evaluate(self):
        names = list(self.unique_labels)  # ids 0..G-1; every other name is id G, "other"
        ids = {name: k for k, name in enumerate(names)}
        other = len(names)
        gt_ids = np.array([ids.get(name, other) for name in self.groundtruth_labels], dtype=np.int32)
        pr_ids = np.array([ids.get(name, other) for name in self.prediction_labels], dtype=np.int32)
        L = other + (1 if (pr_ids == other).any() else 0)
        gt_pts = self.groundtruth.points if hasattr(self.groundtruth, "points") else self.groundtruth
        pr_pts = self.prediction.points if hasattr(self.prediction, "points") else self.prediction
        if L == 0:  # no ground-truth point at all: nothing to evaluate
            self.results = {"groundtruth-to-prediction": {}, "prediction-to-groundtruth": {}, "miou": {}}
            return
        self.results["groundtruth-to-prediction"] = self._compare(names, self._tables_fn(gt_pts, gt_ids, pr_pts, pr_ids, L))
        self.results["prediction-to-groundtruth"] = self._compare(names, self._tables_fn(pr_pts, pr_ids, gt_pts, gt_ids, L))
        self.results["miou"] = {}
        for label in names:
            iou_1 = self.results["groundtruth-to-prediction"][label]["iou"]
            iou_2 = self.results["prediction-to-groundtruth"][label]["iou"]
            self.results["miou"][label] = (iou_1 + iou_2) / 2.0 if iou_1 is not None and iou_2 is not None else None

    @staticmethod
    def _compare(names, table):
        """One direction's dictionary from its table (rows: the source's label, columns: the nearest target's)."""
        table = np.asarray(table, dtype=np.int64)
        total = int(table.sum())
        results = {}
        for k, label in enumerate(names):
            tp = int(table[k, k])
            fp = int(table[k, :].sum()) - tp
            fn = int(table[:, k].sum()) - tp
            res = {"tp": tp, "fp": fp, "tn": total - tp - fp - fn, "fn": fn, "precision": None, "recall": None, "iou": None}
            if tp + fp > 0:
                res["precision"] = tp / (tp + fp)
            if tp + fn > 0:
                res["recall"] = tp / (tp + fn)
            if tp + fn + fp > 0:
                res["iou"] = tp / (tp + fn + fp)
            results[label] = res
        return results
