"""The checkers of ``plant3dvision_amd.metrics``: the two evaluation tasks of the reference restated in NumPy and
``scipy.ndimage``, in the reference's own order of operations.

``voxel_histograms`` follows ``VoxelsEvaluation.evaluate`` (plant3dvision/tasks/evaluation.py:428-477): the float64
``[nx, ny, nz, L]`` array, ``argmax``, per class ``np.delete`` + ``np.max``, the comparison with 10 times that, the
ground truth's corner, four boolean-index sums.  ``mask_counts`` follows ``MaskEvaluator.evaluate``
(plant3dvision/metrics.py:246-272): ``binary_dilation(image > 0)`` ``dilation_amount`` times, ``!= 0``, four sums.
Nothing here knows how the device counts.
"""
import warnings

import numpy as np

# what the adversarial volumes are drawn from: repeated maxima, negatives, infinities, NaN, values on the contrast
# boundary (1 against 0.1, 10 against 1, 0.5 against 0.05: exact products in float64 or not)
PRED_POOL = np.array([0.0, 1.0, 1.0, 0.1, 10.0, 0.5, 0.05, -1.0, -10.0, -0.1, 2.0, 20.0, 3.0, np.inf, -np.inf, np.nan,
                      1e-30, 0.099999, 0.100001, 5.0], dtype=np.float64)
GT_POOL = np.array([0.0, 1.0, 0.5, 0.49999, 0.50001, np.nan, 2.0, -1.0], dtype=np.float64)


def voxel_histograms(voxels, gts, background="background", min_contrast=10, projections=False):
    """``{label: {"tp", "fp", "tn", "fn"}}`` (and ``{label: prediction_c.max(0)}``) as the reference computes them."""
    histograms, proj = {}, {}
    l = list(gts.keys())
    res = np.zeros((*voxels[l[0]].shape, len(l)))
    for i in range(len(l)):
        res[:, :, :, i] = voxels[l[i]]
    res_idx = np.argmax(res, axis=3)
    for i, c in enumerate(l):
        if c == background:
            continue
        prediction_c = res_idx == i
        pred_no_c = np.max(np.delete(res, i, axis=3), axis=3)
        pred_c = res[:, :, :, i]
        with warnings.catch_warnings(), np.errstate(invalid="ignore"):
            warnings.simplefilter("ignore")
            prediction_c = prediction_c * (pred_c > (min_contrast * pred_no_c))
        gt_c = np.asarray(gts[c])
        gt_c = gt_c[0:prediction_c.shape[0], 0:prediction_c.shape[1], 0:prediction_c.shape[2]]
        proj[c] = prediction_c.max(0).astype(np.uint8)
        with np.errstate(invalid="ignore"):
            hi, lo = gt_c > 0.5, gt_c < 0.5
        tp = np.sum(prediction_c[hi])
        fn = np.sum(1 - prediction_c[hi])
        fp = np.sum(prediction_c[lo])
        tn = np.sum(1 - prediction_c[lo])
        histograms[c] = {"tp": tp.tolist(), "fp": fp.tolist(), "tn": tn.tolist(), "fn": fn.tolist()}
    return (histograms, proj) if projections else histograms


def adversarial_volumes(shape, gshape, nclasses, seed, pred_dtype=np.float64, gt_dtype=np.float64):
    """``(voxels, gts)`` with the labels ``c0 .. c{n-1}``, drawn from the pools above."""
    rng = np.random.default_rng(seed)
    labels = [f"c{q}" for q in range(nclasses)]
    voxels = {k: PRED_POOL[rng.integers(0, PRED_POOL.size, size=shape)].astype(pred_dtype) for k in labels}
    gts = {}
    for k in labels:
        g = GT_POOL[rng.integers(0, GT_POOL.size, size=gshape)]
        if np.dtype(gt_dtype) == np.bool_:
            g = np.nan_to_num(g, nan=0.0) > 0.5
        elif np.dtype(gt_dtype).kind == "u":
            g = np.clip(np.nan_to_num(g, nan=3.0), 0, 255)  # 0, 1, 2, 3 and 0.5 -> 0
        gts[k] = g.astype(gt_dtype)
    return voxels, gts


def mask_counts(groundtruth, prediction, dilation_amount=0):
    """``(tp, fn, tn, fp)`` of one pair of pictures as ``MaskEvaluator.evaluate`` computes them."""
    from scipy.ndimage import binary_dilation
    if groundtruth.shape != prediction.shape:
        raise ValueError("The groundtruth and prediction are different in size: %s vs %s"
                         % (str(groundtruth.shape), str(prediction.shape)))
    image = prediction
    for _ in range(dilation_amount):
        image = binary_dilation(image > 0)
    groundtruth = (groundtruth != 0).astype(int)
    prediction = (image != 0).astype(int)
    tp = int(np.sum(groundtruth * (prediction > 0)))
    fn = int(np.sum(groundtruth * (prediction == 0)))
    tn = int(np.sum((groundtruth == 0) * (prediction == 0)))
    fp = int(np.sum((groundtruth == 0) * (prediction > 0)))
    return tp, fn, tn, fp


def mask_stack_counts(groundtruths, predictions, dilation_amount=0):
    """int64 ``[n, 4]``: ``mask_counts`` of every pair of two stacks (the form ``compare_mask_stacks`` returns)."""
    return np.array([mask_counts(g, p, dilation_amount) for g, p in zip(groundtruths, predictions)], dtype=np.int64).reshape(-1, 4)


def metrics_dict(rows):
    """``SetMetrics.as_dict()`` after adding the ``(tp, fn, tn, fp)`` of ``rows`` one by one (metrics.py:157-204)."""
    tp = fn = tn = fp = 0
    miou, count = 0, 0
    for a, b, c, d in rows:
        tp, fn, tn, fp = tp + a, fn + b, tn + c, fp + d
        if (a + d + b) != 0:
            miou += a / (a + d + b)
            count += 1
    return {"tp": tp, "fn": fn, "tn": tn, "fp": fp, "precision": tp / (tp + fp) if (tp + fp) != 0 else None,
            "recall": tp / (tp + fn) if (tp + fn) != 0 else None, "miou": miou / count if count > 0 else None}


def border_pictures(n, H, W, seed):
    """``(groundtruths, predictions)`` uint8 ``[n, H, W]`` with values from {0, 1, 7, 255}: sparse predictions with
    set pixels on every border and in every corner, denser ground truths."""
    rng = np.random.default_rng(seed)
    values = np.array([1, 7, 255], dtype=np.uint8)
    pred = np.where(rng.random((n, H, W)) < 0.02, values[rng.integers(0, 3, size=(n, H, W))], 0).astype(np.uint8)
    gt = np.where(rng.random((n, H, W)) < 0.4, values[rng.integers(0, 3, size=(n, H, W))], 0).astype(np.uint8)
    for v in range(n):
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1)):
            pred[v, y, x] = values[(v + y + x) % 3]
    return gt, pred
