"""The checkers of ``plant3dvision_amd.metrics``: the two evaluation tasks of the reference restated in NumPy and
``scipy.ndimage``, in the reference's own order of operations.

``voxel_histograms`` follows ``VoxelsEvaluation.evaluate`` (plant3dvision/tasks/evaluation.py:428-477): the float64
``[nx, ny, nz, L]`` array, ``argmax``, per class ``np.delete`` + ``np.max``, the comparison with 10 times that, the
ground truth's corner, four boolean-index sums.  ``mask_counts`` follows ``MaskEvaluator.evaluate``
(plant3dvision/metrics.py:246-272): ``binary_dilation(image > 0)`` ``dilation_amount`` times, ``!= 0``, four sums.
Nothing here knows how the device counts.

``quad_plan`` is the one exception, and it decides no result: a replica of the run plan of csrc/sc_quads.h
(``plan_quads``), with its constants read out of the header's text, so that the tests can choose volumes whose blocks
walk several x-planes and say so (tests/test_unit_plans_host.py pins it).  ``needle_volumes`` places its predictions
by that plan.
"""
import os
import re
import warnings

import numpy as np

# The smallest volumes whose blocks walk more than one x-plane (quad_plan: xc, planes of the last run): one tile and
# xc 2 with a last run of 1, nz a multiple of 4; xc 3 with a last run of 1, row tails; two tiles with a whole last run
# of 2, misaligned rows; two tiles with a last run of 1, whole aligned quads.
LONG_SHAPES = [(4099, 2, 8), (10000, 3, 7), (2100, 17, 61), (2049, 17, 64)]
# host volumes of SLAB_SHAPE under a chunk limit with room for SLAB_PLANES planes: slabs of 4100, 4100 and 1800 planes
SLAB_SHAPE, SLAB_PLANES = (10000, 3, 7), 4100

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "plant-3d-vision_amd", "csrc")


def source_constant(source, name, pattern=None):
    """The integer ``name`` is set to in csrc/``source``: ``constexpr <type> name = <digits>;``, or group 1 of
    ``pattern``.  A constant that is no longer there fails loudly: the tests' sizes were chosen by its value."""
    with open(os.path.join(CSRC, source)) as f:
        text = f.read()
    found = re.findall(pattern or r"\bconstexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % re.escape(name), text)
    if len(found) != 1:
        raise AssertionError(f"csrc/{source}: {name} was expected once as a plain integer constant, found {len(found)} "
                             f"times -- the launch plans' replica in the tests has to follow the source")
    return int(found[0])


def quad_plan(planes, ny, nz):
    """``plan_quads`` of csrc/sc_quads.h for one launch over ``planes`` x-planes of ``ny`` x ``nz`` voxels: ``tiles``
    (blocks per run of planes), ``xc`` (x-planes a block walks), ``runs`` and ``last`` (the planes of the last run)."""
    threads, fill = source_constant("sc_quads.h", "kQuadThreads"), source_constant("sc_quads.h", "kFillBlocks")
    log2 = source_constant("sc_quads.h", "kRunPlanesLog2")
    tiles = (ny * ((nz + 3) // 4) + threads - 1) // threads
    least = (planes + (1 << log2) - 1) >> log2
    runs = min(planes, max((fill + tiles - 1) // tiles, least))
    xc = (planes + runs - 1) // runs
    runs = (planes + xc - 1) // xc
    return {"tiles": tiles, "xc": xc, "runs": runs, "last": planes - (runs - 1) * xc, "threads": threads}

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
    return voxels, {k: _adversarial_gt(rng, gshape, gt_dtype) for k in labels}


def _adversarial_gt(rng, gshape, gt_dtype):
    g = GT_POOL[rng.integers(0, GT_POOL.size, size=gshape)]
    if np.dtype(gt_dtype) == np.bool_:
        g = np.nan_to_num(g, nan=0.0) > 0.5
    elif np.dtype(gt_dtype).kind == "u":
        g = np.clip(np.nan_to_num(g, nan=3.0), 0, 255)  # 0, 1, 2, 3 and 0.5 -> 0
    return g.astype(gt_dtype)


def needle_planes(nx, plan):
    """The x-planes of a launch by their place in a block's run (``plan``: ``quad_plan``'s): ``first`` and ``last`` of
    a whole run, ``middle`` (runs of 3 planes and more), ``short`` (a last run of fewer planes than the others).  Only
    the kinds the plan has."""
    xc, x = plan["xc"], np.arange(nx)
    short = (x >= (plan["runs"] - 1) * xc) & (plan["last"] < xc)
    kinds = {"first": x[~short & (x % xc == 0)], "last": x[~short & (x % xc == xc - 1)],
             "middle": x[~short & (x % xc > 0) & (x % xc < xc - 1)], "short": x[short]}
    return {name: planes for name, planes in kinds.items() if len(planes)}


def needle_volumes(shape, gshape, nclasses, seed, pred_dtype=np.float32, gt_dtype=np.uint8):
    """``(voxels, gts, at, placed)`` for the projection over long volumes.  Every class has the same value (1, 0.5 or
    2) at a voxel, so nothing is predicted, except that about a third of the ``(class, y, z)`` columns have ONE x where
    their class is 32 times that: ``at[c, y, z]`` is this x, or -1.  The x are taken in turn from the kinds of
    ``needle_planes``; ``placed[kind]`` counts them.  Ground truths are the adversarial pool's."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    kinds = needle_planes(nx, quad_plan(nx, ny, nz))
    names = list(kinds)
    labels = [f"c{q}" for q in range(nclasses)]
    base = np.array([1.0, 0.5, 2.0])[rng.integers(0, 3, size=shape)]
    at = np.full((nclasses, ny, nz), -1, dtype=np.int64)
    flat = at.reshape(-1)
    for q, cell in enumerate(np.flatnonzero(rng.random(flat.size) < 0.3)):
        planes = kinds[names[q % len(names)]]
        flat[cell] = planes[rng.integers(0, len(planes))]
    for c in range(1, nclasses):  # two classes at one voxel would tie and predict nothing: the later one gives way
        for b in range(c):
            at[c][at[c] == at[b]] = -1
    voxels = {}
    for c, k in enumerate(labels):
        v = base.copy()
        y, z = np.nonzero(at[c] >= 0)
        v[at[c][y, z], y, z] *= 32.0
        voxels[k] = v.astype(pred_dtype)
    placed = {name: int(np.isin(at[at >= 0], kinds[name]).sum()) for name in names}
    return voxels, {k: _adversarial_gt(rng, gshape, gt_dtype) for k in labels}, at, placed


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
