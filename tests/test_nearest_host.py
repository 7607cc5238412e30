"""CPU: the nearest-point checker itself (tests/nearest_oracle.py), the argument errors of ``sc_nearest`` and
``sc_nearest_confusion`` that need no device, and the logic around the search -- ``CompareSegmentedPointClouds`` and
the two run functions -- driven with the checker's functions in place of the kernels."""
import math

import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import metrics, proc3d
from plant3dvision_amd.tasks.evaluation import point_cloud_evaluation_run, segmented_point_cloud_evaluation_run
from tests import dbscan_oracle
from tests import nearest_oracle as oracle

# the hand-worked case of __graft_entry__.smoke(): five targets, four queries, one tie, one query beyond max_distance
SMOKE_TARGETS = np.array([[0, 0, 0], [2, 0, 0], [0, 3, 0], [2, 0, 0], [10, 10, 10]], dtype=np.float64)
SMOKE_QUERIES = np.array([[1, 0, 0], [2, 0.5, 0], [0, 2, 0], [5, 5, 5]], dtype=np.float64)
SMOKE_INDEX, SMOKE_D2 = [0, 1, 2, -1], [1.0, 0.25, 1.0, np.inf]  # max_distance 2: (5, 5, 5) is sqrt(54) from target 2


# ---- the checker ----------------------------------------------------------------------------------------------------
def test_hand_worked_case():
    for fn in (oracle.nearest, oracle.nearest_all_pairs):
        index, d2 = fn(SMOKE_QUERIES, SMOKE_TARGETS, 2.0)
        assert index.dtype == np.int32 and index.tolist() == SMOKE_INDEX and d2.tolist() == SMOKE_D2
        index, d2 = fn(SMOKE_QUERIES, SMOKE_TARGETS)
        assert index.tolist() == [0, 1, 2, 2] and d2.tolist() == [1.0, 0.25, 1.0, 54.0]
    assert oracle.sums(np.array(SMOKE_D2)) == (3, 2.25, 2.5)
    assert oracle.registration_fitness(SMOKE_QUERIES, SMOKE_TARGETS, 2.0) == (0.75, math.sqrt(0.75))


def test_exactly_max_distance_is_unmatched():
    targets = np.array([[0.0, 0.0, 0.0]])
    queries = np.array([[2.0, 0.0, 0.0], [np.nextafter(2.0, 0.0), 0.0, 0.0], [np.nextafter(2.0, 3.0), 0.0, 0.0], [0.0, 1.2, 1.6]])
    index, d2 = oracle.nearest(queries, targets, 2.0)
    assert index.tolist() == [-1, 0, -1, -1 if (1.2 * 1.2 + 1.6 * 1.6) >= 4.0 else 0] and d2[0] == np.inf and d2[1] < 4.0


def test_tree_form_equals_all_pairs_on_ties_and_duplicates():
    queries, targets = oracle.tie_clouds()
    assert queries.shape == (200, 3) and targets.shape == (228, 3)
    for shift, sign in (((0.0, 0.0, 0.0), 1.0), ((1e6, -1e6, 0.5), 1.0), ((0.0, 0.0, 0.0), -1.0)):
        q, t = sign * queries + np.array(shift), sign * targets + np.array(shift)
        index, d2, ties = oracle.nearest(q, t, return_ties=True)
        want = oracle.nearest_all_pairs(q, t)
        assert ties >= 150
        assert np.array_equal(index, want[0]) and np.array_equal(d2, want[1])
        for md in (0.5, 0.75, 2.0):  # 0.5: the edge midpoints lie at exactly max_distance
            got, want = oracle.nearest(q, t, md), oracle.nearest_all_pairs(q, t, md)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    blobs = dbscan_oracle.blobs_cloud()
    targets = oracle.blob_targets(blobs)
    got, want = oracle.nearest(blobs, targets), oracle.nearest_all_pairs(blobs, targets)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # a duplicate with a smaller index wins
    index, _ = oracle.nearest(np.array([[1.0, 1.0, 1.0]]), np.array([[5.0, 5, 5], [1, 1, 1], [1, 1, 1]]))
    assert index.tolist() == [1]
    for fn in (oracle.nearest, oracle.nearest_all_pairs):
        index, d2 = fn(np.zeros((3, 3)), np.zeros((0, 3)))
        assert index.tolist() == [-1] * 3 and np.all(np.isinf(d2))
        assert fn(np.zeros((0, 3)), np.zeros((3, 3)))[0].shape == (0,)


# ---- sc_nearest: judged before any device call -------------------------------------------------------------------------
def _call(Q=4, P=5, md=0.0, queries=SMOKE_QUERIES, targets=SMOKE_TARGETS, q_null=False, t_null=False, outs=True, device=0, dev_out=0):
    b = nat.backend()
    index, d2, sums = np.full(8, 7, dtype=np.int32), np.full(8, 7.0), np.full(3, 7.0)
    rc = b.call("sc_nearest", 0 if q_null else nat.addr(queries), 0, int(Q), 0 if t_null else nat.addr(targets), 0, int(P), float(md), device,
                nat.addr(index) if outs else 0, nat.addr(d2) if outs else 0, dev_out, nat.addr(sums) if outs else 0, 0)
    return rc, b.string(b.call("sc_nearest_last_error")), index, d2, sums


def test_nearest_argument_errors_need_no_device():
    for kw, word in [(dict(q_null=True), "null"), (dict(t_null=True), "null"), (dict(outs=False), "null"),
                     (dict(Q=-1), "Q must be"), (dict(Q=2 ** 31), "Q must be"), (dict(P=-1), "P must be"), (dict(P=2 ** 40), "P must be"),
                     (dict(md=float("nan")), "max_distance must be finite"), (dict(md=float("inf")), "max_distance must be finite"),
                     (dict(md=1e-200), "max_distance * max_distance"), (dict(md=1e200), "max_distance * max_distance"),
                     (dict(device=-1), "device"), (dict(device=64), "device"), (dict(P=0, dev_out=1), "P == 0")]:
        rc, msg, index, d2, _ = _call(**kw)
        assert rc == nat.SC_ERR_INVALID and word in msg, (kw, msg)
        assert index.tolist() == [7] * 8 and d2.tolist() == [7.0] * 8  # nothing written
    for bad in (np.nan, np.inf, -np.inf):
        broken = SMOKE_QUERIES.copy()
        broken[2, 1] = bad
        rc, msg, _, _, _ = _call(queries=broken)
        assert rc == nat.SC_ERR_INVALID and "non-finite coordinate in query 2" in msg
        broken = SMOKE_TARGETS.copy()
        broken[4, 0] = bad
        rc, msg, _, _, _ = _call(targets=broken)
        assert rc == nat.SC_ERR_INVALID and "non-finite coordinate in target 4" in msg


def test_empty_clouds_need_no_device():
    rc, _, index, d2, sums = _call(P=0)  # N4
    assert rc == nat.SC_OK and index.tolist() == [-1] * 4 + [7] * 4 and np.all(np.isinf(d2[:4])) and sums.tolist() == [0.0, 0.0, 0.0]
    rc, _, index, _, sums = _call(Q=0)
    assert rc == nat.SC_OK and index.tolist() == [7] * 8 and sums.tolist() == [0.0, 0.0, 0.0]
    rc, _, _, _, _ = _call(Q=0, P=0, q_null=True, t_null=True)
    assert rc == nat.SC_OK
    index, d2 = proc3d.nearest_points(np.zeros((3, 3)), np.zeros((0, 3)))
    assert index.dtype == np.int32 and index.tolist() == [-1] * 3 and d2.dtype == np.float64 and np.all(np.isinf(d2))
    index, d2 = proc3d.nearest_points(np.zeros((0, 3)), proc3d.PointCloud(np.zeros((4, 3)), None), 1.0)
    assert index.shape == (0,) and d2.shape == (0,)
    assert metrics.point_cloud_registration_fitness(np.zeros((0, 3)), np.zeros((4, 3))) == (0.0, 0.0)
    assert metrics.point_cloud_registration_fitness(np.zeros((4, 3)), np.zeros((0, 3))) == (0.0, 0.0)
    for a, b in ((np.zeros((0, 3)), np.zeros((4, 3))), (np.zeros((4, 3)), np.zeros((0, 3)))):
        with pytest.raises(ValueError, match="not empty"):
            metrics.chamfer_distance(a, b)


def _confusion(index, qlab, tlab, L, Q=None, P=None, nulls=(), device=0):
    b = nat.backend()
    index, qlab, tlab = (np.ascontiguousarray(a, dtype=np.int32) for a in (index, qlab, tlab))
    counts = np.full(max(L, 1) ** 2 if 0 < L <= 64 else 4, 7, dtype=np.int64)
    ptr = [0 if k in nulls else nat.addr(a) for k, a in enumerate((index, qlab, tlab, counts))]
    rc = b.call("sc_nearest_confusion", ptr[0], ptr[1], 0, len(index) if Q is None else Q, ptr[2], 0, len(tlab) if P is None else P, L, device,
                ptr[3], 0)
    return rc, b.string(b.call("sc_nearest_last_error")), counts


def test_confusion_argument_errors_need_no_device():
    idx, ql, tl = [0, 1, -1], [0, 1, 1], [1, 0]
    for kw, word in [(dict(nulls=(0,)), "null"), (dict(nulls=(1,)), "null"), (dict(nulls=(2,)), "null"), (dict(nulls=(3,)), "null"),
                     (dict(Q=-1), "Q must be"), (dict(Q=2 ** 31), "Q must be"), (dict(P=2 ** 31), "P must be"), (dict(device=99), "device")]:
        rc, msg, counts = _confusion(idx, ql, tl, 2, **kw)
        assert rc == nat.SC_ERR_INVALID and word in msg, (kw, msg)
        assert np.all(counts == 7)
    for L in (0, -3, 4097):
        rc, msg, _ = _confusion(idx, ql, tl, L)
        assert rc == nat.SC_ERR_INVALID and "L must be" in msg
    for args, word in [(([0, 2, -1], ql, tl), "index 1 is outside"), (([0, -2, -1], ql, tl), "index 1 is outside"),
                       ((idx, [0, 1, 2], tl), "query label 2 is outside"), ((idx, [-1, 1, 1], tl), "query label 0 is outside"),
                       ((idx, ql, [1, 5]), "target label 1 is outside")]:
        rc, msg, counts = _confusion(*args, 2)
        assert rc == nat.SC_ERR_INVALID and word in msg
        assert np.all(counts == 7)
    rc, _, counts = _confusion([], [], tl, 2)  # no query: zeros, no device call
    assert rc == nat.SC_OK and counts.tolist() == [0] * 4


def test_python_entries_raise_value_error():
    import torch
    with pytest.raises(ValueError, match="max_distance must be positive"):
        proc3d.nearest_points(SMOKE_QUERIES, SMOKE_TARGETS, 0.0)
    with pytest.raises(ValueError, match="max_distance must be positive"):
        proc3d.nearest_points(SMOKE_QUERIES, SMOKE_TARGETS, float("inf"))
    with pytest.raises(ValueError, match="max_distance must be positive"):
        metrics.point_cloud_registration_fitness(SMOKE_QUERIES, SMOKE_TARGETS, -2)
    with pytest.raises(ValueError, match=r"max_distance \* max_distance"):
        proc3d.nearest_points(SMOKE_QUERIES, SMOKE_TARGETS, 1e-200)
    with pytest.raises(ValueError, match="non-finite coordinate in target 1"):
        proc3d.nearest_points(SMOKE_QUERIES, proc3d.PointCloud(np.array([[0.0, 0, 0], [0, np.nan, 0]]), None))
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        proc3d.nearest_points(np.zeros((3, 2)), SMOKE_TARGETS)
    # mixed kinds: a tensor on one side, an array on the other (a CPU tensor is refused as a device cloud first)
    with pytest.raises(ValueError, match="CUDA tensor"):
        proc3d.nearest_points(torch.zeros((3, 3), dtype=torch.float64), SMOKE_TARGETS)

    class FakeDeviceCloud:  # passes for a device tensor as far as the kind check looks
        dtype, is_cuda, shape = torch.float64, True, (3, 3)
        def data_ptr(self): return 0
        def is_contiguous(self): return True
        def dim(self): return 2

    for args in ((FakeDeviceCloud(), SMOKE_TARGETS), (SMOKE_QUERIES, FakeDeviceCloud())):
        with pytest.raises(ValueError, match="both be arrays"):
            proc3d.nearest_points(*args)
    with pytest.raises(ValueError, match="both be arrays or both CUDA"):
        proc3d.nearest_confusion(FakeDeviceCloud(), np.zeros(3, np.int32), np.zeros(3, np.int32), 2)


def test_no_cpu_fallback_without_device():
    try:
        n = nat.device_count()
    except nat.SpaceCarveError:
        n = 0
    if n > 0:
        pytest.skip("a gfx950 device is present")
    with pytest.raises(nat.SpaceCarveError):
        proc3d.nearest_points(SMOKE_QUERIES, SMOKE_TARGETS)
    with pytest.raises(nat.SpaceCarveError):
        metrics.chamfer_distance(SMOKE_QUERIES, SMOKE_TARGETS)
    with pytest.raises(nat.SpaceCarveError):
        proc3d.nearest_confusion([0, 1], [0, 1], [0, 1], 2)


# ---- the logic around the search, with the checker's functions injected ----------------------------------------------
def _labelled():
    rng = np.random.default_rng(17)
    gt = rng.uniform(0.0, 4.0, size=(60, 3))
    pred = np.concatenate([gt[:40] + rng.normal(scale=0.2, size=(40, 3)), rng.uniform(0.0, 4.0, size=(15, 3))])
    gt_labels = ["leaf"] * 25 + ["stem"] * 20 + ["fruit"] * 15  # fruit: no predicted point
    pred_labels = ["leaf"] * 20 + ["stem"] * 20 + ["flower"] * 15  # flower: only in the prediction
    return gt, gt_labels, pred, pred_labels


def test_compare_segmented_point_clouds_arithmetic():
    gt, gt_labels, pred, pred_labels = _labelled()
    seen = []

    def tables_fn(source, source_ids, target, target_ids, L):
        seen.append((len(source), len(target), L, int(max(source_ids)), int(max(target_ids))))
        return oracle.tables(source, source_ids, target, target_ids, L)

    got = metrics.CompareSegmentedPointClouds(proc3d.PointCloud(gt, None), gt_labels, proc3d.PointCloud(pred, None), pred_labels,
                                              tables_fn=tables_fn)
    want = oracle.compare_segmented(gt, gt_labels, pred, pred_labels)
    assert got.results == want
    assert got.unique_labels == {"leaf", "stem", "fruit"} and "flower" not in got.results["miou"]
    assert [s[:3] for s in seen] == [(60, 55, 4), (55, 60, 4)] and seen[0][4] == 3 and seen[1][3] == 3  # "other" is id 3
    g2p, p2g = want["groundtruth-to-prediction"], want["prediction-to-groundtruth"]
    assert g2p["fruit"]["tp"] == 0 and g2p["fruit"]["fp"] == 15 and g2p["fruit"]["fn"] == 0 and g2p["fruit"]["recall"] is None
    assert p2g["fruit"]["precision"] is None and p2g["fruit"]["tp"] + p2g["fruit"]["fp"] == 0 and want["miou"]["fruit"] == 0.0
    assert g2p["leaf"]["tp"] > 0 and all(sum(r[k] for k in ("tp", "fp", "tn", "fn")) == 60 for r in g2p.values())
    # one label everywhere: L = 1
    one = metrics.CompareSegmentedPointClouds(gt, ["a"] * 60, pred, ["a"] * 55, tables_fn=tables_fn)
    assert seen[-1][2] == 1 and one.results == oracle.compare_segmented(gt, ["a"] * 60, pred, ["a"] * 55)
    assert one.results["miou"] == {"a": 1.0}
    # the size check is the reference's
    with pytest.raises(ValueError, match=r"#points\(60\) != #labels\(59\)"):
        metrics.CompareSegmentedPointClouds(gt, gt_labels[:-1], pred, pred_labels, tables_fn=tables_fn)
    with pytest.raises(ValueError, match=r"#points\(55\) != #labels\(56\)"):
        metrics.CompareSegmentedPointClouds(gt, gt_labels, pred, pred_labels + ["leaf"], tables_fn=tables_fn)


def test_segmented_point_cloud_evaluation_run():
    gt, gt_labels, pred, pred_labels = _labelled()
    calls = []

    def compare_fn(groundtruth, labels_gt, prediction, labels):
        calls.append((len(groundtruth), len(labels_gt), len(prediction), len(labels)))
        return metrics.CompareSegmentedPointClouds(groundtruth, labels_gt, prediction, labels, tables_fn=oracle.tables)

    got = segmented_point_cloud_evaluation_run(pred, pred_labels, gt, gt_labels, compare_fn=compare_fn)
    assert calls == [(60, 60, 55, 55)] and got == oracle.compare_segmented(gt, gt_labels, pred, pred_labels)
    with pytest.raises(ValueError, match="labels parameter is empty"):
        segmented_point_cloud_evaluation_run(pred, [], gt, gt_labels, compare_fn=compare_fn)
    with pytest.raises(ValueError, match="#points"):
        segmented_point_cloud_evaluation_run(pred, pred_labels[:-2], gt, gt_labels, compare_fn=compare_fn)


def test_point_cloud_evaluation_run():
    gt, gt_labels, pred, pred_labels = _labelled()
    calls = []

    def registration_fn(source, target, max_distance):
        calls.append((len(source), len(target), max_distance))
        return oracle.registration_fitness(source, target, max_distance)

    got = point_cloud_evaluation_run(proc3d.PointCloud(pred, None), gt, pred_labels, gt_labels, max_distance=0.5, task_id="PointCloud_x",
                                     registration_fn=registration_fn)
    assert set(got) == {"id", "all", "leaf", "stem", "fruit"} and got["id"] == "PointCloud_x"  # flower has no ground truth: skipped
    fit, rmse = oracle.registration_fitness(pred, gt, 0.5)
    assert got["all"] == {"fitness": fit, "inlier_rmse": rmse} and 0.0 < fit < 1.0 and rmse > 0.0
    fit, rmse = oracle.registration_fitness(pred[:20], gt[:25], 0.5)
    assert got["leaf"] == {"fitness": fit, "inlier_rmse": rmse}
    assert got["fruit"] == {"fitness": 0.0, "inlier_rmse": 0.0}  # no source point
    assert sorted(calls) == sorted([(55, 60, 0.5), (20, 25, 0.5), (20, 20, 0.5)])
    # without labels: the whole clouds only, the reference's default max_distance
    calls.clear()
    got = point_cloud_evaluation_run(pred, gt, registration_fn=registration_fn)
    assert set(got) == {"id", "all"} and got["id"] is None and calls == [(55, 60, 2)]
