"""CPU: the DBSCAN checker itself (tests/dbscan_oracle.py) on hand-worked cases, the argument errors of ``sc_dbscan``
that need no device, and the task loop ``organ_segmentation_run`` around a clustering function of the test's own."""
import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd.tasks.proc3d import organ_segmentation_run
from tests import dbscan_oracle as oracle


# ---- the checker on cases worked by hand ------------------------------------------------------------------------
def test_two_points_exactly_eps_apart_are_not_neighbours():
    pts = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    i, j = oracle.neighbour_pairs(pts, 2.0)
    assert list(zip(i.tolist(), j.tolist())) == [(0, 0), (1, 1)]  # each its own neighbour, nothing else
    assert oracle.labels(pts, 2.0, 2).tolist() == [-1, -1]
    assert oracle.labels(pts, 2.0, 1).tolist() == [0, 1]
    closer = np.array([[0.0, 0.0, 0.0], [np.nextafter(2.0, 0.0), 0.0, 0.0]])
    assert oracle.labels(closer, 2.0, 2).tolist() == [0, 0]
    # a 3-4-5 tie off the axes: d2 = 9 + 16 = 25 exactly
    assert oracle.labels(np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]]), 5.0, 2).tolist() == [-1, -1]


def test_hand_worked_line():
    # x: 0 1 2 | 10 | 20 21, eps 1.5, min_points 3: 1 is core (0, 1, 2), 0 and 2 are border, the rest noise
    pts = np.zeros((6, 3))
    pts[:, 0] = [0, 1, 2, 10, 20, 21]
    assert oracle.labels(pts, 1.5, 3).tolist() == [0, 0, 0, -1, -1, -1]
    assert oracle.labels(pts, 1.5, 2).tolist() == [0, 0, 0, -1, 1, 1]
    assert oracle.labels(pts, 1.5, 1).tolist() == [0, 0, 0, 1, 2, 2]
    assert oracle.labels(pts, 1.5, 0).tolist() == [0, 0, 0, 1, 2, 2]  # 0 behaves as 1
    assert oracle.labels(pts, 1.5, 4).tolist() == [-1] * 6
    assert oracle.labels(np.zeros((0, 3)), 1.0, 5).shape == (0,)
    # ids follow the smallest index of each cluster, not the position
    assert oracle.labels(pts[::-1].copy(), 1.5, 2).tolist() == [0, 0, -1, 1, 1, 1]


def test_contested_border_point_takes_the_first_cluster():
    pts2 = np.zeros((9, 3))
    pts2[:, 0] = [0.0, -0.5, -1.0, 1.8, 2.3, 2.8, 0.9, -0.25, 2.05]
    st = oracle.structure(pts2, 1.0, 4)
    assert st["core"][0] and st["core"][3] and not st["core"][6]
    assert st["contested"][6]
    assert st["labels"][6] == 0 and st["labels"][0] == 0 and st["labels"][3] == 1
    swapped = pts2[[3, 4, 5, 0, 1, 2, 6, 8, 7]].copy()  # the other group first: the point follows it
    lab = oracle.labels(swapped, 1.0, 4)
    assert lab[0] == 0 and lab[3] == 1 and lab[6] == 0


@pytest.mark.parametrize("cloud,params", [("blobs", oracle.BLOBS), ("lattice", oracle.LATTICE)])
def test_pop_order_and_the_order_free_form(cloud, params):
    """The literal loop gives one answer whatever element its work set hands out, and the vectorised order-free form
    (what the kernels build, and what the benchmark checks large clouds with) gives the same."""
    pts = oracle.blobs_cloud() if cloud == "blobs" else oracle.lattice_cloud()
    a = oracle.labels(pts, pop=oracle.pop_min, **params)
    b = oracle.labels(pts, pop=oracle.pop_max, **params)
    c = oracle.labels(pts, **params)
    assert a.max() >= 1 and (a == -1).any()
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(a, oracle.labels_order_free(pts, **params))
    for mp in (0, 1, 2, 50):
        assert np.array_equal(oracle.labels(pts, params["eps"], mp), oracle.labels_order_free(pts, params["eps"], mp))


def test_tree_candidates_equal_all_pairs(monkeypatch):
    pts = oracle.lattice_cloud()
    want = oracle.neighbour_pairs(pts, 2.0)
    monkeypatch.setattr(oracle, "BRUTE_MAX", 0)
    got = oracle.neighbour_pairs(pts, 2.0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_sklearn_agrees_where_nothing_ties():
    """sklearn's test is ``<=``: a cross-check on a tie-free cloud only, never the checker."""
    cluster = pytest.importorskip("sklearn.cluster")
    pts = oracle.blobs_cloud()
    st = oracle.structure(pts, **oracle.BLOBS)
    assert st["ties"] == 0
    sk = cluster.DBSCAN(eps=oracle.BLOBS["eps"], min_samples=oracle.BLOBS["min_points"], algorithm="brute").fit(pts)
    core = np.zeros(len(pts), dtype=bool)
    core[sk.core_sample_indices_] = True
    assert np.array_equal(core, st["core"])
    assert np.array_equal(sk.labels_, st["labels"])  # contested border points included: both walk in index order


# ---- sc_dbscan: judged before any device call -------------------------------------------------------------------
def _call(points, P, eps, min_points, labels=True, pts_null=False):
    b = nat.backend()
    lab = np.full(max(int(P), 1) if 0 <= P < 1000 else 1, 7, dtype=np.int32)
    ncl = np.full(1, 7, dtype=np.int32)
    rc = b.call("sc_dbscan", 0 if pts_null else nat.addr(points), 0, int(P), float(eps), int(min_points), 0,
                nat.addr(lab) if labels else 0, 0, nat.addr(ncl), 0)
    return rc, b.string(b.call("sc_dbscan_last_error")), lab, ncl


def test_argument_errors_need_no_device():
    pts = np.zeros((4, 3))
    for kw, word in [(dict(pts_null=True), "null"), (dict(labels=False), "null")]:
        rc, msg, _, _ = _call(pts, 4, 1.0, 5, **kw)
        assert rc == nat.SC_ERR_INVALID and word in msg
    for P in (-1, 2 ** 31, 2 ** 40):
        rc, msg, _, _ = _call(pts, P, 1.0, 5)
        assert rc == nat.SC_ERR_INVALID and "P must be" in msg
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg, _, _ = _call(pts, 4, eps, 5)
        assert rc == nat.SC_ERR_INVALID and "eps must be finite and positive" in msg
    for eps in (1e-200, 1e200):  # eps * eps is 0 or infinite: rule 2 would mean nothing
        rc, msg, _, _ = _call(pts, 4, eps, 5)
        assert rc == nat.SC_ERR_INVALID and "eps * eps" in msg
    rc, msg, _, _ = _call(pts, 4, 1.0, -1)
    assert rc == nat.SC_ERR_INVALID and "min_points" in msg
    for bad in (np.nan, np.inf, -np.inf):
        broken = pts.copy()
        broken[2, 1] = bad
        rc, msg, lab, _ = _call(broken, 4, 1.0, 5)
        assert rc == nat.SC_ERR_INVALID and "non-finite coordinate in point 2" in msg
        assert lab.tolist() == [7] * 4  # nothing written


def test_empty_cloud_needs_no_device():
    rc, _, _, ncl = _call(np.zeros((1, 3)), 0, 1.0, 5)
    assert rc == nat.SC_OK and ncl[0] == 0


def test_python_entry_raises_value_error():
    from plant3dvision_amd import proc3d
    with pytest.raises(ValueError, match="eps must be finite"):
        proc3d.cluster_dbscan(np.zeros((3, 3)), 0.0, 5)
    with pytest.raises(ValueError, match="non-finite coordinate in point 1"):
        proc3d.cluster_dbscan(proc3d.PointCloud(np.array([[0.0, 0, 0], [0, np.nan, 0]]), None), 1.0, 5)
    with pytest.raises(ValueError, match=r"\[P, 3\]"):
        proc3d.cluster_dbscan(np.zeros((3, 2)), 1.0, 5)
    got = proc3d.cluster_dbscan(np.zeros((0, 3)), 1.0, 5)
    assert got.dtype == np.int32 and got.shape == (0,)


# ---- the task loop ----------------------------------------------------------------------------------------------
def test_organ_segmentation_run():
    rng = np.random.default_rng(3)
    pts = rng.uniform(size=(12, 3))
    labels = ["leaf", "stem", "leaf", "fruit", "stem", "leaf", "flower", "leaf", "fruit", "leaf", "stem", "flower"]
    calls = []

    def cluster_fn(p, eps, min_points):
        calls.append((np.array(p), eps, min_points))
        n = len(p)
        if n == 5:  # leaf: clusters 1, 0, noise, 1, 0 -- ids out of order, one point dropped
            return np.array([1, 0, -1, 1, 0], dtype=np.int32)
        if n == 2 and np.array_equal(p, pts[[3, 8]]):  # fruit: all noise
            return [-1, -1]
        return np.zeros(n, dtype=np.int32)  # flower: one cluster

    parts = organ_segmentation_run(pts, labels, eps=0.25, min_points=3, cluster_fn=cluster_fn)
    names = [p[0] for p in parts]
    # labels in order of first appearance (leaf, stem, fruit, flower), clusters by id, a label without clusters: no part
    assert names == ["leaf_000", "leaf_001", "stem_000", "flower_000"]
    got = {name: idx.tolist() for name, idx, _ in parts}
    assert got == {"leaf_000": [2, 9], "leaf_001": [0, 7], "stem_000": [1, 4, 10], "flower_000": [6, 11]}
    assert [p[2] for p in parts] == [{"label": "leaf"}, {"label": "leaf"}, {"label": "stem"}, {"label": "flower"}]
    # stem never reaches the clustering; every other label does, with its own points and the task's parameters
    assert len(calls) == 3
    assert np.array_equal(calls[0][0], pts[[0, 2, 5, 7, 9]]) and calls[0][1:] == (0.25, 3)
    assert np.array_equal(calls[2][0], pts[[6, 11]])


def test_organ_segmentation_run_defaults_and_inputs():
    from plant3dvision_amd import proc3d
    seen = []

    def cluster_fn(p, eps, min_points):
        seen.append((eps, min_points))
        return np.arange(len(p)) % 12  # more than ten clusters: the name keeps three digits

    pcd = proc3d.PointCloud(np.zeros((24, 3)), None)
    parts = organ_segmentation_run(pcd, ["leaf"] * 24, cluster_fn=cluster_fn)
    assert seen == [(2.0, 5)]
    assert [p[0] for p in parts] == ["leaf_%03d" % k for k in range(12)] and parts[11][0] == "leaf_011"
    assert parts[3][1].tolist() == [3, 15]
    assert organ_segmentation_run(np.zeros((0, 3)), [], cluster_fn=cluster_fn) == []
    with pytest.raises(ValueError):
        organ_segmentation_run(np.zeros((3, 3)), ["a"], cluster_fn=cluster_fn)
