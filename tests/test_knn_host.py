"""CPU: the k-nearest checker itself (tests/knn_oracle.py, its two forms against each other), the argument errors of
``sc_knn`` that need no device, and the host logic of ``knn_edges`` / ``knn_graph`` with the checker's search injected."""
import builtins

import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import proc3d
from tests import dbscan_oracle
from tests import knn_oracle as oracle
from tests import nearest_oracle

# the hand-worked case of __graft_entry__.smoke(): five targets (1 and 3 coincide), two queries, k = 3.  Query 0 has
# d2 = 1, 1, 4, 1, 182: the three-way tie holds the row, in rising index.  Query 1 has d2 = 2, 2, 1, 2, 163: after
# target 2 the tie of three is CUT at the third place and target 3 stays out.
SMOKE_TARGETS = np.array([[0, 0, 0], [2, 0, 0], [1, 2, 0], [2, 0, 0], [10, 10, 1]], dtype=np.float64)
SMOKE_QUERIES = np.array([[1, 0, 0], [1, 1, 0]], dtype=np.float64)
SMOKE_INDEX, SMOKE_D2 = [[0, 1, 3], [2, 0, 1]], [[1.0, 1.0, 1.0], [1.0, 2.0, 2.0]]


# ---- the checker --------------------------------------------------------------------------------------------------
def test_hand_worked_case():
    for fn in (oracle.knn, oracle.knn_all_pairs):
        index, d2 = fn(SMOKE_QUERIES, SMOKE_TARGETS, 3)
        assert index.dtype == np.int32 and index.tolist() == SMOKE_INDEX and d2.tolist() == SMOKE_D2
        index, d2 = fn(SMOKE_QUERIES, SMOKE_TARGETS, 5)
        assert index.tolist() == [[0, 1, 3, 2, 4], [2, 0, 1, 3, 4]] and d2.tolist() == [[1.0, 1.0, 1.0, 4.0, 182.0], [1.0, 2.0, 2.0, 2.0, 163.0]]
        index, d2 = fn(SMOKE_QUERIES, SMOKE_TARGETS, 5, 1.25)  # K3, K4: sqrt(2) is beyond 1.25
        assert index.tolist() == [[0, 1, 3, -1, -1], [2, -1, -1, -1, -1]] and d2.tolist() == [[1.0] * 3 + [np.inf] * 2, [1.0] + [np.inf] * 4]
        index, d2 = fn(SMOKE_QUERIES, SMOKE_TARGETS, 2, 1.0)  # strict: exactly max_distance does not count
        assert np.all(index == -1) and np.all(np.isinf(d2))


def test_tree_form_equals_all_pairs_on_ties_and_duplicates():
    queries, targets = nearest_oracle.tie_clouds()
    for shift, sign in (((0.0, 0.0, 0.0), 1.0), ((1e6, -1e6, 0.5), 1.0), ((0.0, 0.0, 0.0), -1.0)):
        q, t = sign * queries + np.array(shift), sign * targets + np.array(shift)
        for k in (1, 5, 8, 64, 300):  # 300: more places than the 228 targets
            for md in (None, 0.5, 2.0):
                got, want = oracle.knn(q, t, k, md), oracle.knn_all_pairs(q, t, k, md)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (shift, sign, k, md)
        one = nearest_oracle.nearest_all_pairs(q, t)  # k = 1 is the nearest point's checker
        got = oracle.knn_all_pairs(q, t, 1)
        assert np.array_equal(got[0][:, 0], one[0]) and np.array_equal(got[1][:, 0], one[1])
    eight = oracle.knn_all_pairs(queries, targets, 8)
    five = oracle.knn_all_pairs(queries, targets, 5)
    assert np.all(eight[1][:80] == 0.75) and np.all(np.diff(eight[0][:80], axis=1) > 0)  # the cell centres: 8-way ties
    assert np.array_equal(five[0], eight[0][:, :5])  # cut: the five smallest indices
    # duplicates: 300 copies of one point
    copies = np.tile([[1.25, -2.5, 0.75]], (300, 1))
    q = np.random.default_rng(3).uniform(-5.0, 5.0, size=(40, 3))
    for fn in (oracle.knn, oracle.knn_all_pairs):
        index, d2 = fn(q, copies, 10)
        assert np.array_equal(index, np.tile(np.arange(10, dtype=np.int32), (40, 1))) and np.all(d2 == d2[:, :1])
    blobs = dbscan_oracle.blobs_cloud()[:600]
    targets = nearest_oracle.blob_targets(blobs)
    got, want = oracle.knn(blobs, targets, 16), oracle.knn_all_pairs(blobs, targets, 16)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for fn in (oracle.knn, oracle.knn_all_pairs):
        index, d2 = fn(np.zeros((3, 3)), np.zeros((0, 3)), 4)
        assert index.shape == (3, 4) and np.all(index == -1) and np.all(np.isinf(d2))
        assert fn(np.zeros((0, 3)), np.zeros((3, 3)), 4)[0].shape == (0, 4)


# ---- sc_knn: judged before any device call ---------------------------------------------------------------------------
def _call(Q=2, P=5, k=3, md=0.0, queries=SMOKE_QUERIES, targets=SMOKE_TARGETS, nulls=(), device=0, dev_out=0, far=True):
    b = nat.backend()
    index, d2, nfar = np.full(16, 7, dtype=np.int32), np.full(16, 7.0), np.full(1, 7, dtype=np.int64)
    ptr = [0 if name in nulls else nat.addr(a) for name, a in (("q", queries), ("t", targets), ("index", index), ("d2", d2))]
    rc = b.call("sc_knn", ptr[0], 0, int(Q), ptr[1], 0, int(P), int(k), float(md), device, ptr[2], ptr[3], dev_out, nat.addr(nfar) if far else 0, 0)
    return rc, b.string(b.call("sc_nearest_last_error")), index, d2, nfar


def test_knn_argument_errors_need_no_device():
    for kw, word in [(dict(k=0), "k must be"), (dict(k=-3), "k must be"), (dict(k=nat.SC_KNN_MAX + 1), "k must be"),
                     (dict(Q=2 ** 31 // 512, k=512), "Q * k"), (dict(Q=2 ** 31 - 1, k=2), "Q * k"),
                     (dict(nulls=("q",)), "null"), (dict(nulls=("t",)), "null"), (dict(nulls=("index",)), "null"), (dict(nulls=("d2",)), "null"),
                     (dict(Q=-1), "Q must be"), (dict(Q=2 ** 31), "Q must be"), (dict(P=-1), "P must be"), (dict(P=2 ** 40), "P must be"),
                     (dict(md=float("nan")), "max_distance must be finite"), (dict(md=float("inf")), "max_distance must be finite"),
                     (dict(md=1e-200), "max_distance * max_distance"), (dict(md=1e200), "max_distance * max_distance"),
                     (dict(device=-1), "device"), (dict(device=64), "device"), (dict(P=0, dev_out=1), "P == 0")]:
        rc, msg, index, d2, nfar = _call(**kw)
        assert rc == nat.SC_ERR_INVALID and word in msg, (kw, msg)
        assert index.tolist() == [7] * 16 and d2.tolist() == [7.0] * 16 and nfar[0] == 7  # nothing written
    for bad in (np.nan, np.inf, -np.inf):
        broken = SMOKE_QUERIES.copy()
        broken[1, 1] = bad
        rc, msg, _, _, _ = _call(queries=broken)
        assert rc == nat.SC_ERR_INVALID and "non-finite coordinate in query 1" in msg
        broken = SMOKE_TARGETS.copy()
        broken[4, 0] = bad
        rc, msg, _, _, _ = _call(targets=broken)
        assert rc == nat.SC_ERR_INVALID and "non-finite coordinate in target 4" in msg


def test_empty_clouds_need_no_device():
    rc, _, index, d2, nfar = _call(P=0)  # K4: every place of the two rows unused
    assert rc == nat.SC_OK and index.tolist() == [-1] * 6 + [7] * 10 and np.all(np.isinf(d2[:6])) and d2[6] == 7.0 and nfar[0] == 0
    rc, _, index, _, nfar = _call(Q=0)
    assert rc == nat.SC_OK and index.tolist() == [7] * 16 and nfar[0] == 0
    rc, _, _, _, _ = _call(Q=0, P=0, nulls=("q", "t"), far=False)
    assert rc == nat.SC_OK
    index, d2 = proc3d.knn_points(np.zeros((3, 3)), np.zeros((0, 3)), 4)
    assert index.dtype == np.int32 and index.shape == (3, 4) and np.all(index == -1) and d2.dtype == np.float64 and np.all(np.isinf(d2))
    index, d2, far = proc3d.knn_points(np.zeros((0, 3)), proc3d.PointCloud(np.zeros((4, 3)), None), 2, 1.0, return_far=True)
    assert index.shape == (0, 2) and d2.shape == (0, 2) and far == 0


def test_python_entries_raise_value_error():
    import torch
    for k in (0, -1, nat.SC_KNN_MAX + 1):
        with pytest.raises(ValueError, match="k must be"):
            proc3d.knn_points(SMOKE_QUERIES, SMOKE_TARGETS, k)
    with pytest.raises(ValueError, match="max_distance must be positive"):
        proc3d.knn_points(SMOKE_QUERIES, SMOKE_TARGETS, 3, 0.0)
    with pytest.raises(ValueError, match=r"max_distance \* max_distance"):
        proc3d.knn_points(SMOKE_QUERIES, SMOKE_TARGETS, 3, 1e-200)
    with pytest.raises(ValueError, match="non-finite coordinate in target 1"):
        proc3d.knn_points(SMOKE_QUERIES, proc3d.PointCloud(np.array([[0.0, 0, 0], [0, np.nan, 0]]), None), 3)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        proc3d.knn_points(np.zeros((3, 2)), SMOKE_TARGETS, 3)
    with pytest.raises(ValueError, match="CUDA tensor"):  # a CPU tensor is refused as a device cloud first
        proc3d.knn_points(torch.zeros((3, 3), dtype=torch.float64), SMOKE_TARGETS, 3)

    class FakeDeviceCloud:  # passes for a device tensor as far as the kind check looks
        dtype, is_cuda, shape = torch.float64, True, (3, 3)
        def data_ptr(self): return 0
        def is_contiguous(self): return True
        def dim(self): return 2

    for args in ((FakeDeviceCloud(), SMOKE_TARGETS), (SMOKE_QUERIES, FakeDeviceCloud())):  # mixed kinds
        with pytest.raises(ValueError, match="both be arrays"):
            proc3d.knn_points(*args, 3)
    with pytest.raises(ValueError, match="host points"):
        proc3d.knn_edges(FakeDeviceCloud(), 3)


def test_no_cpu_fallback_without_device():
    try:
        n = nat.device_count()
    except nat.SpaceCarveError:
        n = 0
    if n > 0:  # with a device the call computes (tests/test_knn_gpu.py); nothing to show here
        return
    with pytest.raises(nat.SpaceCarveError):
        proc3d.knn_points(SMOKE_QUERIES, SMOKE_TARGETS, 3)
    with pytest.raises(nat.SpaceCarveError):
        proc3d.knn_edges(SMOKE_TARGETS, 3)


# ---- the host logic over the search, with the checker's search injected -------------------------------------------------
def _cloud():
    rng = np.random.default_rng(23)
    pts = rng.uniform(0.0, 4.0, size=(120, 3))
    pts[100:110] = pts[5:15]  # duplicates
    return np.ascontiguousarray(pts)


def test_knn_edges_dedupe_and_order():
    pts = _cloud()
    seen = []

    def knn_fn(a, b, k):
        seen.append((len(a), len(b), k))
        return oracle.knn_all_pairs(a, b, k)

    edges, weights = proc3d.knn_edges(pts, 6, knn_fn=knn_fn)
    assert seen == [(120, 120, 6)] and edges.dtype == np.int32 and weights.dtype == np.float64
    _, want = oracle.reference_knn_graph(pts, 6)
    pairs = [tuple(e) for e in edges.tolist()]
    assert pairs == sorted(set(pairs)) == sorted(want) and all(a <= b for a, b in pairs)  # deduplicated, lexicographic
    assert all((i, i) in want for i in range(120)) and len(pairs) < 120 * 6  # self-loops; mutual neighbours were folded
    index, d2 = oracle.knn_all_pairs(pts, pts, 6)
    for (a, b), w in zip(pairs, weights.tolist()):
        d = nearest_oracle.dist2(pts[a], pts[b])
        assert w == np.sqrt(d) == np.sqrt(nearest_oracle.dist2(pts[b], pts[a]))  # d2 is bitwise symmetric
        assert abs(w - want[(a, b)]) <= 2.0 ** -50 * w  # np.linalg.norm, see tests/test_knn_gpu.py
    # fewer points than places: the unused places make no edge
    edges, weights = proc3d.knn_edges(pts[:4], 6, knn_fn=knn_fn)
    assert [tuple(e) for e in edges.tolist()] == [(a, b) for a in range(4) for b in range(a, 4)]
    edges, weights = proc3d.knn_edges(np.zeros((0, 3)), 6, knn_fn=knn_fn)
    assert edges.shape == (0, 2) and weights.shape == (0,)
    cloud = proc3d.PointCloud(pts, None)
    assert np.array_equal(proc3d.knn_edges(cloud, 6, knn_fn=knn_fn)[0], proc3d.knn_edges(pts, 6, knn_fn=knn_fn)[0])


def test_knn_graph_with_and_without_networkx(monkeypatch):
    import networkx as nx
    pts = _cloud()
    g = proc3d.knn_graph(proc3d.PointCloud(pts, None), 6, knn_fn=oracle.knn_all_pairs)
    nodes, want = oracle.reference_knn_graph(pts, 6)
    assert isinstance(g, nx.Graph) and not g.is_directed()
    assert sorted(g.nodes) == sorted(nodes) and all(np.array_equal(g.nodes[i]["center"], nodes[i]) for i in nodes)
    assert sorted((min(a, b), max(a, b)) for a, b in g.edges) == sorted(want)
    assert all(abs(g.edges[e]["weight"] - w) <= 2.0 ** -50 * w for e, w in want.items())
    real_import = builtins.__import__

    def hidden(name, *args, **kwargs):
        if name == "networkx" or name.startswith("networkx."):
            raise ImportError("No module named 'networkx'")
        return real_import(name, *args, **kwargs)

    monkeypatch.setattr(builtins, "__import__", hidden)
    with pytest.raises(ImportError, match="knn_graph needs networkx"):
        proc3d.knn_graph(pts, 6, knn_fn=oracle.knn_all_pairs)
