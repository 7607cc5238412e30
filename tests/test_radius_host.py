"""CPU: the radius checker itself (tests/radius_oracle.py, its two forms against each other), the argument errors of
``sc_radius`` that need no device, and the host logic of ``radius_edges`` / ``radius_graph`` with the checker's search
injected."""
import builtins

import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import proc3d
from tests import dbscan_oracle
from tests import nearest_oracle
from tests import radius_oracle as oracle

# the hand-worked case of __graft_entry__.smoke(): six targets (2 and 3 coincide), three queries, radius 2.  Query 0 has
# d2 = 0, 4, 1, 1, 2.25, 300: target 1 lies at exactly the radius and is out, the coincident pair stands in rising
# index.  Query 1 has d2 = 1, 1, 0, 0, 3.25, 262: two ties of two.  Query 2 has nothing within 2.
SMOKE_TARGETS = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0], [1, 0, 0], [0, 1.5, 0], [10, 10, 10]], dtype=np.float64)
SMOKE_QUERIES = np.array([[0, 0, 0], [1, 0, 0], [5, 5, 5]], dtype=np.float64)
SMOKE_OFFSETS, SMOKE_INDEX, SMOKE_D2 = [0, 4, 9, 9], [0, 2, 3, 4, 2, 3, 0, 1, 4], [0.0, 1.0, 1.0, 2.25, 0.0, 0.0, 1.0, 1.0, 3.25]


def same(got, want):
    return all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want)) and len(got) == len(want)


# ---- the checker --------------------------------------------------------------------------------------------------
def test_hand_worked_case():
    for fn in (oracle.radius, oracle.radius_all_pairs):
        offsets, index, d2 = fn(SMOKE_QUERIES, SMOKE_TARGETS, 2.0)
        assert offsets.dtype == np.int64 and index.dtype == np.int32 and d2.dtype == np.float64
        assert offsets.tolist() == SMOKE_OFFSETS and index.tolist() == SMOKE_INDEX and d2.tolist() == SMOKE_D2
        offsets, index, d2 = fn(SMOKE_QUERIES, SMOKE_TARGETS, np.nextafter(2.0, 3.0))  # the target at exactly 2 comes in
        assert offsets.tolist() == [0, 5, 10, 10] and index[:5].tolist() == [0, 2, 3, 4, 1] and d2[4] == 4.0
        offsets, index, d2 = fn(SMOKE_QUERIES, SMOKE_TARGETS, 1.0)  # strict: the targets at exactly 1 are out
        assert offsets.tolist() == [0, 1, 3, 3] and index.tolist() == [0, 2, 3] and d2.tolist() == [0.0, 0.0, 0.0]
        assert oracle.counts(offsets).tolist() == [1, 2, 0] and oracle.counts(offsets).dtype == np.int32


def test_tree_form_equals_all_pairs_on_ties_and_duplicates():
    queries, targets = nearest_oracle.tie_clouds()
    for shift, sign in (((0.0, 0.0, 0.0), 1.0), ((1e6, -1e6, 0.5), 1.0), ((0.0, 0.0, 0.0), -1.0)):
        q, t = sign * queries + np.array(shift), sign * targets + np.array(shift)
        for r in (0.25, 0.5, np.sqrt(0.75), 1.0, 2.0, 20.0):  # 0.5, 1 and 2 are distances of the lattice: strictness decides
            assert same(oracle.radius(q, t, r), oracle.radius_all_pairs(q, t, r)), (shift, sign, r)
    offsets, index, d2 = oracle.radius_all_pairs(queries, targets, 0.9)
    lengths = np.diff(offsets)[:80]  # the cell centres: 8-way ties, 11-way where a corner has its three extra copies
    assert set(lengths.tolist()) == {8, 11} and np.all(d2[:offsets[80]] == 0.75)
    assert all(np.all(np.diff(index[offsets[k]:offsets[k + 1]]) > 0) for k in range(80))  # equal d2: rising index
    assert np.all(np.diff(oracle.radius_all_pairs(queries, targets, 0.5)[0])[80:150] == 0)  # edge midpoints: exactly 0.5 is out
    assert np.all(np.diff(oracle.radius_all_pairs(queries, targets, 20.0)[0]) == len(targets))  # the one-sort branch
    # duplicates: 300 copies of one point
    copies = np.tile([[1.25, -2.5, 0.75]], (300, 1))
    for fn in (oracle.radius, oracle.radius_all_pairs):
        offsets, index, d2 = fn(copies[:7], copies, 1e-3)
        assert offsets.tolist() == [300 * k for k in range(8)] and np.array_equal(index, np.tile(np.arange(300, dtype=np.int32), 7)) and np.all(d2 == 0.0)
    blobs = dbscan_oracle.blobs_cloud()[:600]
    targets = nearest_oracle.blob_targets(blobs)
    assert same(oracle.radius(blobs, targets, 1.5), oracle.radius_all_pairs(blobs, targets, 1.5))
    for fn in (oracle.radius, oracle.radius_all_pairs):
        offsets, index, d2 = fn(np.zeros((3, 3)), np.zeros((0, 3)), 4.0)
        assert offsets.tolist() == [0, 0, 0, 0] and index.shape == (0,) and d2.shape == (0,)
        offsets, index, d2 = fn(np.zeros((0, 3)), np.zeros((3, 3)), 4.0)
        assert offsets.tolist() == [0] and offsets.dtype == np.int64 and index.dtype == np.int32 and index.shape == (0,)


# ---- sc_radius: judged before any device call ---------------------------------------------------------------------------
def _call(Q=3, P=6, radius=2.0, queries=SMOKE_QUERIES, targets=SMOKE_TARGETS, nulls=(), device=0, dev_out=0, capacity=16, long=True):
    b = nat.backend()
    out = {"counts": np.full(16, 7, dtype=np.int32), "offsets": np.full(16, 7, dtype=np.int64), "index": np.full(16, 7, dtype=np.int32),
           "d2": np.full(16, 7.0), "total": np.full(1, 7, dtype=np.int64), "long": np.full(1, 7, dtype=np.int64)}
    ptr = {name: 0 if name in nulls else nat.addr(a) for name, a in (("q", queries), ("t", targets), *out.items())}
    rc = b.call("sc_radius", ptr["q"], 0, int(Q), ptr["t"], 0, int(P), float(radius), device, ptr["counts"], ptr["offsets"], ptr["index"], ptr["d2"],
                int(capacity), dev_out, ptr["total"], ptr["long"] if long else 0, 0)
    return rc, b.string(b.call("sc_nearest_last_error")), out


def _untouched(out):
    return all(np.all(a == 7) for a in out.values())


def test_radius_argument_errors_need_no_device():
    for kw, word in [(dict(radius=0.0), "radius must be finite and positive"), (dict(radius=-1.0), "radius must be finite and positive"),
                     (dict(radius=float("nan")), "radius must be finite and positive"), (dict(radius=float("inf")), "radius must be finite and positive"),
                     (dict(radius=1e-200), "radius * radius"), (dict(radius=1e200), "radius * radius"),
                     (dict(Q=-1), "Q must be"), (dict(Q=2 ** 31), "Q must be"), (dict(P=-1), "P must be"), (dict(P=2 ** 40), "P must be"),
                     (dict(nulls=("q",)), "null"), (dict(nulls=("t",)), "null"), (dict(nulls=("total",)), "null"),
                     (dict(nulls=("index",)), "both or neither"), (dict(nulls=("d2",)), "both or neither"), (dict(capacity=-1), "capacity"),
                     (dict(device=-1), "device"), (dict(device=64), "device"),
                     (dict(P=0, dev_out=1), "makes no device call"), (dict(Q=0, dev_out=1), "makes no device call")]:
        rc, msg, out = _call(**kw)
        assert rc == nat.SC_ERR_INVALID and word in msg, (kw, msg)
        assert _untouched(out), kw  # nothing written
    for bad in (np.nan, np.inf, -np.inf):
        broken = SMOKE_QUERIES.copy()
        broken[1, 1] = bad
        rc, msg, out = _call(queries=broken)
        assert rc == nat.SC_ERR_INVALID and "non-finite coordinate in query 1" in msg and _untouched(out)
        broken = SMOKE_TARGETS.copy()
        broken[4, 0] = bad
        rc, msg, out = _call(targets=broken)
        assert rc == nat.SC_ERR_INVALID and "non-finite coordinate in target 4" in msg and _untouched(out)


def test_empty_clouds_need_no_device():
    rc, _, out = _call(P=0)  # R4: every count 0
    assert rc == nat.SC_OK and out["counts"].tolist() == [0] * 3 + [7] * 13 and out["offsets"].tolist() == [0] * 4 + [7] * 12
    assert out["total"][0] == 0 and out["long"][0] == 0 and np.all(out["index"] == 7) and np.all(out["d2"] == 7.0)
    rc, _, out = _call(Q=0)
    assert rc == nat.SC_OK and out["offsets"].tolist() == [0] + [7] * 15 and np.all(out["counts"] == 7) and out["total"][0] == 0
    rc, _, out = _call(Q=0, P=0, nulls=("q", "t", "counts", "offsets", "index", "d2"), long=False)
    assert rc == nat.SC_OK and out["total"][0] == 0 and out["long"][0] == 7
    offsets, index, d2 = proc3d.radius_points(np.zeros((3, 3)), np.zeros((0, 3)), 4.0)
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 0, 0, 0] and index.dtype == np.int32 and index.shape == (0,) and d2.dtype == np.float64
    offsets, index, d2, nlong = proc3d.radius_points(np.zeros((0, 3)), proc3d.PointCloud(np.zeros((4, 3)), None), 1.0, return_long=True)
    assert offsets.tolist() == [0] and index.shape == (0,) and d2.shape == (0,) and nlong == 0
    counts = proc3d.radius_counts(np.zeros((3, 3)), np.zeros((0, 3)), 4.0)
    assert counts.dtype == np.int32 and counts.tolist() == [0, 0, 0]
    assert proc3d.radius_counts(np.zeros((0, 3)), np.zeros((5, 3)), 4.0).shape == (0,)


def test_python_entries_raise_value_error():
    import torch
    for r in (0.0, -2.0, float("nan"), float("inf")):
        for fn in (proc3d.radius_points, proc3d.radius_counts):
            with pytest.raises(ValueError, match="radius must be positive and finite"):
                fn(SMOKE_QUERIES, SMOKE_TARGETS, r)
    with pytest.raises(ValueError, match=r"radius \* radius"):
        proc3d.radius_points(SMOKE_QUERIES, SMOKE_TARGETS, 1e-200)
    with pytest.raises(ValueError, match="non-finite coordinate in target 1"):
        proc3d.radius_points(SMOKE_QUERIES, proc3d.PointCloud(np.array([[0.0, 0, 0], [0, np.nan, 0]]), None), 3.0)
    with pytest.raises(ValueError, match="non-finite coordinate in query 2"):
        proc3d.radius_counts(np.array([[0.0, 0, 0], [0, 1, 0], [np.inf, 0, 0]]), SMOKE_TARGETS, 3.0)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        proc3d.radius_points(np.zeros((3, 2)), SMOKE_TARGETS, 3.0)
    with pytest.raises(ValueError, match="CUDA tensor"):  # a CPU tensor is refused as a device cloud first
        proc3d.radius_points(torch.zeros((3, 3), dtype=torch.float64), SMOKE_TARGETS, 3.0)

    class FakeDeviceCloud:  # passes for a device tensor as far as the kind check looks
        dtype, is_cuda, shape = torch.float64, True, (3, 3)
        def data_ptr(self): return 0
        def is_contiguous(self): return True
        def dim(self): return 2

    for args in ((FakeDeviceCloud(), SMOKE_TARGETS), (SMOKE_QUERIES, FakeDeviceCloud())):  # mixed kinds
        for fn in (proc3d.radius_points, proc3d.radius_counts):
            with pytest.raises(ValueError, match="both be arrays"):
                fn(*args, 3.0)
    with pytest.raises(ValueError, match="host points"):
        proc3d.radius_edges(FakeDeviceCloud(), 3.0)


def test_no_cpu_fallback_without_device():
    try:
        n = nat.device_count()
    except nat.SpaceCarveError:
        n = 0
    if n > 0:  # with a device the call computes (tests/test_radius_gpu.py); nothing to show here
        return
    for fn in (proc3d.radius_points, proc3d.radius_counts, proc3d.radius_edges):
        with pytest.raises(nat.SpaceCarveError):
            fn(SMOKE_QUERIES, SMOKE_TARGETS, 2.0) if fn is not proc3d.radius_edges else fn(SMOKE_TARGETS, 2.0)


def test_the_unit_keeps_its_getters_and_releases():
    assert proc3d.RELEASES == ("sc_vol2pcd_release", "sc_dbscan_release", "sc_eval_release", "sc_select_release", "sc_nearest_release")
    assert "sc_radius" not in nat.UNIT_ERRORS and "sc_knn" not in nat.UNIT_ERRORS
    assert sorted(set(nat.UNIT_ERRORS.values())) == sorted(
        ["sc_vol2pcd_last_error", "sc_label_points_last_error", "sc_masks_last_error", "sc_undistort_last_error", "sc_dbscan_last_error",
         "sc_eval_last_error", "sc_select_last_error", "sc_nearest_last_error"])
    assert len(nat.UNIT_ERRORS) == 12
    assert "sc_radius" in nat.EXPORTED_SYMBOLS and "sc_radius_last_error" not in nat.EXPORTED_SYMBOLS and "sc_radius_release" not in nat.EXPORTED_SYMBOLS
    assert nat.SC_RADIUS_LDS_ROW == 1024
    import os, re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spacecarve.h")).read()
    assert int(re.search(r"#define SC_RADIUS_LDS_ROW (\d+)", text).group(1)) == nat.SC_RADIUS_LDS_ROW


# ---- the host logic over the search, with the checker's search injected -------------------------------------------------
def _cloud():
    rng = np.random.default_rng(23)
    pts = rng.uniform(0.0, 4.0, size=(120, 3))
    pts[100:110] = pts[5:15]  # duplicates
    return np.ascontiguousarray(pts)


def test_radius_edges_dedupe_and_order():
    pts = _cloud()
    seen = []

    def radius_fn(a, b, r):
        seen.append((len(a), len(b), r))
        return oracle.radius_all_pairs(a, b, r)

    edges, weights = proc3d.radius_edges(pts, 0.9, radius_fn=radius_fn)
    assert seen == [(120, 120, 0.9)] and edges.dtype == np.int32 and weights.dtype == np.float64
    _, want = oracle.reference_radius_graph(pts, 0.9)
    pairs = [tuple(e) for e in edges.tolist()]
    offsets = oracle.radius_all_pairs(pts, pts, 0.9)[0]
    assert pairs == sorted(set(pairs)) == sorted(want) and all(a <= b for a, b in pairs)  # deduplicated, lexicographic
    assert all((i, i) in want for i in range(120)) and 120 < len(pairs) == (offsets[-1] + 120) // 2  # self-loops; both directions folded
    assert all((5 + k, 100 + k) in want and want[(5 + k, 100 + k)] == 0.0 for k in range(10))  # a duplicate is a neighbour at 0
    for (a, b), w in zip(pairs, weights.tolist()):
        d = nearest_oracle.dist2(pts[a], pts[b])
        assert d < 0.9 * 0.9 and w == np.sqrt(d) == np.sqrt(nearest_oracle.dist2(pts[b], pts[a]))  # d2 is bitwise symmetric
        assert abs(w - want[(a, b)]) <= 2.0 ** -50 * w  # np.linalg.norm, see tests/test_knn_gpu.py
    edges, weights = proc3d.radius_edges(pts[:4], 100.0, radius_fn=radius_fn)  # everything within the radius: all pairs
    assert [tuple(e) for e in edges.tolist()] == [(a, b) for a in range(4) for b in range(a, 4)]
    edges, weights = proc3d.radius_edges(pts, 1e-6, radius_fn=radius_fn)  # only the self-loops and the duplicates
    assert len(edges) == 130 and np.all(weights == 0.0)
    edges, weights = proc3d.radius_edges(np.zeros((0, 3)), 1.0, radius_fn=radius_fn)
    assert edges.shape == (0, 2) and edges.dtype == np.int32 and weights.shape == (0,)
    cloud = proc3d.PointCloud(pts, None)
    assert np.array_equal(proc3d.radius_edges(cloud, 0.9, radius_fn=radius_fn)[0], proc3d.radius_edges(pts, 0.9, radius_fn=radius_fn)[0])


def test_radius_graph_with_and_without_networkx(monkeypatch):
    import networkx as nx
    pts = _cloud()
    g = proc3d.radius_graph(proc3d.PointCloud(pts, None), 0.9, radius_fn=oracle.radius_all_pairs)
    nodes, want = oracle.reference_radius_graph(pts, 0.9)
    assert isinstance(g, nx.Graph) and not g.is_directed()
    assert sorted(g.nodes) == nodes == list(range(120)) and all(g.nodes[i] == {} for i in nodes)  # no `center`, no attribute at all
    assert sorted((min(a, b), max(a, b)) for a, b in g.edges) == sorted(want)
    assert all(abs(g.edges[e]["weight"] - w) <= 2.0 ** -50 * w for e, w in want.items())
    assert all(set(g.edges[e]) == {"weight"} for e in g.edges)
    lone = proc3d.radius_graph(pts, 1e-9, radius_fn=oracle.radius)  # isolated points are nodes all the same
    assert lone.number_of_nodes() == 120 and lone.number_of_edges() == 130
    real_import = builtins.__import__

    def hidden(name, *args, **kwargs):
        if name == "networkx" or name.startswith("networkx."):
            raise ImportError("No module named 'networkx'")
        return real_import(name, *args, **kwargs)

    monkeypatch.setattr(builtins, "__import__", hidden)
    with pytest.raises(ImportError, match="radius_graph needs networkx"):
        proc3d.radius_graph(pts, 0.9, radius_fn=oracle.radius_all_pairs)
