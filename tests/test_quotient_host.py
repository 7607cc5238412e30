"""CPU: the checker of ``sc_graph_quotient`` (tests/quotient_oracle.py) held against ``nx.quotient_graph`` and
``nx.minimum_spanning_tree`` -- what the reference's XU skeleton calls (plant3dvision/proc3d.py:323, :425) -- and what the
library and ``proc3d.graph_quotient`` refuse and do without a device."""
import ctypes

import networkx as nx
import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import proc3d
from tests import graph_oracle
from tests import quotient_oracle as oracle


def _blobs():
    """The five-blob cloud of tests/test_graph_gpu.py."""
    rng = np.random.default_rng(8)
    centres = np.array([[0, 0, 0], [6, 0, 0], [0, 7, 0], [5, 5, 5], [-6, 1, 2]], dtype=np.float64)
    return np.concatenate([c + rng.uniform(-1.0, 1.0, size=(40, 3)) for c in centres])


@pytest.fixture(scope="module")
def blob_case():
    """k = 5, root 7, bins of 0.8, connected: rows from cKDTree, everything before the quotient from tests/graph_oracle.py."""
    pts = _blobs()
    rows = oracle.d2_rows_knn(pts, 5)
    labels, _ = graph_oracle.components(rows)
    extra = graph_oracle.connect_edges(pts, labels, 7)
    d = graph_oracle.distances(rows, 7, extra)
    bins = graph_oracle.bins_of(d, 0.8)
    labels, count = graph_oracle.components(rows, bins, extra)
    got = oracle.quotient(rows, labels, count, points=pts, key=bins, extra=extra, weights=True)
    g = nx.Graph()
    g.add_nodes_from(range(len(pts)))
    for i, j, w in oracle.arcs_of(rows, extra)[1]:
        g.add_edge(i, j, weight=w)
    cluster = got[0]
    sets = [frozenset(np.flatnonzero(cluster == c).tolist()) for c in range(len(got[1]))]
    return pts, rows, extra, got, nx.quotient_graph(g, sets, relabel=True)


def test_checker_edges_and_weights_equal_networkx(blob_case):
    pts, rows, extra, (cluster, counts, centers, edges, edge_w), q = blob_case
    assert len(counts) == 46 and len(edges) == 64 and (cluster >= 0).all()
    assert sorted((min(a, b), max(a, b)) for a, b in q.edges()) == [tuple(e) for e in edges.tolist()]
    terms = oracle.pairs_per_edge(rows, cluster, extra)
    worst = 0.0
    for (a, b), w in zip(edges.tolist(), edge_w.tolist()):
        want = q[a][b]["weight"]
        n = terms[(a, b)]
        assert abs(w - want) <= 2 * n * 2.0 ** -53 * want, (a, b, w, want)  # two orders of one sum of n non-negative terms
        worst = max(worst, abs(w - want) / want)
    print(f"largest relative difference from networkx's weights: {worst:.3g}")
    for c in range(len(counts)):  # Q2 is np.bincount's sum
        members = cluster == c
        for a in range(3):
            assert centers[c, a] == np.bincount(np.zeros(counts[c], dtype=np.int64), weights=pts[members, a])[0] / float(counts[c])


def test_weighted_tree_is_networkx_tree_and_the_unweighted_is_not(blob_case):
    _, _, _, (cluster, counts, centers, edges, edge_w), q = blob_case
    want = sorted((min(a, b), max(a, b)) for a, b in nx.minimum_spanning_tree(q).edges())
    g = nx.Graph()
    g.add_nodes_from(range(len(counts)))
    g.add_weighted_edges_from((a, b, w) for (a, b), w in zip(edges.tolist(), edge_w.tolist()))
    assert sorted((min(a, b), max(a, b)) for a, b in nx.minimum_spanning_tree(g).edges()) == want
    u = nx.Graph()
    u.add_nodes_from(range(len(counts)))
    u.add_edges_from(map(tuple, edges.tolist()))
    assert sorted((min(a, b), max(a, b)) for a, b in nx.minimum_spanning_tree(u).edges()) != want


# ---- the whole-array checker of the large GPU cases against the loops -------------------------------------------------
def _np_cases():
    """name -> the arguments of ``quotient``: every form of input tests/test_quotient_gpu.py feeds, at small sizes."""
    rng = np.random.default_rng(61)
    out = {}
    for n in (1, 2, 65, 300):
        pts = rng.uniform(0.0, 1.0, size=(n, 3))
        slab = (pts[:, 0] * 3).astype(np.int32)
        slab[rng.random(n) < 0.1] = -1  # outside nodes
        key = rng.integers(-5, 5, size=n).astype(np.int32)  # keys with negatives
        for name, rows in (("knn", oracle.d2_rows_knn(pts, 5)), ("csr", graph_oracle.radius_rows(pts, 1.2 * (1.0 / n) ** (1.0 / 3.0)))):
            labels, count = graph_oracle.components(rows, slab)
            out[f"{name} {n} slabs, key"] = dict(rows=rows, labels=labels, n_labels=count, points=pts, key=key)
            out[f"{name} {n} slabs"] = dict(rows=rows, labels=labels, n_labels=count)
    n, n_labels = 300, 40
    pts = rng.uniform(0.0, 1.0, size=(n, 3))
    names = rng.permutation(n_labels)[:25]  # 15 labels stay empty
    labels = names[rng.integers(0, 25, size=n)].astype(np.int32)
    labels[rng.random(n) < 0.1] = -1
    labels[0] = -3
    rows = oracle.d2_rows_knn(pts, 6)
    out["labels in any order, empty ones"] = dict(rows=rows, labels=labels, n_labels=n_labels, points=pts)
    out["labels in any order, wide keys"] = dict(rows=rows, labels=labels, n_labels=n_labels, points=pts,
                                                 key=rng.integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32))
    out["every node its own cluster"] = dict(rows=rows, labels=np.arange(n, dtype=np.int32), n_labels=n, points=pts)
    out["one cluster"] = dict(rows=rows, labels=np.zeros(n, dtype=np.int32), n_labels=3, points=pts)
    out["nobody inside"] = dict(rows=rows, labels=np.full(n, -1, dtype=np.int32), n_labels=5, points=pts, key=np.zeros(n, np.int32))
    out["no labels offered"] = dict(rows=rows, labels=np.full(n, -1, dtype=np.int32), n_labels=0)
    inf, tiny = np.inf, 5e-324
    index = np.array([[2, -1, 0], [2, -1, -1], [1, -1, -1], [1, 3, -1], [-1, -1, -1]], dtype=np.int32)  # the hand-made rows
    d2 = np.array([[16.0, inf, 0.0], [9.0, inf, inf], [4.0, inf, inf], [25.0, 0.0, inf], [inf, inf, inf]])
    extra = (np.array([[4, 0], [3, 4], [4, 3], [4, 4], [2, 1]], dtype=np.int32), np.array([0.5, 7.0, 6.0, 1.0, 1.5]))  # repeated pairs
    out["hand-made rows"] = dict(rows=(index, d2), labels=np.array([0, 0, 1, 1, 2], dtype=np.int32), n_labels=3)
    out["hand-made rows, extras"] = dict(rows=(index, d2), labels=np.array([0, 0, 1, 1, 2], dtype=np.int32), n_labels=3, extra=extra)
    out["hand-made csr, extras, key"] = dict(rows=(np.array([0, 2, 3, 4, 6, 6], dtype=np.int64), np.array([2, 0, 2, 1, 1, 3], dtype=np.int32),
                                                   np.array([16.0, 0.0, 9.0, 4.0, 25.0, 0.0])),
                                             labels=np.array([0, 0, 1, 1, 2], dtype=np.int32), n_labels=3, key=np.array([5, 5, 0, 0, -1], np.int32),
                                             extra=extra)
    out["no arcs, csr"] = dict(rows=(np.zeros(66, np.int64), np.zeros(0, np.int32), np.zeros(0)), labels=np.arange(65, dtype=np.int32), n_labels=65,
                               points=rng.normal(size=(65, 3)))
    out["extras alone"] = dict(rows=(np.full((65, 2), -1, np.int32), np.full((65, 2), inf)), labels=np.arange(65, dtype=np.int32), n_labels=65,
                               extra=(np.array([[0, 64], [64, 0], [7, 3]], dtype=np.int32), np.array([2.0, 1.0, 3.0])))
    pts = np.array([[1e16, tiny, 1.0], [1.0, tiny, np.nan], [-1e16, -tiny, 2.0], [-0.0, tiny, 3.0],  # test_the_order_of_summation_shows
                    [1.0, 1e-310, -0.0], [1e16, 2e-310, -0.0], [-1e16, -3e-310, -0.0], [-0.0, -0.0, 1e308], [-0.0, -0.0, 1e308]])
    out["the order of summation shows"] = dict(rows=(np.array([[1], [2], [3], [4], [5], [6], [7], [8], [0]], dtype=np.int32), np.ones((9, 1))),
                                               labels=np.array([2, 2, 2, 2, 5, 5, 5, 7, 7], dtype=np.int32), n_labels=8, points=pts)
    # a few thousand arcs whose weights span 30 decades, many per cluster pair: every order of a sum gives other bits
    n = 400
    index = rng.integers(0, n, size=(n, 12)).astype(np.int32)
    index[rng.random(index.shape) < 0.05] = -1
    out["heavy-tailed weights"] = dict(rows=(index, 10.0 ** rng.uniform(-30.0, 30.0, size=index.shape)), labels=rng.integers(-1, 6, size=n).astype(np.int32),
                                       n_labels=6, points=rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-8.0, 8.0, size=(n, 3)),
                                       key=rng.integers(-3, 3, size=n).astype(np.int32),
                                       extra=(rng.integers(0, n, size=(500, 2)).astype(np.int32), 10.0 ** rng.uniform(-30.0, 30.0, size=500)))
    return out


NP_CASES = _np_cases()


@pytest.mark.parametrize("name", sorted(NP_CASES))
def test_the_array_checker_equals_the_loops(name):
    case = NP_CASES[name]
    want = oracle.quotient(weights=True, **case)
    got = oracle.quotient_np(weights=True, **case)
    for what, a, b in zip(("cluster", "counts", "centers", "edges", "edge weights"), got, want):
        assert (a is None and b is None) or oracle.same_bits(a, b), what
    assert oracle.quotient_np(weights=False, **case)[4] is None
    crossing = sum(1 for i, j, _ in oracle.arcs_of(case["rows"], case.get("extra"))[1] if want[0][i] >= 0 and want[0][j] >= 0 and want[0][i] != want[0][j])
    assert oracle.crossing_np(case["rows"], want[0], case.get("extra")) == crossing
    if name == "heavy-tailed weights":  # the order shows: the same terms summed from the other end give other bits
        assert len(want[3]) == 15 and crossing > 3000
        terms = oracle.node_edges(oracle.arcs_of(case["rows"], case["extra"])[1])
        back = {}
        for (i, j), w in sorted(terms.items(), reverse=True):
            a, b = sorted((int(want[0][i]), int(want[0][j])))
            if a >= 0 and a != b:
                back[(a, b)] = back.get((a, b), 0.0) + w
        assert any(back[tuple(e)] != w for e, w in zip(want[3].tolist(), want[4].tolist()))


# ---- what the library refuses without a device (rule Q6) ------------------------------------------------------------
INDEX =np.array([[1, -1], [0, 2], [1, -1]], dtype=np.int32)
D2 = np.array([[1.0, np.inf], [1.0, 4.0], [4.0, np.inf]])
ROWS = (INDEX, D2)


def test_argument_errors_of_the_library_need_no_device():
    b = nat.backend()
    labels, cluster, counts = np.array([0, 0, 1], np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)
    points, centers = np.zeros((3, 3)), np.zeros((3, 3))
    edges, edge_w = np.zeros((4, 2), np.int32), np.zeros(4)
    nc, ne = np.zeros(1, np.int32), np.zeros(1, np.int64)
    given = dict(N=3, offsets=0, row_len=2, index=nat.addr(INDEX), weights=nat.addr(D2), E=6, squared=1, extra=0, extra_w=0, M=0,
                 labels=nat.addr(labels), L=2, key=0, points=nat.addr(points), on_device=0, device=0, cluster=nat.addr(cluster),
                 counts=nat.addr(counts), centers=nat.addr(centers), edges=nat.addr(edges), edge_w=nat.addr(edge_w), capacity=4,
                 nc=nat.addr(nc), ne=nat.addr(ne), stream=0)

    def refused(text, **change):
        args = dict(given, **change)
        rc = b.call("sc_graph_quotient", *args.values())
        said = b.string(b.call("sc_graph_error"))
        assert rc == nat.SC_ERR_INVALID and text in said, (change, rc, said)

    refused("null", nc=0)
    refused("null", ne=0)
    refused("null", labels=0)
    refused("null", cluster=0)
    refused("null", counts=0)
    refused("null", centers=0)
    refused("L must be", L=-1)
    refused("L must be", L=4)
    bad = np.array([0, 2, 1], np.int32)
    refused("label outside", labels=nat.addr(bad))
    refused("capacity", capacity=-1)
    refused("capacity", edges=0, edge_w=0)
    refused("edge_w_out without edges_out", edges=0, capacity=0)
    refused("null argument (index, weights)", weights=0)  # edge_w_out without weights
    pair, pw = np.array([[0, 2]], np.int32), np.array([1.0])
    refused("null argument (extra, extra_w)", extra=nat.addr(pair), M=1)
    refused("extra pair", extra=nat.addr(np.array([[0, 3]], np.int32)), extra_w=nat.addr(pw), M=1)
    refused("device ordinal", device=64)
    refused("row_len", E=5)
    refused("N must be", N=2 ** 31, E=2 ** 32)
    refused("index outside", index=nat.addr(np.array([[1, -1], [0, 3], [1, -1]], np.int32)))
    for w in (np.nan, -1.0, np.inf):
        d2 = D2.copy()
        d2[1, 1] = w
        refused("weights must be finite", weights=nat.addr(d2))
    o = np.array([0, 1, 3, 3], np.int64)
    flat_i, flat_w = np.array([1, 0, 2, 1], np.int32), np.ones(4)
    refused("offsets must rise", offsets=nat.addr(o), row_len=0, index=nat.addr(flat_i), weights=nat.addr(flat_w), E=4)
    # no nodes: no device call, C = K = 0
    nc[0], ne[0] = 7, 7
    args = dict(given, N=0, E=0, L=0)
    assert b.call("sc_graph_quotient", *args.values()) == nat.SC_OK and nc[0] == 0 and ne[0] == 0
    assert "sc_graph_quotient" in nat.EXPORTED_SYMBOLS


def test_weights_are_not_judged_without_edge_weights():
    """Rule Q6: a NaN weight is refused only when edge_w_out is given; without it the call goes on to the device (and
    fails there when there is none: anything but SC_ERR_INVALID)."""
    b = nat.backend()
    d2 = D2.copy()
    d2[1, 1] = np.nan
    labels, cluster, counts = np.array([0, 0, 1], np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)
    edges, edge_w = np.zeros((4, 2), np.int32), np.zeros(4)
    nc, ne = np.zeros(1, np.int32), np.zeros(1, np.int64)

    def ask(with_weights):
        return b.call("sc_graph_quotient", 3, 0, 2, nat.addr(INDEX), nat.addr(d2), 6, 1, 0, 0, 0, nat.addr(labels), 2, 0, 0, 0, 0,
                      nat.addr(cluster), nat.addr(counts), 0, nat.addr(edges), nat.addr(edge_w) if with_weights else 0, 4, nat.addr(nc),
                      nat.addr(ne), 0)

    assert ask(True) == nat.SC_ERR_INVALID and "weights must be finite" in b.string(b.call("sc_graph_error"))
    try:
        have_device = nat.device_count() > 0
    except nat.SpaceCarveError:
        have_device = False
    rc = ask(False)
    assert rc == nat.SC_OK if have_device else rc not in (nat.SC_OK, nat.SC_ERR_INVALID)


# ---- the Python wrapper without a device ----------------------------------------------------------------------------
def test_python_refusals():
    import torch
    labels = np.array([0, 0, 1], np.int32)
    with pytest.raises(ValueError, match="all arrays or all CUDA tensors"):
        proc3d.graph_quotient(ROWS, torch.zeros(3, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="all arrays or all CUDA tensors"):
        proc3d.graph_quotient(ROWS, labels, 2, key=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="all arrays or all CUDA tensors"):
        proc3d.graph_quotient(ROWS, labels, 2, points=torch.zeros((3, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="all arrays or all CUDA tensors"):
        proc3d.graph_quotient(ROWS, labels, 2, extra=(torch.zeros((1, 2), dtype=torch.int32), np.zeros(1)))
    with pytest.raises(ValueError, match="one label per node"):
        proc3d.graph_quotient(ROWS, labels[:2], 2)
    with pytest.raises(ValueError, match="one key per node"):
        proc3d.graph_quotient(ROWS, labels, 2, key=np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="one point per node"):
        proc3d.graph_quotient(ROWS, labels, 2, points=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="points must be"):
        proc3d.graph_quotient(ROWS, labels, 2, points=np.zeros((3, 2)))
    for bad in (-1, 4):
        with pytest.raises(ValueError, match="n_labels must be 0 .. 3"):
            proc3d.graph_quotient(ROWS, labels, bad)
    with pytest.raises(ValueError):
        proc3d.graph_quotient((INDEX,), labels, 2)


class _Stub:
    """Answers SC_OK; ``edges`` is the K it reports through nedges_out, ``clusters`` the C."""

    def __init__(self, edges=0, clusters=0):
        self.asked, self.edges, self.clusters = [], edges, clusters

    def call(self, name, *args):
        self.asked.append((name,) + args)
        if name == "sc_graph_quotient":
            ctypes.c_int32.from_address(args[-3]).value = self.clusters
            ctypes.c_int64.from_address(args[-2]).value = self.edges
        return nat.SC_OK

    @staticmethod
    def string(ret):
        return ""


def test_no_nodes_no_native_call(monkeypatch):
    stub = _Stub()
    monkeypatch.setattr(nat, "_backend", stub)
    for rows in ((np.zeros((0, 4), np.int32), np.zeros((0, 4))), (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0))):
        cluster, counts, centers, edges, edge_w = proc3d.graph_quotient(rows, np.zeros(0, np.int32), 0, points=np.zeros((0, 3)), weights=True)
        assert cluster.shape == (0,) and cluster.dtype == np.int32 and counts.shape == (0,) and counts.dtype == np.int32
        assert centers.shape == (0, 3) and edges.shape == (0, 2) and edges.dtype == np.int32 and edge_w.shape == (0,)
        got = proc3d.graph_quotient(rows, np.zeros(0, np.int32), 0)
        assert got[2] is None and got[4] is None
        got = proc3d.distance_to_root_clusters(np.zeros((0, 3)), rows, 0, 1.0, weights=True)
        assert len(got) == 5 and got[4].shape == (0,) and got[2].shape == (0, 2)
    assert stub.asked == []


def test_weighted_clusters_refuse_bins_that_do_not_fit_int32(monkeypatch):
    """The weighted form goes through the same bins: refused before any device call, accepted at 2^31 bins exactly."""
    stub = _Stub(edges=0, clusters=1)
    monkeypatch.setattr(nat, "_backend", stub)
    monkeypatch.setattr(proc3d, "graph_distances", lambda rows, root, **kw: np.array([0.0, 1.0, 0.5]))
    for bad in (1e-12, 5e-324, np.nextafter(2.0 ** -31, 0.0)):
        with pytest.raises(ValueError, match="bin_size"):
            proc3d.distance_to_root_clusters(np.zeros((3, 3)), ROWS, 0, bad, weights=True)
    assert stub.asked == []
    keys = []
    components = proc3d.graph_components
    monkeypatch.setattr(proc3d, "graph_components", lambda rows, key=None, **kw: (keys.append(np.array(key)), components(rows, key=key, **kw))[1])
    out = proc3d.distance_to_root_clusters(np.zeros((3, 3)), ROWS, 0, 2.0 ** -31, weights=True)
    assert len(out) == 5 and keys[0].dtype == np.int32 and keys[0].tolist() == [0, 2 ** 31 - 1, 2 ** 30]
    assert [a[0] for a in stub.asked] == ["sc_graph_components", "sc_graph_quotient"]


def test_the_call_is_in_the_headers_order(monkeypatch):
    stub = _Stub(edges=2, clusters=2)
    monkeypatch.setattr(nat, "_backend", stub)
    monkeypatch.setattr(proc3d, "QUOTIENT_FIRST_EDGES", 5)
    extra = (np.array([[0, 2]], np.int32), np.array([2.0]))
    out = proc3d.graph_quotient(ROWS, [0, 0, 1], 3, points=np.zeros((3, 3)), key=[4, 4, 5], extra=extra, weights=True, device=3)
    assert len(stub.asked) == 1
    (name, N, offsets, row_len, index, weights, E, squared, ex, ex_w, M, labels, L, key, points, on_device, device, cluster, counts,
     centers, edges, edge_w, capacity, nc, ne, stream) = stub.asked[0]
    assert (name, N, offsets, row_len, E, squared, M, L, on_device, device, capacity, stream) == \
        ("sc_graph_quotient", 3, 0, 2, 6, 1, 1, 3, 0, 3, 5, 0)
    assert all([index, weights, ex, ex_w, labels, key, points, cluster, counts, centers, edges, edge_w, nc, ne])
    assert [a.shape for a in out] == [(3,), (2,), (2, 3), (2, 2), (2,)]
    stub.asked = []
    out = proc3d.graph_quotient(ROWS, [0, 0, 1], 3)  # no points, no key, no weights: their places are NULL
    args = stub.asked[0]
    assert args[5] == 0 and args[9] == 0 and args[13] == 0 and args[14] == 0 and args[19] == 0 and args[21] == 0 and args[20]
    assert out[2] is None and out[4] is None


def test_the_second_ask_when_the_first_was_too_small(monkeypatch):
    stub = _Stub(edges=3, clusters=2)
    monkeypatch.setattr(nat, "_backend", stub)
    monkeypatch.setattr(proc3d, "QUOTIENT_FIRST_EDGES", 1)
    out = proc3d.graph_quotient(ROWS, [0, 0, 1], 2, weights=True)
    assert [a[22] for a in stub.asked] == [1, 3] and out[3].shape == (3, 2) and out[4].shape == (3,)
    stub.asked = []
    monkeypatch.setattr(proc3d, "QUOTIENT_FIRST_EDGES", 3)
    proc3d.graph_quotient(ROWS, [0, 0, 1], 2)
    assert [a[22] for a in stub.asked] == [3]
