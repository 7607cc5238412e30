"""CPU: the checker of the graph unit (tests/graph_oracle.py) pinned against networkx and scipy -- the reference's own
dependency, ``nx.dijkstra_predecessor_and_distance`` (plant3dvision/proc3d.py:287) -- bit for bit, and what the Python
wrappers of ``proc3d`` judge and do without a device."""
import os
import re

import networkx as nx
import numpy as np
import pytest
from scipy import sparse
from scipy.sparse import csgraph

from plant3dvision_amd import _native as nat
from plant3dvision_amd import proc3d
from tests import graph_oracle as oracle


def _graphs():
    """name -> (points, rows, root): the three knn graphs DESIGN.md 20 names, a two-blob cloud and radius rows."""
    rng = np.random.default_rng(20)
    out = {}
    p = rng.uniform(0.0, 10.0, size=(3000, 3))
    out["random 3000 k6"] = (p, oracle.knn_rows(p, 6), 17)
    p = np.round(rng.uniform(0.0, 12.0, size=(4000, 3)))  # an integer lattice: many ties, duplicate points
    out["lattice 4000 k5"] = (p, oracle.knn_rows(p, 5), 0)
    p = rng.normal(size=(257, 3))
    out["random 257 k4"] = (p, oracle.knn_rows(p, 4), 256)
    p = np.concatenate([rng.uniform(0.0, 1.0, size=(150, 3)), rng.uniform(0.0, 1.0, size=(150, 3)) + 50.0])
    out["two blobs k4"] = (p, oracle.knn_rows(p, 4), 3)
    out["two blobs radius"] = (p, oracle.radius_rows(p, 0.25), 151)
    return out


GRAPHS = _graphs()


def _nx_graph(rows):
    """The reference's graph: ``nx.Graph`` with ``add_edge(i, j, weight=...)`` for every arc, self-loops included."""
    n, arcs = oracle.arcs_of(rows)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    for i, j, w in arcs:
        g.add_edge(i, j, weight=w)
    return g


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_checker_distances_equal_networkx_and_scipy(name):
    _, rows, root = GRAPHS[name]
    n, arcs = oracle.arcs_of(rows)
    got = oracle.distances(rows, root)
    _, dist = nx.dijkstra_predecessor_and_distance(_nx_graph(rows), root)
    want = np.full(n, np.inf)
    for v, d in dist.items():
        want[v] = d
    assert np.array_equal(got, want)
    if name.startswith("two blobs"):
        assert np.isinf(got).any() and np.isfinite(got).any()
    edges = {}
    for i, j, w in arcs:  # one entry per undirected edge and direction: a csr_matrix would ADD repeated entries
        edges[(i, j)] = edges[(j, i)] = w
    ij = np.array(sorted(edges), dtype=np.int64).reshape(-1, 2)
    m = sparse.csr_matrix((np.array([edges[tuple(e)] for e in ij.tolist()]), (ij[:, 0], ij[:, 1])), shape=(n, n))
    assert np.array_equal(got, csgraph.dijkstra(m, directed=True, indices=root))


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_checker_components_equal_networkx(name):
    _, rows, _ = GRAPHS[name]
    labels, count = oracle.components(rows)
    want = sorted(sorted(c) for c in nx.connected_components(_nx_graph(rows)))
    got = sorted(sorted(np.flatnonzero(labels == c).tolist()) for c in range(count))
    assert got == want and labels.min() == 0
    firsts = [int(np.flatnonzero(labels == c)[0]) for c in range(count)]
    assert firsts == sorted(firsts)  # numbered by the smallest member


@pytest.mark.parametrize("name", ["random 257 k4", "two blobs k4", "two blobs radius"])
def test_checker_clusters_equal_the_subgraph_loop(name):
    """The per-bin loop of the reference (proc3d.py:303-311) -- ``g.subgraph(nodes of the bin)``, its connected components --
    with the bins of our rule in place of its ``bisect`` cut."""
    points, rows, root = GRAPHS[name]
    cluster, centers, cluster_edges, d = oracle.clusters(points, rows, root, 0.4)
    bins = oracle.bins_of(d, 0.4)
    g = _nx_graph(rows)
    want = []
    for b in range(bins.max() + 1):
        want += [sorted(c) for c in nx.connected_components(g.subgraph(np.flatnonzero(bins == b).tolist()))]
    got = [np.flatnonzero(cluster == c).tolist() for c in range(cluster.max() + 1)]
    assert sorted(got) == sorted(want) and len(centers) == len(got)
    assert np.array_equal(cluster < 0, np.isinf(d))
    keys = [(int(bins[m[0]]), m[0]) for m in got]
    assert keys == sorted(keys)  # numbered by (bin, smallest member)
    q = nx.quotient_graph(g.subgraph(np.flatnonzero(cluster >= 0).tolist()), [frozenset(m) for m in got], relabel=True)
    assert sorted((min(a, b), max(a, b)) for a, b in q.edges()) == [tuple(e) for e in cluster_edges.tolist()]


def test_checker_keeps_inf_where_a_sum_overflows():
    """1e308 + 1e308 is +inf, which is not below the +inf of an unreached node: the node stays unreached, as in networkx
    and scipy."""
    rows = (np.full((4, 1), -1, dtype=np.int32), np.full((4, 1), np.inf))
    extra = (np.array([[0, 1], [1, 2], [2, 3]], dtype=np.int32), np.full(3, 1e308))
    got = oracle.distances(rows, 0, extra)
    assert got.tolist() == [0.0, 1e308, np.inf, np.inf]
    g = nx.Graph()
    g.add_nodes_from(range(4))
    g.add_weighted_edges_from((int(a), int(b), float(w)) for (a, b), w in zip(extra[0].tolist(), extra[1].tolist()))
    _, dist = nx.dijkstra_predecessor_and_distance(g, 0)
    assert [dist.get(v, np.inf) for v in range(4)] == got.tolist()
    with np.errstate(over="ignore"):
        m = sparse.csr_matrix((np.tile(extra[1], 2), (np.concatenate([extra[0][:, 0], extra[0][:, 1]]), np.concatenate([extra[0][:, 1], extra[0][:, 0]]))),
                              shape=(4, 4))
        assert np.array_equal(got, csgraph.dijkstra(m, directed=True, indices=0))
    labels, count = oracle.components(rows, None, extra)
    assert labels.tolist() == [0, 0, 0, 0] and count == 1  # joined all the same: the components read no weight


def test_strip_self_arcs_of_the_scattered_cloud():
    """The input of the empty-row tests of the GPU files, made here by brute force: the properties hold, the arcs are the
    same without the self-arcs."""
    rows = oracle.radius_rows(oracle.scattered_cloud(), oracle.SCATTER_RADIUS)
    stripped = oracle.strip_self_arcs(rows)
    assert oracle.arcs_of(stripped) == oracle.arcs_of(rows)
    assert np.array_equal(oracle.distances(stripped, 0), [0.0] + [np.inf] * 1024)


# ---- the bins of distance_to_root_clusters -------------------------------------------------------------------------
def _fixed_distances(monkeypatch, d, want_weights=False):
    """``proc3d`` with its three device calls replaced: the distances are ``d``, the keys the components get are kept."""
    seen = {}
    n = len(d)

    def components(rows, key=None, **kw):
        seen["bins"] = np.array(key)
        return np.zeros(n, np.int32), 1

    def quotient(rows, labels, n_labels, **kw):
        return np.zeros(n, np.int32), np.array([n], np.int32), np.zeros((1, 3)), np.zeros((0, 2), np.int32), np.zeros(0) if kw.get("weights") else None

    monkeypatch.setattr(proc3d, "graph_distances", lambda rows, root, **kw: np.array(d, dtype=np.float64))
    monkeypatch.setattr(proc3d, "graph_components", components)
    monkeypatch.setattr(proc3d, "graph_quotient", quotient)
    return seen


def test_bins_that_do_not_fit_int32_are_refused(monkeypatch):
    seen = _fixed_distances(monkeypatch, [0.0, 1.0, 0.5])
    pts = np.zeros((3, 3))
    for bad in (1e-12, 5e-324, np.nextafter(2.0 ** -31, 0.0)):  # 1e12 bins; a quotient that overflows; 2^31 + 1 bins
        with pytest.raises(ValueError, match="bin_size"):
            proc3d.distance_to_root_clusters(pts, ROWS, 0, bad)
        assert seen == {}
    out = proc3d.distance_to_root_clusters(pts, ROWS, 0, 2.0 ** -31)  # 2^31 bins: the last one is 2^31 - 1
    assert len(out) == 4 and seen["bins"].dtype == np.int32 and seen["bins"].tolist() == [0, 2 ** 31 - 1, 2 ** 30]
    seen.clear()
    _fixed_distances(monkeypatch, [0.0, np.inf, 1e300])
    with pytest.raises(ValueError, match="bin_size"):
        proc3d.distance_to_root_clusters(pts, ROWS, 0, 1e-10)  # 1e310 overflows
    seen = _fixed_distances(monkeypatch, [np.inf, 0.0, np.inf])  # the root alone: one bin whatever its size
    proc3d.distance_to_root_clusters(pts, ROWS, 1, 5e-324)
    assert seen["bins"].tolist() == [-1, 0, -1]


# ---- what the wrappers refuse and do without a device -------------------------------------------------------------
ROWS =(np.array([[1, -1], [0, 2], [1, -1]], dtype=np.int32), np.array([[1.0, np.inf], [1.0, 4.0], [4.0, np.inf]]))


def test_refusals_that_need_no_device():
    import torch
    index, d2 = ROWS
    for root in (-1, 3, 10 ** 12):
        with pytest.raises(ValueError, match="root must be 0 .. 2"):
            proc3d.graph_distances(ROWS, root)
    with pytest.raises(ValueError, match="all arrays or all CUDA tensors"):
        proc3d.graph_distances((torch.from_numpy(index), d2), 0)
    with pytest.raises(ValueError, match="all arrays or all CUDA tensors"):
        proc3d.graph_components(ROWS, extra=(torch.zeros((1, 2), dtype=torch.int32), np.zeros(1)))
    with pytest.raises(ValueError, match="all arrays or all CUDA tensors"):
        proc3d.graph_components(ROWS, key=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous CUDA tensors"):
        proc3d.graph_distances((torch.from_numpy(index), torch.from_numpy(d2)), 0)  # CPU tensors
    for bad in [(index,), (index, d2, d2, d2), (index, d2[:, :1]), (index.reshape(-1), d2.reshape(-1)),
                (np.zeros((2, 2), np.int64), index.reshape(-1), d2.reshape(-1)), (np.zeros(0, np.int64), index[:0, 0], d2[:0, 0])]:
        with pytest.raises(ValueError):
            proc3d.graph_distances(bad, 0)
    with pytest.raises(ValueError, match="n is 4, the rows hold 3 nodes"):
        proc3d.graph_distances(ROWS, 0, n=4)
    with pytest.raises(ValueError, match="extra must be"):
        proc3d.graph_distances(ROWS, 0, extra=(np.zeros((2, 3), np.int32), np.zeros(2)))
    with pytest.raises(ValueError, match="one key per node"):
        proc3d.graph_components(ROWS, key=np.zeros(2, np.int32))
    with pytest.raises(ValueError, match="bin_size"):
        proc3d.distance_to_root_clusters(np.zeros((3, 3)), ROWS, 0, 0.0)
    with pytest.raises(ValueError, match="one label per point"):
        proc3d.connect_edges(np.zeros((3, 3)), np.zeros(2, np.int32), 0)


class _Stub:
    def __init__(self):
        self.asked = []

    def call(self, name, *args):
        self.asked.append((name,) + args)
        return nat.SC_OK

    @staticmethod
    def string(ret):
        return ""


def test_no_nodes_no_native_call(monkeypatch):
    stub = _Stub()
    monkeypatch.setattr(nat, "_backend", stub)
    empty_knn = (np.zeros((0, 4), np.int32), np.zeros((0, 4)))
    empty_csr = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    for rows in (empty_knn, empty_csr):
        d, rounds = proc3d.graph_distances(rows, 0, return_rounds=True)
        assert d.dtype == np.float64 and d.shape == (0,) and rounds == 0
        labels, count = proc3d.graph_components(rows)
        assert labels.dtype == np.int32 and labels.shape == (0,) and count == 0
        cluster, centers, cluster_edges, d = proc3d.distance_to_root_clusters(np.zeros((0, 3)), rows, 0, 1.0)
        assert cluster.shape == (0,) and centers.shape == (0, 3) and cluster_edges.shape == (0, 2) and d.shape == (0,)
    edges, weights = proc3d.connect_edges(np.zeros((0, 3)), np.zeros(0, np.int32), 0)
    assert edges.shape == (0, 2) and edges.dtype == np.int32 and weights.shape == (0,)
    assert stub.asked == []


def test_the_calls_the_wrappers_make(monkeypatch):
    """The arguments as the header orders them; a connected cloud asks ``nearest_points`` for nothing."""
    stub = _Stub()
    monkeypatch.setattr(nat, "_backend", stub)
    proc3d.graph_distances(ROWS, 2, device=3)
    name, N, offsets, row_len, index, values, E, squared, extra, extra_w, M, on_device, root, device, out, rounds, stream = stub.asked[0]
    assert (name, N, offsets, row_len, E, squared, extra, extra_w, M, on_device, root, device, rounds, stream) == \
        ("sc_graph_distances", 3, 0, 2, 6, 1, 0, 0, 0, 0, 2, 3, 0, 0) and index and values and out
    stub.asked = []
    csr = (np.array([0, 1, 2], np.int64), np.array([1, 0], np.int32), np.array([1.0, 1.0]))
    proc3d.graph_components(csr, key=[0, -1], extra=(np.array([[0, 1]]), np.array([2.0])))
    name, N, offsets, row_len, index, E, extra, M, key, on_device, device, labels, count, stream = stub.asked[0]
    assert (name, N, row_len, E, M, on_device, device, stream) == ("sc_graph_components", 2, 0, 2, 1, 0, 0, 0)
    assert offsets and index and extra and key and labels and count
    stub.asked = []
    assert proc3d.connect_edges(np.zeros((3, 3)), [0, 0, 0], 1)[0].shape == (0, 2) and stub.asked == []
    proc3d.release_graph_buffers()
    assert stub.asked == [("sc_graph_release",)]
    assert "sc_graph_release" not in proc3d.RELEASES and "release_device_buffers" in proc3d.release_graph_buffers.__doc__


def test_errors_are_read_with_the_units_getter(monkeypatch):
    class Refusing(_Stub):
        def call(self, name, *args):
            self.asked.append(name)
            return b"text" if name == "sc_graph_error" else nat.SC_ERR_INVALID

        @staticmethod
        def string(ret):
            return ret.decode()

    stub = Refusing()
    monkeypatch.setattr(nat, "_backend", stub)
    with pytest.raises(ValueError, match="sc_graph_distances: text"):
        proc3d.graph_distances(ROWS, 0)
    assert stub.asked == ["sc_graph_distances", "sc_graph_error"]


def test_argument_errors_of_the_library_need_no_device():
    b = nat.backend()
    index, d2 = np.ascontiguousarray(ROWS[0]), np.ascontiguousarray(ROWS[1])
    out, lab = np.zeros(3), np.zeros(3, np.int32)

    def distances(index=index, d2=d2, N=3, E=6, root=0, device=0, offsets=0, row_len=2, out=out, extra=0, extra_w=0, M=0):
        return b.call("sc_graph_distances", N, offsets, row_len, nat.addr(index), nat.addr(d2), E, 1, extra, extra_w, M, 0, root, device,
                      nat.addr(out) if out is not None else 0, 0, 0)

    def refused(rc, text):
        assert rc == nat.SC_ERR_INVALID and text in b.string(b.call("sc_graph_error")), b.string(b.call("sc_graph_error"))

    refused(distances(root=3), "root")
    refused(distances(root=-1), "root")
    refused(distances(device=64), "device ordinal")
    refused(distances(out=None), "null")
    refused(distances(E=5), "row_len")
    refused(distances(N=2 ** 31, E=2 ** 32), "N must be")
    refused(distances(index=np.array([[1, -1], [0, 3], [1, -1]], np.int32)), "index outside")
    refused(distances(index=np.array([[1, -2], [0, 2], [1, -1]], np.int32)), "index outside")
    for w in (np.nan, -1.0, np.inf):
        bad = d2.copy()
        bad[1, 1] = w
        refused(distances(d2=bad), "weights must be finite")
    pair, pw = np.array([[0, 3]], np.int32), np.array([1.0])
    refused(distances(extra=nat.addr(pair), extra_w=nat.addr(pw), M=1), "extra pair")
    pair, pw = np.array([[0, 2]], np.int32), np.array([np.nan])
    refused(distances(extra=nat.addr(pair), extra_w=nat.addr(pw), M=1), "extra weights")
    flat_i, flat_w = np.array([1, 0, 2, 1], np.int32), np.ones(4)
    for offsets in ([0, 1, 3, 3], [0, 3, 2, 4], [1, 1, 3, 4], [0, 1, 3, 5]):
        o = np.array(offsets, np.int64)
        refused(distances(index=flat_i, d2=flat_w, E=4, offsets=nat.addr(o), row_len=0), "offsets must rise")
    o = np.array([0, 1, 3, 4], np.int64)
    refused(distances(index=np.array([1, 0, -1, 1], np.int32), d2=flat_w, E=4, offsets=nat.addr(o), row_len=0), "index outside")
    rc = b.call("sc_graph_components", 3, 0, 2, nat.addr(index), 6, 0, 0, 0, 0, 0, 0, 0, 0)
    refused(rc, "null")
    count = np.full(1, 7, np.int32)  # no nodes: no device call, zero components
    assert b.call("sc_graph_components", 0, 0, 2, nat.addr(index), 0, 0, 0, 0, 0, 0, nat.addr(lab), nat.addr(count), 0) == nat.SC_OK
    assert count[0] == 0


def test_header_constant_and_symbols():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spacecarve.h")).read()
    assert int(re.search(r"#define SC_GRAPH_ROUNDS_PER_WAIT (\d+)", text).group(1)) == nat.SC_GRAPH_ROUNDS_PER_WAIT == 64
    for name in ("sc_graph_distances", "sc_graph_components", "sc_graph_error", "sc_graph_release", "sc_graph_set_blocks"):
        assert name in nat.EXPORTED_SYMBOLS


def test_no_cpu_fallback_without_device():
    try:
        n = nat.device_count()
    except nat.SpaceCarveError:
        n = 0
    if n > 0:  # with a device the calls compute (tests/test_graph_gpu.py); nothing to show here
        return
    with pytest.raises(nat.SpaceCarveError):
        proc3d.graph_distances(ROWS, 0)
    with pytest.raises(nat.SpaceCarveError):
        proc3d.graph_components(ROWS)
