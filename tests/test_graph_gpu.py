"""GPU: ``proc3d.graph_distances`` / ``graph_components`` (``sc_graph_distances`` / ``sc_graph_components``,
csrc/graph.hip) and ``connect_edges`` / ``distance_to_root_clusters`` / ``skeleton_from_distance_to_root_clusters`` over
them against the checker (tests/graph_oracle.py, which tests/test_graph_host.py pins against networkx and scipy).
Every comparison is ``np.array_equal``, from arrays and from tensors."""
import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import proc3d
from tests import graph_oracle as oracle

pytestmark = pytest.mark.gpu


def on_device(rows):
    import torch
    return None if rows is None else tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in rows)


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def check_graph(rows, root, extra=None, key=None):
    """Distances and components of one graph, from arrays and from tensors, against the checker: ``(d, labels, count)``."""
    import torch
    want_d = oracle.distances(rows, root, extra)
    want_l, want_c = oracle.components(rows, key, extra)
    for form in (lambda x: x, on_device):
        d, rounds = proc3d.graph_distances(form(rows), root, extra=form(extra), return_rounds=True)
        assert (type(d) is np.ndarray) == (form is not on_device) and host(d).dtype == np.float64
        assert np.array_equal(host(d), want_d), "distances"
        assert 1 <= rounds <= len(want_d)
        k = None if key is None else (key if form is not on_device else torch.from_numpy(key).cuda())
        labels, count = proc3d.graph_components(form(rows), key=k, extra=form(extra))
        assert host(labels).dtype == np.int32 and np.array_equal(host(labels), want_l) and count == want_c, "components"
    return want_d, want_l, want_c


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1025])
def test_sizes(gpu_device, n):
    rng = np.random.default_rng(n)
    pts = rng.uniform(0.0, 1.0, size=(n, 3))
    root = n // 2
    for k in (1, 2, 5):
        rows = proc3d.knn_points(pts, pts, k)
        d, labels, count = check_graph(rows, root)
        if k == 1 and n > 1:  # every point's nearest is itself: self-arcs only, nothing is joined
            assert np.isinf(d).sum() == n - 1 and count == n
        if k == 2 and n > 2:
            assert np.isinf(d).any() and np.isfinite(d).sum() >= 2 and 1 < count < n  # pairs and short chains
    radius = 1.2 * (1.0 / n) ** (1.0 / 3.0)
    rows = proc3d.radius_points(pts, pts, radius)
    d, labels, count = check_graph(rows, root)
    if n >= 63:
        assert 1 < count < n and np.isinf(d).any() and np.isfinite(d).sum() > 1


def test_ties_on_a_doubled_lattice(gpu_device):
    g = np.arange(9.0)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = np.concatenate([pts, pts])  # every point twice: zero-weight edges, equal sums along many walks
    d, _, count = check_graph(proc3d.knn_points(pts, pts, 8), 100)
    assert (d == 0.0).sum() == 2
    d, _, count = check_graph(proc3d.radius_points(pts, pts, 1.5), 0)
    assert count == 1 and np.isfinite(d).all() and len(np.unique(d)) < len(d) // 4


def test_one_way_arcs_are_used_both_ways(gpu_device):
    rows = (np.array([[-1], [0], [1], [2]], dtype=np.int32), np.array([[np.inf], [1.0], [4.0], [9.0]]))
    d, labels, count = check_graph(rows, 0)
    assert d.tolist() == [0.0, 1.0, 3.0, 6.0] and labels.tolist() == [0, 0, 0, 0] and count == 1
    rows = (np.array([0, 0, 1, 2, 3], dtype=np.int64), np.array([0, 1, 2], dtype=np.int32), np.array([1.0, 4.0, 9.0]))
    assert check_graph(rows, 0)[0].tolist() == [0.0, 1.0, 3.0, 6.0]


def test_rounds_past_the_first_wait_and_capped_grids(gpu_device):
    rng = np.random.default_rng(4)
    x = np.cumsum(rng.uniform(1.0, 1.5, size=300))  # two steps are longer than any one: the 3 nearest are i - 1, i, i + 1
    pts = np.stack([x, np.zeros(300), np.zeros(300)], axis=1)
    rows = proc3d.knn_points(pts, pts, 3)
    want = oracle.distances(rows, 0)
    assert np.isfinite(want).all()
    d, rounds = proc3d.graph_distances(rows, 0, return_rounds=True)
    assert nat.SC_GRAPH_ROUNDS_PER_WAIT < rounds <= 300  # about one node per round: the far end is 298 hops away
    assert np.array_equal(d, want)
    nat.backend().call("sc_graph_set_blocks", 1)  # one block: every grid-stride loop goes past its first trip
    try:
        check_graph(rows, 299)
        blob = np.random.default_rng(5).uniform(0.0, 1.0, size=(700, 3))
        check_graph(proc3d.knn_points(blob, blob, 6), 1)
        check_graph(proc3d.radius_points(blob, blob, 0.12), 1, key=(np.arange(700) % 3 - 1).astype(np.int32))
    finally:
        nat.backend().call("sc_graph_set_blocks", 0)


W = nat.SC_GRAPH_ROUNDS_PER_WAIT


def _chain(n, d2):
    """Rows of length 1: node i points at i + 1, the last place is unused."""
    index = np.arange(1, n + 1, dtype=np.int32).reshape(n, 1)
    index[-1, 0] = -1
    return index, np.asarray(d2, dtype=np.float64).reshape(n, 1)


@pytest.mark.parametrize("n", [W - 1, W, W + 1, 2 * W, 2 * W + 1])
def test_chains_end_on_either_side_of_a_wait(gpu_device, n):
    """A chain's frontier is the nodes one hop further: the number of rounds is exact, and the last live round falls
    on, before and behind the round after which the host looks at the header."""
    rows = _chain(n, np.random.default_rng(n).uniform(1.0, 4.0, size=n))
    for root in (0, n - 1, n // 3):  # from the far end every arc is used backwards
        want = oracle.distances(rows, root)
        assert np.isfinite(want).all()
        for form in (lambda x: x, on_device):
            d, rounds = proc3d.graph_distances(form(rows), root, return_rounds=True)
            assert rounds == max(root, n - 1 - root) + 1, (root, rounds)
            assert np.array_equal(host(d), want)
    check_graph(rows, n // 3)


def _fan(extra_weight):
    """A chain of unit arcs and extra pairs from node 0 to every node from 2 on."""
    n = 2 * W + 3
    far = np.arange(2, n, dtype=np.int32)
    extra = (np.stack([np.zeros_like(far), far], axis=1), np.array([extra_weight(v) for v in far.tolist()], dtype=np.float64))
    return n, _chain(n, np.ones(n)), extra


def test_nodes_that_fall_again_and_again(gpu_device):
    """Round 0 lowers node v to 2 v through its extra pair; the chain then lowers it again, in the end to v: nodes re-enter
    the frontier many times (the stamps).  Inside a round a node may be read after it fell, so the count is not fixed."""
    n, rows, extra = _fan(lambda v: 2.0 * v)
    for blocks in (0, 1):
        nat.backend().call("sc_graph_set_blocks", blocks)
        try:
            d, _, count = check_graph(rows, 0, extra=extra)  # 1 <= rounds <= n is asserted there
        finally:
            nat.backend().call("sc_graph_set_blocks", 0)
        assert d.tolist() == [float(v) for v in range(n)] and count == 1


def test_ties_lower_nothing(gpu_device):
    """The extra pairs weigh what the chain's walk does: round 0 reaches every node, round 1 finds only equal sums and
    lowers nothing (rule G2 asks for less, not for less or equal), and there is no round 2."""
    n, rows, extra = _fan(float)
    d, _, _ = check_graph(rows, 0, extra=extra)
    assert d.tolist() == [float(v) for v in range(n)]
    for form in (lambda x: x, on_device):
        assert proc3d.graph_distances(form(rows), 0, extra=form(extra), return_rounds=True)[1] == 2


def test_sums_that_overflow_stay_unreached(gpu_device):
    rows = (np.full((4, 1), -1, dtype=np.int32), np.full((4, 1), np.inf))
    extra = (np.array([[0, 1], [1, 2], [2, 3]], dtype=np.int32), np.full(3, 1e308))
    d, labels, count = check_graph(rows, 0, extra=extra)
    assert d.tolist() == [0.0, 1e308, np.inf, np.inf] and count == 1


# ---- rows without arcs ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stripped(gpu_device):
    """The radius rows of the scattered cloud without their self-arcs: runs of empty rows, at both ends too."""
    pts = oracle.scattered_cloud()
    return pts, oracle.strip_self_arcs(proc3d.radius_points(pts, pts, oracle.SCATTER_RADIUS))


def test_csr_rows_without_self_arcs(gpu_device, stripped):
    _, rows = stripped
    busy = int(np.flatnonzero(np.diff(rows[0]) > 0)[0])
    key = (np.arange(1025) % 3 - 1).astype(np.int32)
    for blocks in (0, 1):
        nat.backend().call("sc_graph_set_blocks", blocks)
        try:
            for k in (None, key):
                d, _, count = check_graph(rows, busy, key=k)
                assert 1 < np.isfinite(d).sum() < 1025
                d, _, _ = check_graph(rows, 0, key=k)  # the root's own row is empty
                assert d[0] == 0.0 and np.isinf(d[1:]).all()
        finally:
            nat.backend().call("sc_graph_set_blocks", 0)


NO_ARCS = {"csr": (np.zeros(66, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0)),
           "fixed": (np.full((65, 3), -1, dtype=np.int32), np.full((65, 3), np.inf))}
ONLY_EXTRA = (np.array([[64, 0], [3, 64], [0, 64]], dtype=np.int32), np.array([2.0, 0.25, 1.5]))


@pytest.mark.parametrize("form", sorted(NO_ARCS))
def test_graphs_without_arcs(gpu_device, form):
    """E == 0 (no index array at all, an empty CUDA tensor) and rows of unused places; then extra pairs as the only arcs."""
    rows = NO_ARCS[form]
    for root in (0, 64):
        d, labels, count = check_graph(rows, root)
        assert np.isinf(d).sum() == 64 and d[root] == 0.0 and count == 65 and np.array_equal(labels, np.arange(65))
    d, labels, count = check_graph(rows, 0, extra=ONLY_EXTRA)
    assert d[64] == 1.5 and d[3] == 1.75 and np.isinf(d).sum() == 62 and count == 63
    key = (np.arange(65) % 2).astype(np.int32)
    key[3] = -1
    d, labels, count = check_graph(rows, 3, extra=ONLY_EXTRA, key=key)
    assert d[64] == 0.25 and d[0] == 1.75 and count == 63 and labels[3] == -1 and labels[64] == labels[0] == 0


# ---- streams and the life of the work buffers ------------------------------------------------------------------------
def test_streams_refusals_and_work_buffers(gpu_device):
    """The three entries share one slot of work buffers: calls on two streams, a call that has to grow the buffers behind
    another's work, a call the device judge refuses in between, ``release_graph_buffers`` and the host-array route."""
    import torch
    from tests import quotient_oracle
    rng = np.random.default_rng(51)
    sp, lp = rng.uniform(0.0, 1.0, size=(300, 3)), rng.uniform(0.0, 1.0, size=(6000, 3))
    small, large = proc3d.knn_points(sp, sp, 4), proc3d.knn_points(lp, lp, 8)
    want = {}
    for name, rows, pts in (("small", small, sp), ("large", large, lp)):
        d = oracle.distances(rows, 5)
        labels, count = oracle.components(rows)
        slab = (pts[:, 0] * 6).astype(np.int32)
        q = quotient_oracle.quotient(rows, slab, 6, points=pts, weights=True)
        assert len(q[1]) == 6 and len(q[3]) >= 5
        want[name] = (d, labels, count, slab, q)
    proc3d.release_graph_buffers()  # whatever earlier tests left: the first call allocates
    dev = {name: (on_device(rows), torch.from_numpy(want[name][3]).cuda(), torch.from_numpy(pts).cuda())
           for name, rows, pts in (("small", small, sp), ("large", large, lp))}
    bad_index = small[0].copy()
    bad_index[299, 3] = 300  # the last place: the judge reads inside the stated lengths only
    bad = (torch.from_numpy(bad_index).cuda(), dev["small"][0][1])

    def ask(name):
        rows, slab, pts = dev[name]
        return (proc3d.graph_distances(rows, 5), proc3d.graph_components(rows), proc3d.graph_quotient(rows, slab, 6, points=pts, weights=True))

    def same(got, name):
        d, labels, count, _, q = want[name]
        assert np.array_equal(host(got[0]), d) and np.array_equal(host(got[1][0]), labels) and got[1][1] == count
        assert all(quotient_oracle.same_bits(host(a), b) for a, b in zip(got[2], q))

    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))  # the uploads
    r1 = ask("small")
    with torch.cuda.stream(side):
        r2 = ask("large")  # a second stream; grows the buffers behind the first call
    r3 = ask("small")
    for entry in (lambda: proc3d.graph_distances(bad, 5), lambda: proc3d.graph_components(bad),
                  lambda: proc3d.graph_quotient(bad, dev["small"][1], 6, points=dev["small"][2], weights=True)):
        with pytest.raises(ValueError, match="index outside"):
            entry()
    r4 = ask("small")
    side.synchronize()
    torch.cuda.current_stream(gpu_device).synchronize()
    for got, name in ((r1, "small"), (r2, "large"), (r3, "small"), (r4, "small")):
        same(got, name)
    proc3d.release_graph_buffers()
    same(ask("small"), "small")  # in fresh buffers
    for name, rows, pts in (("small", small, sp), ("large", large, lp)):  # the host-array route
        same((proc3d.graph_distances(rows, 5), proc3d.graph_components(rows),
              proc3d.graph_quotient(rows, want[name][3], 6, points=pts, weights=True)), name)
    proc3d.release_graph_buffers()
    same(ask("large"), "large")


def test_bins_at_the_edge_of_int32(gpu_device):
    """The smallest ``bin_size`` whose last bin still fits int32 is accepted and gives the checker's clusters; the float64
    just below it is refused, from arrays and from tensors."""
    import math
    pts = _blobs()
    rows = proc3d.knn_points(pts, pts, 5)
    d = oracle.distances(rows, 7)
    top = float(d[np.isfinite(d)].max())

    def fits(b):  # the rule, in Python's integers: n_bins - 1 <= 2^31 - 1
        return math.isfinite(top / b) and math.ceil(top / b) - 1 <= 2 ** 31 - 1

    good = top / 2.0 ** 31
    for _ in range(8):
        if fits(good):
            break
        good = float(np.nextafter(good, np.inf))
    for _ in range(8):
        if not fits(float(np.nextafter(good, 0.0))):
            break
        good = float(np.nextafter(good, 0.0))
    refused = float(np.nextafter(good, 0.0))
    assert fits(good) and not fits(refused) and math.ceil(top / good) == 2 ** 31
    want = oracle.clusters(pts, rows, 7, good)
    assert oracle.bins_of(d, good).max() == 2 ** 31 - 1
    for form in (lambda x: x, on_device):
        for weights in (False, True):
            with pytest.raises(ValueError, match="bin_size"):
                proc3d.distance_to_root_clusters(pts, form(rows), 7, refused, weights=weights)
            got = proc3d.distance_to_root_clusters(pts, form(rows), 7, good, weights=weights)
            for a, b in zip(got, want):
                assert host(a).dtype == b.dtype and np.array_equal(host(a), b)


def test_sqrt_is_numpys(gpu_device):
    d2 = np.array([2.0, 0.1, np.nextafter(1.0, 2.0), 1e-300, 1e300, 3.0, 1e-320, 0.0])
    n = len(d2) + 1
    index = np.full((n, len(d2)), -1, dtype=np.int32)
    index[0] = np.arange(1, n)
    values = np.full((n, len(d2)), np.inf)
    values[0] = d2
    for form in (lambda x: x, on_device):
        d = host(proc3d.graph_distances(form((index, values)), 0))
        assert np.array_equal(d[1:], np.sqrt(d2)) and d[0] == 0.0


def test_components_with_a_key(gpu_device):
    rng = np.random.default_rng(6)
    pts = rng.uniform(0.0, 1.0, size=(500, 3))
    rows = proc3d.knn_points(pts, pts, 7)
    _, _, whole = check_graph(rows, 0)
    key = (pts[:, 0] * 4).astype(np.int32)  # slabs split the graph
    key[rng.choice(500, 60, replace=False)] = -1
    key[3] = -7
    _, labels, count = check_graph(rows, 0, key=key)
    assert count > whole and (labels[key < 0] == -1).all() and (labels[key >= 0] >= 0).all()
    for c in range(count):
        assert len(set(key[labels == c].tolist())) == 1
    _, labels, count = check_graph(rows, 0, key=np.full(500, -1, dtype=np.int32))
    assert count == 0 and (labels == -1).all()


GOOD_KNN = (np.array([[0, 1], [1, 0], [2, 1]], dtype=np.int32), np.array([[0.0, 1.0], [0.0, 1.0], [0.0, 4.0]]))
GOOD_CSR = (np.array([0, 1, 3, 4], dtype=np.int64), np.array([1, 0, 2, 1], dtype=np.int32), np.array([1.0, 1.0, 4.0, 4.0]))


def _bad_rows():
    out = {}
    for name, w in (("a NaN weight", np.nan), ("a negative weight", -1.0), ("an infinite weight", np.inf)):
        d2 = GOOD_KNN[1].copy()
        d2[2, 1] = w
        out[name + ", knn"] = (GOOD_KNN[0], d2), "weights must be finite"
        d2 = GOOD_CSR[2].copy()
        d2[1] = w
        out[name + ", csr"] = (GOOD_CSR[0], GOOD_CSR[1], d2), "weights must be finite"
    for bad in (3, -2):
        index = GOOD_KNN[0].copy()
        index[1, 1] = bad
        out[f"index {bad}, knn"] = (index, GOOD_KNN[1]), "index outside"
    for bad in (3, -1):
        index = GOOD_CSR[1].copy()
        index[2] = bad
        out[f"index {bad}, csr"] = (GOOD_CSR[0], index, GOOD_CSR[2]), "index outside"
    for offsets in ([0, 3, 1, 4], [0, 1, 3, 3], [1, 1, 3, 4]):
        out[f"offsets {offsets}"] = (np.array(offsets, dtype=np.int64), GOOD_CSR[1], GOOD_CSR[2]), "offsets must rise"
    return out


BAD = _bad_rows()


@pytest.mark.parametrize("name", sorted(BAD))
def test_refusals_and_the_call_after(gpu_device, name):
    rows, text = BAD[name]
    for form in (lambda x: x, on_device):
        with pytest.raises(ValueError, match=text):
            proc3d.graph_distances(form(rows), 0)
        assert host(proc3d.graph_distances(form(GOOD_KNN), 0)).tolist() == [0.0, 1.0, 3.0]
        if "weight" not in name:  # the components read no weight
            with pytest.raises(ValueError, match=text):
                proc3d.graph_components(form(rows))
        labels, count = proc3d.graph_components(form(GOOD_CSR))
        assert host(labels).tolist() == [0, 0, 0] and count == 1
    extra = (np.array([[0, 3]], dtype=np.int32), np.array([1.0]))
    for form in (lambda x: x, on_device):
        with pytest.raises(ValueError, match="extra pair"):
            proc3d.graph_distances(form(GOOD_KNN), 0, extra=form(extra))
        with pytest.raises(ValueError, match="extra weights"):
            proc3d.graph_distances(form(GOOD_KNN), 0, extra=form((np.array([[0, 2]], dtype=np.int32), np.array([np.nan]))))


def _blobs():
    rng = np.random.default_rng(8)
    centres = np.array([[0, 0, 0], [6, 0, 0], [0, 7, 0], [5, 5, 5], [-6, 1, 2]], dtype=np.float64)
    return np.concatenate([c + rng.uniform(-1.0, 1.0, size=(40, 3)) for c in centres])


def test_connect_edges(gpu_device):
    pts = _blobs()
    rows = proc3d.radius_points(pts, pts, 1.2)
    labels, count = proc3d.graph_components(rows)
    assert count >= 5
    for root in (0, 199):
        edges, weights = proc3d.connect_edges(pts, labels, root)
        want_e, want_w = oracle.connect_edges(pts, labels, root)
        assert edges.dtype == np.int32 and edges.shape == (count - 1, 2) and np.array_equal(edges, want_e) and np.array_equal(weights, want_w)
        d, joined, one = check_graph(rows, root, extra=(edges, weights))
        assert one == 1 and np.isfinite(d).all() and (joined == 0).all()


@pytest.mark.parametrize("connect", [True, False])
def test_clusters_and_skeleton(gpu_device, connect):
    import networkx as nx
    pts = _blobs()
    k, root, bin_size = 5, 7, 0.8
    rows = proc3d.knn_points(pts, pts, k)
    extra = None
    if connect:
        labels, _ = proc3d.graph_components(rows)
        extra = proc3d.connect_edges(pts, labels, root)
    want = oracle.clusters(pts, rows, root, bin_size, extra)
    for form in (lambda x: x, on_device):
        got = proc3d.distance_to_root_clusters(pts, form(rows), root, bin_size, extra=form(extra))
        for a, b in zip(got, want):
            assert host(a).dtype == b.dtype and np.array_equal(host(a), b)
    cluster, centers, cluster_edges, d = want
    assert connect == bool(np.isfinite(d).all())
    bins = oracle.bins_of(d, bin_size)
    n, arcs = oracle.arcs_of(rows, extra)
    g = nx.Graph((i, j) for i, j, _ in arcs)
    for c in range(len(centers)):
        members = np.flatnonzero(cluster == c).tolist()
        assert len(set(bins[members].tolist())) == 1 and (len(members) == 1 or nx.is_connected(g.subgraph(members)))
    tree, values = proc3d.skeleton_from_distance_to_root_clusters(proc3d.PointCloud(pts, None), root, bin_size, k, connect_all_points=connect)
    assert nx.is_tree(tree) and sorted(tree.nodes) == list(range(len(centers)))
    assert values == {v: int(c) for v, c in enumerate(cluster.tolist()) if c >= 0}
    assert all(np.array_equal(tree.nodes[c]["center"], centers[c]) for c in tree.nodes)
    assert set(tuple(sorted(e)) for e in tree.edges) <= set(map(tuple, cluster_edges.tolist()))
