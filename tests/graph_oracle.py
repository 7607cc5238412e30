"""The checker of the graph unit (``csrc/graph.hip``): plain Python and NumPy, written from the rules G1..G4
of ``include/spacecarve.h`` and the rules of ``proc3d.distance_to_root_clusters`` / ``connect_edges``, sharing no code
with the package.  ``tests/test_graph_host.py`` pins its distances bit for bit against networkx and scipy."""
import heapq
import math

import numpy as np


def arcs_of(rows, extra=None):
    """The arcs of ``(index [N, k], d2)`` or ``(offsets, index, d2)`` plus the extra pairs, as ``(n, [(i, j, w)])`` with
    ``w = sqrt(d2)`` (the extra weights as they are); unused places (``-1``) and self-arcs are dropped (rule G1)."""
    rows = [np.asarray(a) for a in rows]
    arcs = []
    if len(rows) == 2:
        index, d2 = rows
        n = index.shape[0]
        for i in range(n):
            for j, v in zip(index[i].tolist(), d2[i].tolist()):
                if j >= 0 and j != i:
                    arcs.append((i, j, float(np.sqrt(np.float64(v)))))
    else:
        offsets, index, d2 = rows
        n = len(offsets) - 1
        for i in range(n):
            for e in range(int(offsets[i]), int(offsets[i + 1])):
                j = int(index[e])
                if j != i:
                    arcs.append((i, j, float(np.sqrt(np.float64(d2[e])))))
    if extra is not None:
        for (i, j), w in zip(np.asarray(extra[0]).tolist(), np.asarray(extra[1]).tolist()):
            if i != j:
                arcs.append((int(i), int(j), float(w)))
    return n, arcs


def adjacency(n, arcs):
    adj = [[] for _ in range(n)]
    for i, j, w in arcs:
        adj[i].append((j, w))
        adj[j].append((i, w))
    return adj


def distances(rows, root, extra=None):
    """Rule G2 by a heap Dijkstra with a float64 accumulator: float64 ``[n]``, ``+inf`` for unreached nodes."""
    n, arcs = arcs_of(rows, extra)
    adj = adjacency(n, arcs)
    d = [math.inf] * n
    d[root] = 0.0
    heap = [(0.0, root)]
    done = [False] * n
    while heap:
        du, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        for v, w in adj[u]:
            nd = du + w
            if nd < d[v]:
                d[v] = nd
                heapq.heappush(heap, (nd, v))
    return np.array(d, dtype=np.float64)


def components(rows, key=None, extra=None):
    """Rule G3 by a host union-find: ``(labels int32 [n], count)``."""
    n, arcs = arcs_of(rows, extra)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i, j, _ in arcs:
        if key is not None and (key[i] < 0 or key[i] != key[j]):
            continue
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    labels = np.full(n, -1, dtype=np.int32)
    rank = {}
    for v in range(n):  # rising v: a component is met first at its smallest member
        if key is not None and key[v] < 0:
            continue
        r = find(v)
        if r not in rank:
            rank[r] = len(rank)
        labels[v] = rank[r]
    return labels, len(rank)


def bins_of(d, bin_size):
    finite = np.isfinite(d)
    n_bins = max(1, int(math.ceil(float(d[finite].max()) / bin_size)))
    out = np.full(len(d), -1, dtype=np.int32)
    for v in range(len(d)):
        if finite[v]:
            out[v] = min(int(math.floor(float(d[v]) / bin_size)), n_bins - 1)
    return out


def clusters(points, rows, root, bin_size, extra=None):
    """``(cluster int32 [n], centers [C, 3], cluster_edges int32 [K, 2], distances)`` by the rules of
    ``proc3d.distance_to_root_clusters``."""
    points = np.asarray(points, dtype=np.float64)
    n, arcs = arcs_of(rows, extra)
    d = distances(rows, root, extra)
    bins = bins_of(d, bin_size)
    labels, count = components(rows, bins, extra)
    members = [[] for _ in range(count)]
    for v in range(n):
        if labels[v] >= 0:
            members[labels[v]].append(v)
    order = sorted(range(count), key=lambda c: (int(bins[members[c][0]]), members[c][0]))
    cluster = np.full(n, -1, dtype=np.int32)
    centers = np.zeros((count, 3))
    for new, c in enumerate(order):
        cluster[members[c]] = new
        for axis in range(3):
            centers[new, axis] = np.bincount(np.zeros(len(members[c]), dtype=np.int64), weights=points[members[c], axis])[0] / float(len(members[c]))
    pairs = set()
    for i, j, _ in arcs:
        a, b = int(cluster[i]), int(cluster[j])
        if a >= 0 and b >= 0 and a != b:
            pairs.add((min(a, b), max(a, b)))
    return cluster, centers, np.array(sorted(pairs), dtype=np.int32).reshape(-1, 2), d


def connect_edges(points, labels, root):
    """``proc3d.connect_edges`` by brute force over all pairs: ``d2 = ((dx dx) + (dy dy)) + (dz dz)`` (rule N1), the least
    key ``(d2, i, j)`` over ``i`` outside and ``j`` inside the root's component."""
    points = np.asarray(points, dtype=np.float64)
    labels = np.asarray(labels)
    inside = labels == labels[root]
    edges, weights = [], []
    while not inside.all():
        best = None
        for i in np.flatnonzero(~inside).tolist():
            for j in np.flatnonzero(inside).tolist():
                dx, dy, dz = (points[i] - points[j]).tolist()
                key = ((dx * dx + dy * dy) + dz * dz, i, j)
                if best is None or key < best:
                    best = key
        edges.append((best[1], best[2]))
        weights.append(np.sqrt(np.float64(best[0])))
        inside |= labels == labels[best[1]]
    return np.array(edges, dtype=np.int32).reshape(-1, 2), np.array(weights, dtype=np.float64)


# ---- rows for the host tests, where no device makes them: brute-force k nearest with (d2, index) keys -----------------
def _d2_row(points, i):
    diff = points[i][None, :] - points
    return (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]


def knn_rows(points, k):
    points = np.asarray(points, dtype=np.float64)
    n = len(points)
    index = np.full((n, k), -1, dtype=np.int32)
    out = np.full((n, k), np.inf)
    for i in range(n):
        d2 = _d2_row(points, i)
        order = np.lexsort((np.arange(n), d2))[:k]
        index[i, :len(order)] = order
        out[i, :len(order)] = d2[order]
    return index, out


SCATTER_RADIUS = 0.055  # about 0.7 neighbours a point among 1025 uniform ones: half the stripped rows are empty


def scattered_cloud():
    """1025 uniform points, the first and the last two moved far from all others: with ``SCATTER_RADIUS`` their rows hold
    themselves alone."""
    pts = np.random.default_rng(77).uniform(0.0, 1.0, size=(1025, 3))
    pts[[0, 1023, 1024]] += np.array([[50.0, 0.0, 0.0], [0.0, 60.0, 0.0], [0.0, 0.0, 70.0]])
    return pts


def strip_self_arcs(rows):
    """CSR rows without the places ``index == row``, and the properties the tests of empty rows stand on, asserted from
    the stripped rows themselves: a third of the rows at least is empty, a third is not, row 0 and the last two are
    empty, and somewhere three empty rows follow one another."""
    offsets, index, d2 = (np.asarray(a) for a in rows)
    n = len(offsets) - 1
    row = np.repeat(np.arange(n), np.diff(offsets))
    keep = index != row
    length = np.bincount(row[keep], minlength=n)
    out = (np.concatenate([[0], np.cumsum(length)]).astype(np.int64), index[keep].astype(np.int32), d2[keep].astype(np.float64))
    empty = np.diff(out[0]) == 0
    assert 3 * empty.sum() >= n and 3 * (~empty).sum() >= n
    assert empty[0] and empty[n - 2] and empty[n - 1]
    assert (empty[:-2] & empty[1:-1] & empty[2:]).any()
    assert keep.sum() == len(out[1]) > 0 and not (out[1] == np.repeat(np.arange(n), np.diff(out[0]))).any()
    return out


def radius_rows(points, r):
    points = np.asarray(points, dtype=np.float64)
    n = len(points)
    offsets, index, out = [0], [], []
    for i in range(n):
        d2 = _d2_row(points, i)
        near = np.flatnonzero(d2 < r * r)
        near = near[np.lexsort((near, d2[near]))]
        index += near.tolist()
        out += d2[near].tolist()
        offsets.append(len(index))
    return np.array(offsets, dtype=np.int64), np.array(index, dtype=np.int32), np.array(out, dtype=np.float64)
