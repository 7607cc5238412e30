"""The checker of ``sc_graph_quotient`` (``csrc/graph_quotient.inl``): plain Python and NumPy loops written
from the rules Q1..Q4 of ``include/spacecarve.h``, sharing no code with the package.  ``tests/test_quotient_host.py``
holds it against ``nx.quotient_graph``."""
import numpy as np


def arcs_of(rows, extra=None):
    """``(n, [(i, j, w)])``: the arcs of ``(index [N, k], d2)`` or ``(offsets, index, d2)``, ``w = sqrt(d2)``, then the extra
    pairs with their plain weights.  Unused places (``-1``) and self-arcs are dropped (rule G1)."""
    rows = [np.asarray(a) for a in rows]
    arcs = []
    if len(rows) == 2:
        index, d2 = rows
        n = index.shape[0]
        for i in range(n):
            for j, v in zip(index[i].tolist(), d2[i].tolist()):
                if j >= 0 and j != i:
                    arcs.append((i, int(j), float(np.sqrt(np.float64(v)))))
    else:
        offsets, index, d2 = rows
        n = len(offsets) - 1
        for i in range(n):
            for e in range(int(offsets[i]), int(offsets[i + 1])):
                if int(index[e]) != i:
                    arcs.append((i, int(index[e]), float(np.sqrt(np.float64(d2[e])))))
    if extra is not None:
        for (i, j), w in zip(np.asarray(extra[0]).tolist(), np.asarray(extra[1]).tolist()):
            if i != j:
                arcs.append((int(i), int(j), float(w)))
    return n, arcs


def node_edges(arcs):
    """Rule Q4, first half: ``{(i, j): w}`` with ``i < j``, the least weight of the pair's arcs."""
    out = {}
    for i, j, w in arcs:
        pair = (min(i, j), max(i, j))
        if pair not in out or w < out[pair]:
            out[pair] = w
    return out


def clusters_of(labels, n_labels, key=None):
    """Rule Q1: ``(cluster int32 [N], members)``, ``members[c]`` the rising node list of cluster ``c``."""
    labels = np.asarray(labels).tolist()
    members = [[] for _ in range(n_labels)]
    for v, l in enumerate(labels):
        if l >= 0:
            members[l].append(v)
    used = [m for m in members if m]
    used.sort(key=lambda m: (min(int(key[v]) for v in m) if key is not None else 0, m[0]))
    cluster = np.full(len(labels), -1, dtype=np.int32)
    for c, m in enumerate(used):
        for v in m:
            cluster[v] = c
    return cluster, used


def quotient(rows, labels, n_labels, points=None, key=None, extra=None, weights=False):
    """``(cluster int32 [N], counts int32 [C], centers float64 [C, 3] | None, edges int32 [K, 2], edge_weights float64 [K] |
    None)`` by the rules Q1..Q4."""
    n, arcs = arcs_of(rows, extra)
    cluster, members = clusters_of(labels, n_labels, key)
    counts = np.array([len(m) for m in members], dtype=np.int32)
    centers = None
    if points is not None:
        points = np.asarray(points, dtype=np.float64)
        centers = np.zeros((len(members), 3))
        with np.errstate(all="ignore"):
            for c, m in enumerate(members):
                for a in range(3):
                    s = np.float64(0.0)
                    for v in m:  # rising v, left to right
                        s = s + points[v, a]
                    centers[c, a] = s / np.float64(len(m))
    sums = {}
    for (i, j), w in sorted(node_edges(arcs).items()):  # rising (i, j)
        a, b = int(cluster[i]), int(cluster[j])
        if a < 0 or b < 0 or a == b:
            continue
        e = (min(a, b), max(a, b))
        sums[e] = sums.get(e, 0.0) + w
    edges = np.array(sorted(sums), dtype=np.int32).reshape(-1, 2)
    edge_w = np.array([sums[e] for e in sorted(sums)], dtype=np.float64) if weights else None
    return cluster, counts, centers, edges, edge_w


# ---- the same rules in whole-array NumPy, for graphs of a million arcs: tests/test_quotient_host.py holds it against the
# loops above, which stay the authority.  Every float64 sum is np.bincount's, which adds its weights left to right. --------
def arcs_np(rows, extra=None):
    """``arcs_of`` as arrays: ``(n, i int64 [A'], j int64 [A'], w float64 [A'])``, in the order given."""
    rows = [np.asarray(a) for a in rows]
    if len(rows) == 2:
        index, d2 = rows
        n = index.shape[0]
        i = np.repeat(np.arange(n, dtype=np.int64), index.shape[1])
    else:
        offsets, index, d2 = rows
        n = len(offsets) - 1
        i = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets.astype(np.int64)))
    j = index.reshape(-1).astype(np.int64)
    with np.errstate(all="ignore"):
        w = np.sqrt(d2.reshape(-1).astype(np.float64))
    if extra is not None:
        pairs = np.asarray(extra[0], dtype=np.int64).reshape(-1, 2)
        i, j = np.concatenate([i, pairs[:, 0]]), np.concatenate([j, pairs[:, 1]])
        w = np.concatenate([w, np.asarray(extra[1], dtype=np.float64).reshape(-1)])
    keep = (j >= 0) & (j != i)
    return n, i[keep], j[keep], w[keep]


def clusters_np(labels, n_labels, key=None):
    """Rule Q1: ``(cluster int32 [N], counts int32 [C])``."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    cluster = np.full(len(labels), -1, dtype=np.int32)
    nodes = np.flatnonzero(labels >= 0)
    if len(nodes) == 0:
        return cluster, np.zeros(0, dtype=np.int32)
    order = nodes[np.lexsort((nodes, labels[nodes]))]  # by label, rising node inside a label
    heads = np.flatnonzero(np.concatenate([[True], labels[order][1:] != labels[order][:-1]]))
    used, smallest = labels[order][heads], order[heads]
    kmin = np.minimum.reduceat(np.asarray(key, dtype=np.int64)[order], heads) if key is not None else np.zeros(len(heads), dtype=np.int64)
    rank = np.lexsort((smallest, kmin))  # by (least key, smallest member)
    renumber = np.full(max(int(n_labels), 1), -1, dtype=np.int32)
    renumber[used[rank]] = np.arange(len(rank), dtype=np.int32)
    cluster[nodes] = renumber[labels[nodes]]
    return cluster, np.bincount(cluster[nodes], minlength=len(rank)).astype(np.int32)


def quotient_np(rows, labels, n_labels, points=None, key=None, extra=None, weights=False):
    """``quotient`` without a Python loop over nodes or arcs: the same signature, the same results bit for bit."""
    n, i, j, w = arcs_np(rows, extra)
    cluster, counts = clusters_np(labels, n_labels, key)
    C = len(counts)
    inside = cluster >= 0
    centers = None
    if points is not None:
        points = np.asarray(points, dtype=np.float64)
        with np.errstate(all="ignore"):
            centers = np.stack([np.bincount(cluster[inside], weights=points[inside, a], minlength=C) for a in range(3)], axis=1) \
                / counts.astype(np.float64)[:, None]
        centers = centers.reshape(C, 3)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    order = np.lexsort((hi, lo))  # rising (i, j)
    lo, hi, w = lo[order], hi[order], w[order]
    heads = np.flatnonzero(np.concatenate([[True], (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])])) if len(lo) else np.zeros(0, dtype=np.int64)
    lo, hi = lo[heads], hi[heads]
    least = np.minimum.reduceat(w, heads) if len(heads) else np.zeros(0)  # the least weight of the pair's arcs
    a, b = cluster[lo].astype(np.int64), cluster[hi].astype(np.int64)
    cross = (a >= 0) & (b >= 0) & (a != b)
    code = np.minimum(a, b)[cross] * max(C, 1) + np.maximum(a, b)[cross]
    found, place = np.unique(code, return_inverse=True)
    edges = np.stack([found // max(C, 1), found % max(C, 1)], axis=1).astype(np.int32).reshape(-1, 2)
    edge_w = np.bincount(place.reshape(-1), weights=least[cross], minlength=len(found)).astype(np.float64) if weights else None
    return cluster, counts, centers, edges, edge_w


def crossing_np(rows, cluster, extra=None):
    """The arcs, as given and in both directions where both are given, whose ends lie in two different clusters: the
    device's count X, which sizes its sorts."""
    _, i, j, _ = arcs_np(rows, extra)
    a, b = np.asarray(cluster)[i], np.asarray(cluster)[j]
    return int(((a >= 0) & (b >= 0) & (a != b)).sum())


def pairs_per_edge(rows, cluster, extra=None):
    """``{(a, b): number of undirected node pairs that join clusters a < b}``: the terms of each weight's sum."""
    _, arcs = arcs_of(rows, extra)
    out = {}
    for i, j in node_edges(arcs):
        a, b = int(cluster[i]), int(cluster[j])
        if a >= 0 and b >= 0 and a != b:
            e = (min(a, b), max(a, b))
            out[e] = out.get(e, 0) + 1
    return out


def same_bits(got, want):
    """Equal bit for bit, any NaN standing for any NaN (a NaN's payload is not part of the rules)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != np.float64:
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64)))


def d2_rows_knn(points, k):
    """knn rows by ``scipy.spatial.cKDTree`` with d2 by rule N1 (bitwise symmetric): ``(index int32 [n, k], d2 [n, k])``."""
    from scipy.spatial import cKDTree
    points = np.asarray(points, dtype=np.float64)
    k = min(k, len(points))
    _, index = cKDTree(points).query(points, k=k)
    index = np.asarray(index).reshape(len(points), k)
    diff = points[:, None, :] - points[index]
    d2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    return index.astype(np.int32), d2

