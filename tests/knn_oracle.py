"""The checker of ``proc3d.knn_points`` and ``proc3d.knn_edges`` / ``knn_graph``, NumPy and SciPy only.

open3d is not available here: PARITY UNPINNED.  Candidates may come from anywhere (all pairs, or a k-d
tree asked for everything within its own k-th distance, inflated); what the answer IS is decided by four rules:
  K1. ``d2`` is N1 of tests/nearest_oracle.py (``dist2``), every operation rounded once;
  K2. the key of a target is ``(d2, index)``, compared lexicographically; a row holds the ``min(k, matched)`` smallest
      keys in rising key order (``np.lexsort``), so a tie at the k-th place goes to the smaller index;
  K3. with ``max_distance`` only targets with ``d2 < max_distance * max_distance`` count (strict, the product rounded
      once);
  K4. a row has ``k`` places; the unused ones, after the used ones, hold ``-1`` and ``+inf``.
"""
import numpy as np

from tests.nearest_oracle import _clouds, dist2


def _row(d, cand, k, md2):
    """K2-K4 over the candidates ``cand`` (target indices) with their ``d2`` values ``d``: one row of the answer."""
    index, d2 = np.full(k, -1, dtype=np.int32), np.full(k, np.inf)
    if md2 is not None:
        keep = d < md2
        d, cand = d[keep], cand[keep]
    order = np.lexsort((cand, d))[:k]  # the last key is the primary one: d2, then the index
    index[:len(order)], d2[:len(order)] = cand[order], d[order]
    return index, d2


def _md2(max_distance):
    return None if max_distance is None else np.float64(max_distance) * np.float64(max_distance)


def knn_all_pairs(queries, targets, k, max_distance=None, piece=2048):
    """The literal form: N1 over ``[Q, P]`` (``piece`` queries at a time), ``np.lexsort`` by ``(d2, index)``, the first
    ``k``, then K3 and K4."""
    q, t = _clouds(queries, targets)
    index, d2 = np.full((len(q), k), -1, dtype=np.int32), np.full((len(q), k), np.inf)
    if len(t) == 0:
        return index, d2
    md2, n = _md2(max_distance), min(k, len(t))
    for a in range(0, len(q), piece):
        d = dist2(q[a:a + piece, None, :], t[None, :, :])
        order = np.lexsort((np.broadcast_to(np.arange(len(t)), d.shape), d), axis=1)[:, :n]  # by d2, then by index
        least = np.take_along_axis(d, order, axis=1)
        used = np.ones(least.shape, dtype=bool) if md2 is None else least < md2  # a prefix of each row: d2 rises
        index[a:a + piece, :n] = np.where(used, order, -1)
        d2[a:a + piece, :n] = np.where(used, least, np.inf)
    return index, d2


def knn(queries, targets, k, max_distance=None):
    """The k-d tree form for larger clouds: the tree's k-th distance times ``1 + 1e-9`` gives the candidates
    (``query_ball_point``; with fewer than ``k`` targets, all of them); K1-K4 over them.  The tree's arithmetic decides
    nothing: every target whose true distance is within the k-th one is a candidate, the inflation covering the
    rounding of the tree's own distances."""
    from scipy.spatial import cKDTree
    q, t = _clouds(queries, targets)
    index, d2 = np.full((len(q), k), -1, dtype=np.int32), np.full((len(q), k), np.inf)
    if len(t) == 0 or len(q) == 0:
        return index, d2
    md2 = _md2(max_distance)
    if len(t) <= k:
        cands = [np.arange(len(t))] * len(q)
    else:
        tree = cKDTree(t)
        dist, _ = tree.query(q, k, workers=-1)
        kth = dist[:, -1] if k > 1 else np.asarray(dist).reshape(len(q))
        cands = tree.query_ball_point(q, kth * (1.0 + 1e-9) + np.finfo(np.float64).tiny, workers=-1)
    for r in range(len(q)):
        c = np.asarray(cands[r], dtype=np.int64)
        index[r], d2[r] = _row(dist2(q[r][None, :], t[c]), c, k, md2)
    return index, d2


def reference_knn_graph(points, k, knn_fn=knn_all_pairs):
    """``plant3dvision/proc3d.py:160-183`` restated literally, with the checker's search in place of the tree:
    ``(nodes {i: center}, edges {(min, max): weight})`` as the ``networkx.Graph`` of the reference would hold them --
    ``add_edge`` on an undirected graph overwrites the weight of an edge that exists, the self-loop ``i-i`` included."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    index, _ = knn_fn(pts, pts, k)
    nodes, edges = {}, {}
    for i in range(len(pts)):
        idx = [int(j) for j in index[i] if j >= 0]
        k_ = len(idx)
        nodes[i] = pts[i]
        for j in range(k_):
            edges[(min(i, idx[j]), max(i, idx[j]))] = float(np.linalg.norm(pts[i] - pts[idx[j]]))
    return nodes, edges
