"""The checker of ``proc3d.radius_points`` / ``radius_counts`` and ``radius_edges`` / ``radius_graph``,
NumPy and SciPy only.

open3d is not available here: PARITY UNPINNED.  Candidates may come from anywhere (all pairs, or a k-d
tree asked for everything within the radius, inflated); what the answer IS is decided by four rules:
  R1. ``d2`` is N1 of tests/nearest_oracle.py (``dist2``), every operation rounded once;
  R2. a target is a neighbour iff ``d2 < radius * radius`` (strict, the product rounded once in float64);
  R3. a row holds all its neighbours in rising key ``(d2, index)``, compared lexicographically (``np.lexsort``);
  R4. the answer is in CSR form: ``offsets`` int64 ``[Q + 1]`` from 0, ``index`` int32 ``[E]``, ``d2`` float64 ``[E]``.
"""
import numpy as np

from tests.nearest_oracle import _clouds, dist2


def _md2(radius):
    return np.float64(radius) * np.float64(radius)


def _csr(rows_index, rows_d2, Q):
    """R4 from the rows."""
    offsets = np.zeros(Q + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(r) for r in rows_index], dtype=np.int64)
    index = np.concatenate(rows_index).astype(np.int32) if rows_index else np.zeros(0, dtype=np.int32)
    d2 = np.concatenate(rows_d2).astype(np.float64) if rows_d2 else np.zeros(0, dtype=np.float64)
    return offsets, index.reshape(-1), d2.reshape(-1)


def _row(d, cand, md2):
    """R2 and R3 over the candidates ``cand`` (target indices) with their ``d2`` values ``d``: one row."""
    keep = d < md2
    d, cand = d[keep], cand[keep]
    order = np.lexsort((cand, d))  # the last key is the primary one: d2, then the index
    return cand[order], d[order]


def radius_all_pairs(queries, targets, radius, piece=1024):
    """The literal form: N1 over ``[Q, P]`` (``piece`` queries at a time), R2, ``np.lexsort`` by ``(d2, index)``, R4."""
    q, t = _clouds(queries, targets)
    md2 = _md2(radius)
    rows_index, rows_d2 = [], []
    if len(t) == 0:
        return _csr([np.zeros(0, dtype=np.int64)] * len(q), [np.zeros(0)] * len(q), len(q))
    for a in range(0, len(q), piece):
        d = dist2(q[a:a + piece, None, :], t[None, :, :])
        inside = d < md2
        if inside.all():  # every target in every row: one sort of the whole piece
            order = np.lexsort((np.broadcast_to(np.arange(len(t)), d.shape), d), axis=1)
            rows_index.extend(order)
            rows_d2.extend(np.take_along_axis(d, order, axis=1))
            continue
        for r in range(d.shape[0]):
            cand = np.flatnonzero(inside[r])
            i, dd = _row(d[r, cand], cand, md2)
            rows_index.append(i)
            rows_d2.append(dd)
    return _csr(rows_index, rows_d2, len(q))


def radius(queries, targets, radius, workers=-1):
    """The k-d tree form for larger clouds: ``query_ball_point`` at ``radius (1 + 1e-9)`` gives the candidates; R1-R3
    over them decide.  The tree's arithmetic decides nothing: every target whose true distance is below the radius is a
    candidate, the inflation covering the rounding of the tree's own distances."""
    from scipy.spatial import cKDTree
    q, t = _clouds(queries, targets)
    md2 = _md2(radius)
    if len(t) == 0 or len(q) == 0:
        return _csr([np.zeros(0, dtype=np.int64)] * len(q), [np.zeros(0)] * len(q), len(q))
    cands = cKDTree(t).query_ball_point(q, float(radius) * (1.0 + 1e-9) + np.finfo(np.float64).tiny, workers=workers)
    rows_index, rows_d2 = [], []
    for r in range(len(q)):
        c = np.asarray(cands[r], dtype=np.int64)
        i, dd = _row(dist2(q[r][None, :], t[c]), c, md2)
        rows_index.append(i)
        rows_d2.append(dd)
    return _csr(rows_index, rows_d2, len(q))


def counts(offsets):
    return np.diff(offsets).astype(np.int32)


def reference_radius_graph(points, r, radius_fn=radius_all_pairs):
    """``plant3dvision/proc3d.py:186-209`` restated literally, with the checker's search in place of the tree:
    ``(nodes, edges {(min, max): weight})`` as the ``networkx.Graph`` of the reference would hold them -- ``add_edge`` on
    an undirected graph overwrites the weight of an edge that exists, the self-loop ``i-i`` included; the nodes carry
    no attribute."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    offsets, index, _ = radius_fn(pts, pts, r)
    nodes, edges = [], {}
    for i in range(len(pts)):
        idx = [int(j) for j in index[offsets[i]:offsets[i + 1]]]
        k_ = len(idx)
        nodes.append(i)
        for j in range(k_):
            edges[(min(i, idx[j]), max(i, idx[j]))] = float(np.linalg.norm(pts[i] - pts[idx[j]]))
    return nodes, edges
