"""The checker of ``sc_graph_connect`` / ``proc3d.connect_edges`` (rules C1, C2 of ``include/spacecarve.h``):
Prim's algorithm over the labels in its incremental form, NumPy only, sharing no code with the package.
``tests/test_connect_host.py`` pins it, ``array_equal``, against the brute force over all pairs,
``tests/graph_oracle.connect_edges``, which is the ground truth but takes seconds for a few hundred points."""
import numpy as np


def d2_to(points, i, ids):
    """Rule N1 from point ``i`` to the points ``ids``: ``((dx dx) + (dy dy)) + (dz dz)`` in float64, in this order."""
    diff = points[i][None, :] - points[ids]
    return (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]


def connect_edges(points, labels, root):
    """``(edges int32 [M, 2], weights float64 [M])``: every outside point keeps the least ``(d2, j)`` it has seen among the
    inside points; when a label joins, only its points are offered to the points still outside; the next edge is the
    outside point with the least ``(d2, i, j)``."""
    points = np.asarray(points, dtype=np.float64)
    labels = np.asarray(labels).reshape(-1)
    n = len(points)
    inside = np.zeros(n, dtype=bool)
    best_d = np.full(n, np.inf)
    best_j = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
    edges, weights = [], []
    joining = labels[root] if n else None
    while n:
        new = np.flatnonzero((labels == joining) & ~inside)
        inside[new] = True
        out = np.flatnonzero(~inside)
        if len(out) == 0:
            break
        for j in new.tolist():  # offered one at a time: (d2, j) is compared as a pair, whatever the order of the offers
            d2 = d2_to(points, j, out)  # bitwise symmetric: (a - b)^2 == (b - a)^2
            better = (d2 < best_d[out]) | ((d2 == best_d[out]) & (j < best_j[out]))
            best_d[out[better]] = d2[better]
            best_j[out[better]] = j
        order = np.lexsort((best_j[out], out, best_d[out]))  # the least (d2, i, j)
        i = int(out[order[0]])
        edges.append((i, int(best_j[i])))
        weights.append(np.sqrt(best_d[i]))
        joining = labels[i]
    return np.array(edges, dtype=np.int32).reshape(-1, 2), np.array(weights, dtype=np.float64)


def components_within(points, radius):
    """Labels ``0 .. C - 1`` of the components of the graph that joins points with ``d2 < radius * radius``, numbered by
    smallest member; ``(labels int32 [n], C)``.  Brute force: for the clouds of the host tests, where no device searches."""
    points = np.asarray(points, dtype=np.float64)
    n = len(points)
    labels = np.full(n, -1, dtype=np.int32)
    count = 0
    for s in range(n):
        if labels[s] >= 0:
            continue
        labels[s] = count
        stack = [s]
        while stack:
            v = stack.pop()
            near = np.flatnonzero((d2_to(points, v, np.arange(n)) < radius * radius) & (labels < 0))
            labels[near] = count
            stack += near.tolist()
        count += 1
    return labels, count
