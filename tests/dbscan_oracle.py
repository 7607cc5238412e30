"""The checker of ``proc3d.cluster_dbscan``: open3d's ``cluster_dbscan`` loop, restated literally.

open3d is not available here and its source is not either: PARITY UNPINNED.  ``labels`` is the
sequential procedure as open3d runs it -- a label array that starts at -2 (unvisited), -1 for noise, points walked in
index order, one cluster grown at a time from a work set, noise promoted to border, everything already labelled
skipped -- and deliberately NOT the order-free form the kernels build (``labels_order_free`` is that form,
vectorised, for clouds too large for the loop; tests/test_dbscan_host.py ties the two together).

Candidate pairs may come from anywhere (all pairs, or a k-d tree with an inflated radius); what a pair IS is decided
by two rules alone:
  1. ``d2(i, j) = ((dx dx) + (dy dy)) + (dz dz)`` in IEEE binary64, every operation rounded once (NumPy does not
     contract);
  2. ``j`` is a neighbour of ``i`` iff ``d2(i, j) < eps * eps``: strict, the product rounded once, ``i`` is its own
     neighbour (nanoflann's radius search accepts ``dist^2 < radius^2``).
"""
import numpy as np

BRUTE_MAX = 3000  # all pairs up to here (9e6 distances); a k-d tree with an inflated radius above


def dist2(a, b):
    """Rule 1 for arrays of points ``[..., 3]``."""
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return ((dx * dx) + (dy * dy)) + (dz * dz)


def neighbour_pairs(points, eps):
    """All ordered pairs (i, j), i == j included, with ``d2(i, j) < eps * eps`` (rules 1 and 2), sorted by (i, j)."""
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    P = pts.shape[0]
    eps2 = np.float64(eps) * np.float64(eps)
    if P <= BRUTE_MAX:
        i, j = np.nonzero(dist2(pts[:, None, :], pts[None, :, :]) < eps2)
        return i.astype(np.int64), j.astype(np.int64)
    from scipy.spatial import cKDTree
    # candidates only: the tree's own arithmetic decides nothing, the radius is inflated far beyond its rounding
    cand = cKDTree(pts).query_pairs(float(eps) * (1.0 + 1e-6), output_type="ndarray")
    ok = dist2(pts[cand[:, 0]], pts[cand[:, 1]]) < eps2
    a, b = cand[ok, 0].astype(np.int64), cand[ok, 1].astype(np.int64)
    own = np.nonzero(dist2(pts, pts) < eps2)[0].astype(np.int64)
    i, j = np.concatenate([a, b, own]), np.concatenate([b, a, own])
    order = np.lexsort((j, i))
    return i[order], j[order]


def neighbour_lists(points, eps):
    """CSR form of ``neighbour_pairs``: (indptr [P + 1], indices)."""
    P = np.asarray(points).reshape(-1, 3).shape[0]
    i, j = neighbour_pairs(points, eps)
    indptr = np.zeros(P + 1, dtype=np.int64)
    np.cumsum(np.bincount(i, minlength=P), out=indptr[1:])
    return indptr, j


def labels(points, eps, min_points, pop=None):
    """The literal loop.  ``pop(work_set)`` removes and returns one element: ``set.pop`` (arbitrary) by default;
    the tests force orders of their own to show that the result does not depend on it."""
    P = np.asarray(points).reshape(-1, 3).shape[0]
    indptr, indices = neighbour_lists(points, eps)
    nbs = [indices[indptr[q]:indptr[q + 1]].tolist() for q in range(P)]
    if pop is None:
        pop = set.pop
    lab = [-2] * P
    cluster = 0
    for idx in range(P):
        if lab[idx] != -2:
            continue
        if len(nbs[idx]) < min_points:
            lab[idx] = -1
            continue
        work = set(nbs[idx])
        visited = {idx}
        lab[idx] = cluster
        while work:
            nb = pop(work)
            visited.add(nb)
            if lab[nb] == -1:  # noise so far: a border point of this cluster
                lab[nb] = cluster
            if lab[nb] != -2:
                continue
            lab[nb] = cluster
            if len(nbs[nb]) >= min_points:
                for q in nbs[nb]:
                    if q not in visited:
                        work.add(q)
        cluster += 1
    return np.array(lab, dtype=np.int32).reshape(P)


def pop_min(work):
    q = min(work)
    work.remove(q)
    return q


def pop_max(work):
    q = max(work)
    work.remove(q)
    return q


def structure(points, eps, min_points):
    """What a cloud exercises: dict of ``core`` (bool [P]), ``border`` (non-core with a core neighbour), ``contested``
    (border points whose core neighbours lie in more than one cluster), ``ties`` (unordered pairs at exactly
    ``d2 == eps * eps``; all pairs, so for small clouds only)."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    P = pts.shape[0]
    i, j = neighbour_pairs(pts, eps)
    core = np.bincount(i, minlength=P) >= max(int(min_points), 0)
    lab = labels(pts, eps, min_points)
    cc = core[j] & ~core[i]  # pairs (non-core i, core j)
    border = np.zeros(P, dtype=bool)
    border[i[cc]] = True
    lo = np.full(P, np.iinfo(np.int32).max, dtype=np.int64)
    hi = np.full(P, -1, dtype=np.int64)
    np.minimum.at(lo, i[cc], lab[j[cc]])
    np.maximum.at(hi, i[cc], lab[j[cc]])
    contested = border & (lo != hi)
    ties = -1
    if P <= BRUTE_MAX:
        d2 = dist2(pts[:, None, :], pts[None, :, :])
        ties = int(np.count_nonzero(np.triu(d2 == np.float64(eps) * np.float64(eps), 1)))
    return dict(core=core, border=border, contested=contested, ties=ties, labels=lab)


def labels_order_free(points, eps, min_points):
    """The order-free form (rules 3-6), vectorised: core flags from the neighbour counts, connected
    components of the core-core pairs, ids by the rank of each component's smallest index, border points to the
    smallest id among their core neighbours.  For clouds too large for the literal loop."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    P = pts.shape[0]
    out = np.full(P, -1, dtype=np.int32)
    if P == 0:
        return out
    i, j = neighbour_pairs(pts, eps)
    core = np.bincount(i, minlength=P) >= int(min_points)
    if not core.any():
        return out
    ee = core[i] & core[j]
    graph = coo_matrix((np.ones(int(ee.sum()), dtype=np.int8), (i[ee], j[ee])), shape=(P, P))
    _, comp = connected_components(graph, directed=False)
    first = np.full(comp.max() + 1, P, dtype=np.int64)  # smallest CORE index of each component
    np.minimum.at(first, comp[core], np.nonzero(core)[0])
    roots = np.sort(first[first < P])
    ids = np.searchsorted(roots, first)  # component -> rank of its smallest index (components of non-core: unused)
    out[core] = ids[comp[core]]
    bc = ~core[i] & core[j]
    best = np.full(P, np.iinfo(np.int32).max, dtype=np.int64)
    np.minimum.at(best, i[bc], out[j[bc]])
    hit = best != np.iinfo(np.int32).max
    out[hit] = best[hit]
    return out


# ---- the clouds the tests share ---------------------------------------------------------------------------------
BLOBS = dict(eps=0.9, min_points=5)
LATTICE = dict(eps=2.0, min_points=5)


def blobs_cloud(seed=7):
    """1900 points: four Gaussian blobs of 350 (two of them close enough to contest border points) and 500 points of
    uniform noise.  Continuous coordinates: no pair lies at exactly ``eps``."""
    rng = np.random.default_rng(seed)
    centres = np.array([[0.0, 0.0, 0.0], [6.5, 0.0, 0.0], [0.0, 12.0, 3.0], [10.0, 10.0, -4.0]])
    parts = [c + rng.normal(scale=1.3, size=(350, 3)) for c in centres]
    parts.append(rng.uniform(-6.0, 16.0, size=(500, 3)))
    return np.ascontiguousarray(np.concatenate(parts))


def lattice_cloud(seed=11, n=14, share=0.18):
    """Integer points of a seeded ``n^3`` occupancy: with ``eps = 2.0`` pairs at exactly ``eps`` are everywhere."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.argwhere(rng.random((n, n, n)) < share).astype(np.float64))
