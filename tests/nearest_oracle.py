"""The checker of ``proc3d.nearest_points`` and the cloud metrics over it, NumPy only.

open3d is not available here: PARITY UNPINNED.  Candidates may come from anywhere (all pairs, or a k-d
tree asked for everything within its own nearest distance, inflated); what the answer IS is decided by three rules:
  N1. ``d2(q, t) = ((dx dx) + (dy dy)) + (dz dz)`` in IEEE binary64, every operation rounded once, ``dx = qx - tx``;
  N2. the nearest target is the one of least ``d2``; among equal ``d2`` the smallest target index wins;
  N3. with ``max_distance`` a query is matched iff ``d2 < max_distance * max_distance`` (strict, the product rounded
      once); an unmatched query reports ``-1`` and ``+inf``.
The sums are ``math.fsum`` of the matched terms.  ``compare_segmented`` is the reference's
``CompareSegmentedPointClouds._compare`` loop, restated over the checker's indices.
"""
import math

import numpy as np


def dist2(a, b):
    """N1 for arrays of points ``[..., 3]``."""
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return ((dx * dx) + (dy * dy)) + (dz * dz)


def _clouds(queries, targets):
    queries, targets = (getattr(c, "points", c) if not isinstance(c, np.ndarray) else c for c in (queries, targets))
    q = np.ascontiguousarray(np.asarray(queries, dtype=np.float64).reshape(-1, 3))
    t = np.ascontiguousarray(np.asarray(targets, dtype=np.float64).reshape(-1, 3))
    return q, t


def _bound(index, d2, max_distance):
    """N3 applied to the unbounded answer."""
    if max_distance is not None:
        out = ~(d2 < np.float64(max_distance) * np.float64(max_distance))
        index, d2 = index.copy(), d2.copy()
        index[out] = -1
        d2[out] = np.inf
    return index.astype(np.int32), d2


def nearest_all_pairs(queries, targets, max_distance=None):
    """The literal form for small clouds: ``np.argmin`` over N1's expression (the first least: the smallest index)."""
    q, t = _clouds(queries, targets)
    if len(t) == 0 or len(q) == 0:
        return np.full(len(q), -1, dtype=np.int32), np.full(len(q), np.inf)
    d = dist2(q[:, None, :], t[None, :, :])
    index = np.argmin(d, axis=1)
    return _bound(index, d[np.arange(len(q)), index], max_distance)


def nearest_in_pieces(queries, targets, max_distance=None, piece=16384):
    """``nearest_all_pairs`` for many queries against few targets: the same literal form, ``piece`` queries at a time."""
    q, t = _clouds(queries, targets)
    parts = [nearest_all_pairs(q[k:k + piece], t, max_distance) for k in range(0, len(q), piece)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def nearest(queries, targets, max_distance=None, return_ties=False):
    """The k-d tree form: N1 and N2 over EVERY candidate ``query_ball_point`` returns within the tree's own nearest
    distance times ``1 + 1e-9`` (plus the tree's own answer); the tree's arithmetic decides nothing.
    ``return_ties``: also the number of queries whose least ``d2`` more than one target has."""
    from scipy.spatial import cKDTree
    q, t = _clouds(queries, targets)
    if len(t) == 0 or len(q) == 0:
        out = np.full(len(q), -1, dtype=np.int32), np.full(len(q), np.inf)
        return out + (0,) if return_ties else out
    tree = cKDTree(t)
    dist, first = tree.query(q)
    radius = dist * (1.0 + 1e-9) + np.finfo(np.float64).tiny
    cands = tree.query_ball_point(q, radius)
    index = np.empty(len(q), dtype=np.int64)
    d2 = np.empty(len(q), dtype=np.float64)
    ties = 0
    for k in range(len(q)):
        c = np.unique(np.concatenate([np.asarray(cands[k], dtype=np.int64), [first[k]]]))  # sorted: argmin takes the smallest index
        d = dist2(q[k][None, :], t[c])
        j = int(np.argmin(d))
        index[k], d2[k] = c[j], d[j]
        ties += int(np.count_nonzero(d == d[j]) > 1)
    out = _bound(index, d2, max_distance)
    return out + (ties,) if return_ties else out


def sums(d2):
    """N6: ``(n, fsum d2, fsum sqrt d2)`` over the matched queries."""
    m = np.isfinite(d2)
    return int(m.sum()), math.fsum(d2[m].tolist()), math.fsum(np.sqrt(d2[m]).tolist())


def sums_tolerance(Q):
    """N6's bound, relative: any order of adding Q non-negative terms is within ``(Q - 1) u / (1 - (Q - 1) u)``,
    ``u = 2^-53``, of the exact sum; the tests use ``(Q + 8) 2^-52``, the 8 for the square roots."""
    return (Q + 8) * 2.0 ** -52


def chamfer_distance(a, b):
    a, b = _clouds(a, b)
    _, da = nearest(a, b)
    _, db = nearest(b, a)
    return sums(da)[2] / len(a) + sums(db)[2] / len(b)


def registration_fitness(source, target, max_distance=2):
    """``(fitness, inlier_rmse)`` as open3d's ``evaluate_registration`` defines them; 0.0, 0.0 without a match."""
    source, target = _clouds(source, target)
    _, d2 = nearest(source, target, max_distance)
    n, s2, _ = sums(d2)
    if len(source) == 0 or n == 0:
        return 0.0, 0.0
    return n / len(source), math.sqrt(s2 / n)


def tables(source, source_ids, target, target_ids, n_labels, nearest_fn=nearest):
    """``counts[a, b]``: source points of label id ``a`` whose nearest target has label id ``b``."""
    index, _ = nearest_fn(source, target)
    out = np.zeros((n_labels, n_labels), dtype=np.int64)
    ok = index >= 0
    np.add.at(out, (np.asarray(source_ids)[ok], np.asarray(target_ids)[index[ok]]), 1)
    return out


def _compare(unique_labels, source, source_labels, target, target_labels):
    """metrics.py:449-519, the loop over the points with the nearest index taken from the checker."""
    index, _ = nearest(source, target)
    results = {label: {"tp": 0, "fp": 0, "tn": 0, "fn": 0, "precision": None, "recall": None, "iou": None} for label in unique_labels}
    for k in range(len(index)):
        source_label, target_label = source_labels[k], target_labels[index[k]]
        for label in unique_labels:
            if source_label == label and target_label == label:
                results[label]["tp"] += 1
            elif source_label == label and target_label != label:
                results[label]["fp"] += 1
            elif source_label != label and target_label == label:
                results[label]["fn"] += 1
            else:
                results[label]["tn"] += 1
    for label in unique_labels:
        r = results[label]
        if r["tp"] + r["fp"] > 0:
            r["precision"] = r["tp"] / (r["tp"] + r["fp"])
        if r["tp"] + r["fn"] > 0:
            r["recall"] = r["tp"] / (r["tp"] + r["fn"])
        if r["tp"] + r["fn"] + r["fp"] > 0:
            r["iou"] = r["tp"] / (r["tp"] + r["fn"] + r["fp"])
    return results


def compare_segmented(groundtruth, groundtruth_labels, prediction, prediction_labels):
    """The ``results`` dictionary of the reference's ``CompareSegmentedPointClouds``."""
    unique = set(groundtruth_labels)
    res = {"groundtruth-to-prediction": _compare(unique, groundtruth, groundtruth_labels, prediction, prediction_labels),
           "prediction-to-groundtruth": _compare(unique, prediction, prediction_labels, groundtruth, groundtruth_labels),
           "miou": {}}
    for label in unique:
        a, b = res["groundtruth-to-prediction"][label]["iou"], res["prediction-to-groundtruth"][label]["iou"]
        res["miou"][label] = (a + b) / 2.0 if a is not None and b is not None else None
    return res


# ---- the clouds the tests share -----------------------------------------------------------------------------------
def blob_targets(queries, seed=3):
    """A seeded jittered copy of ``queries`` (normal, scale 0.8: a point's own copy is beyond 0.5 for most and beyond 2
    for about a tenth) plus 600 uniform points, permuted."""
    rng = np.random.default_rng(seed)
    t = np.concatenate([queries + rng.normal(scale=0.8, size=queries.shape), rng.uniform(-6.0, 16.0, size=(600, 3))])
    return np.ascontiguousarray(t[rng.permutation(len(t))])


def tie_clouds(seed=5):
    """Targets: the 6^3 integer lattice, permuted, then three extra copies of four of its points.  Queries (200): cell
    centres (8-way ties), edge midpoints (2-way), lattice points (d2 = 0; where a copy exists the smaller index wins)."""
    rng = np.random.default_rng(seed)
    lattice = np.argwhere(np.ones((6, 6, 6), dtype=bool)).astype(np.float64)
    lattice = lattice[rng.permutation(len(lattice))]
    targets = np.concatenate([lattice, np.tile(lattice[[3, 50, 100, 200]], (3, 1))])
    centres = rng.integers(0, 5, size=(80, 3)) + 0.5
    edges = rng.integers(0, 5, size=(70, 3)).astype(np.float64)
    edges[np.arange(70), rng.integers(0, 3, size=70)] += 0.5
    on = np.concatenate([lattice[[3, 50, 100, 200]], rng.integers(0, 6, size=(46, 3)).astype(np.float64)])
    return np.ascontiguousarray(np.concatenate([centres, edges, on])), np.ascontiguousarray(targets)


# ---- the launch geometry of csrc/nearest.hip, for the tests that go past its capped grids ---------------------------
# Nothing below decides a result.  The caps are read out of the sources' text (a constant that is no longer there fails
# loudly: tests/test_unit_plans_host.py), the grid is sc_nearest.h's plan restated: with them a test can say, from its
# inputs alone, that a thread takes a second trip through its loop or that the far pass has more queries than wavefronts.
FAR_P, FAR_Q, FAR_NEAR_EVERY = 600, 9300, 31      # a far list longer than the far pass has wavefronts; 300 near queries
SUMS_Q, SUMS_P = 66000, 64                         # queries past the blocks of the sums launch
LATE_P = 65836                                     # targets past the blocks of the box launch
LATE_Q = 262144 + 300                              # device queries whose judge takes a trip more than an uncapped grid's 3
CONFUSION_Q, CONFUSION_P = 262144 + 777, 1000      # queries past the blocks of the labels and confusion launches


def launch_caps():
    """The block size and the block caps of nearest.hip's launches, and of sc_points.h's judge of device points."""
    from tests.evaluation_oracle import source_constant
    caps = {name: source_constant("nearest.hip", name) for name in ("kB", "kPartials", "kFarBlocks", "kLdsTable")}
    caps["kNearRings"] = source_constant("sc_nearest.h", "kNearRings")
    caps["label_blocks"] = source_constant("nearest.hip", "the cap of sc_nearest_confusion's grids",
                                           r"std::min<int64_t>\(\(std::max\(Q, P\) \+ kB - 1\) / kB,\s*(\d+)\)")
    caps["finite_blocks"] = source_constant("sc_points.h", "the cap of launch_points_finite's grid",
                                            r"std::min<int64_t>\(\(n \+ 255\) / 256,\s*(\d+)\)")
    return caps


def _stride(n, block, cap):
    return min((n + block - 1) // block, cap) * block


def box_stride(P):
    """Targets a trip of ``nearest_box_kernel``'s loop takes; a target of index >= this is seen on a later trip."""
    caps = launch_caps()
    return _stride(P, caps["kB"], caps["kPartials"])


def sums_stride(Q):
    """The same for the queries of ``nearest_sums_kernel``."""
    return box_stride(Q)


def finite_stride(n):
    """COORDINATES (of the 3 n) a trip of ``points_finite_kernel``'s loop takes for n points."""
    return _stride(n, 256, launch_caps()["finite_blocks"])


def labels_stride(Q, P):
    """Elements a trip of ``nearest_labels_kernel``'s and ``nearest_confusion_kernel``'s loops takes."""
    caps = launch_caps()
    return _stride(max(Q, P), caps["kB"], caps["label_blocks"])


def far_waves(Q):
    """Wavefronts of ``nearest_far_kernel``: a far list longer than this makes them go round."""
    caps = launch_caps()
    return min((Q + 3) // 4, caps["kFarBlocks"]) * (caps["kB"] // 64)


K_MAX_CELLS, K_SHRINK, K_EDGE_MIN, K_EDGE_MAX, K_PLAN_STEPS = 1 << 22, 1.0 - 2.0 ** -20, 2.0 ** -480, 2.0 ** 480, 8192


def plan_grid(targets):
    """``nn::plan_grid`` over the targets' bounding box: ``(lo, h, n)``."""
    t = np.asarray(targets, dtype=np.float64).reshape(-1, 3)
    lo, hi = t.min(axis=0), t.max(axis=0)
    cap = float(min(max(2 * len(t), 64), K_MAX_CELLS))
    ext = hi - lo
    n = np.ones(3, dtype=np.int64)
    if not np.all(np.isfinite(ext)) or not (ext > 0.0).any():
        return lo, 1.0, n
    k = int((ext > 0.0).sum())
    h = math.exp((sum(math.log(e) for e in ext if e > 0.0) - math.log(cap / 2.0)) / k)
    for _ in range(K_PLAN_STEPS):
        if h >= K_EDGE_MIN:
            if not h <= K_EDGE_MAX:
                break
            cnt = np.floor(ext / h) + 1.0
            if cnt[0] * cnt[1] * cnt[2] <= cap:
                return lo, h, cnt.astype(np.int64)
        h *= 1.25
    return lo, 1.0, n


def cell_of(x, lo, h, n):
    """``nn::cell_of`` for arrays ``[..., 3]``."""
    with np.errstate(over="ignore"):
        return np.minimum(np.maximum(np.floor((x - lo) / h), 0.0), (n - 1).astype(np.float64)).astype(np.int64)


def ring_bound(h, r):
    """``nn::ring_bound``."""
    hr = h * float(r)
    return (hr * hr) * K_SHRINK


def certainly_far(queries, targets, d2, max_distance=None):
    """How many queries the rings cannot settle, whatever the last bit of ``h`` is: the ring that reaches every far face
    lies beyond ``kNearRings``, and the bound after ring ``kNearRings``, raised by 1e-9, is still below the query's true
    ``d2`` (the checker's) and below ``md2``.  A condition on the inputs, not a tolerance on the kernel."""
    rings = launch_caps()["kNearRings"]
    lo, h, n = plan_grid(targets)
    c = cell_of(np.asarray(queries, dtype=np.float64).reshape(-1, 3), lo, h, n)
    last = np.maximum(c, n - 1 - c).max(axis=1)
    bound = ring_bound(h, rings) * (1.0 + 1e-9)
    md2 = np.inf if max_distance is None else np.float64(max_distance) * np.float64(max_distance)
    return int(np.count_nonzero((last > rings) & (bound < d2) & (bound < md2)))
