"""GPU: ``proc3d.knn_points`` (``sc_knn``, csrc/nearest.hip) and ``knn_edges`` / ``knn_graph`` over it against the checker
(tests/knn_oracle.py): ``index`` and ``d2`` with ``np.array_equal``, no tolerance, from host arrays and from tensors.
Where a case is meant to exercise something, it first asserts by the CHECKER's account (or by ``far_out``, which the
library reports) that it does."""
import os

import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import proc3d
from tests import dbscan_oracle
from tests import knn_oracle as oracle
from tests import nearest_oracle
from tests.evaluation_oracle import source_constant


def run(queries, targets, k, device, max_distance=None, tensors=False):
    """One call: ``(index, d2, far)`` as NumPy arrays, the kinds and shapes of the outputs asserted."""
    if tensors:
        import torch
        tq = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 3)).cuda(device)
        tt = torch.from_numpy(np.ascontiguousarray(targets, dtype=np.float64).reshape(-1, 3)).cuda(device)
        index, d2, far = proc3d.knn_points(tq, tt, k, max_distance, return_far=True)
        assert index.is_cuda and index.dtype == torch.int32 and d2.is_cuda and d2.dtype == torch.float64
        index, d2 = index.cpu().numpy(), d2.cpu().numpy()
    else:
        index, d2, far = proc3d.knn_points(queries, targets, k, max_distance, device=device, return_far=True)
        assert isinstance(index, np.ndarray) and index.dtype == np.int32 and d2.dtype == np.float64
    assert index.shape == (len(queries), k) and d2.shape == (len(queries), k)
    return index, d2, far


def check(queries, targets, k, device, max_distance=None, want=None, forms=(False, True)):
    """Run the kernels from arrays and from tensors, compare with the checker (or ``want``); returns
    ``(want index, want d2, far_out)``."""
    if want is None:
        want = oracle.knn(queries, targets, k, max_distance)
    far = 0
    for tensors in forms:
        index, d2, far = run(queries, targets, k, device, max_distance, tensors)
        print(f"Q {len(queries)} P {len(targets)} k {k} max_distance {max_distance} tensors {tensors}: index differs at "
              f"{int(np.count_nonzero(index != want[0]))}, d2 at {int(np.count_nonzero(d2 != want[1]))}, far {far}")
        assert np.array_equal(index, want[0]) and np.array_equal(d2, want[1])
    return want[0], want[1], far


# ---- 1: sizes around the wavefront and the block, lists of one and of just over one lane-width --------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 64, 65])
def test_sizes(gpu_device, k):
    rng = np.random.default_rng(200 + k)
    padded = 0
    for Q in (1, 63, 64, 65, 257):
        for P in (1, 63, 64, 65, 257):
            q, t = rng.uniform(0.0, 4.0, size=(Q, 3)), rng.uniform(0.0, 4.0, size=(P, 3))
            index, d2, _ = check(q, t, k, gpu_device, want=oracle.knn_all_pairs(q, t, k))
            padded += int(P < k)
            assert np.all(index[:, :min(k, P)] >= 0) and np.all(index[:, min(k, P):] == -1) and np.all(np.isinf(d2[:, min(k, P):]))
    assert padded == {1: 0, 5: 5, 64: 10, 65: 15}[k]  # the (Q, P) pairs with fewer targets than places
    t = rng.uniform(0.0, 4.0, size=(65, 3))
    index, d2, _ = check(np.zeros((0, 3)), t, k, gpu_device, want=oracle.knn_all_pairs(np.zeros((0, 3)), t, k))
    assert index.shape == (0, k)
    index, d2, far = check(t, np.zeros((0, 3)), k, gpu_device, want=oracle.knn_all_pairs(t, np.zeros((0, 3)), k))
    assert np.all(index == -1) and np.all(np.isinf(d2)) and far == 0


# ---- 2: K6 ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_k_1_is_nearest_points(gpu_device):
    q = dbscan_oracle.blobs_cloud()
    t = nearest_oracle.blob_targets(q)
    for md in (None, 0.5):
        want = proc3d.nearest_points(q, t, md, device=gpu_device)
        checker = nearest_oracle.nearest(q, t, md)
        assert np.array_equal(want[0], checker[0]) and np.array_equal(want[1], checker[1])
        check(q, t, 1, gpu_device, md, want=(want[0][:, None], want[1][:, None]))


# ---- 3: ties ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "shifted", "negative"])
@pytest.mark.parametrize("k", [8, 5])
def test_lattice_ties(gpu_device, form, k):
    q, t = nearest_oracle.tie_clouds()
    plain = oracle.knn_all_pairs(q, t, 8)
    centres = plain[1][:80]  # the cell centres: eight lattice points at d2 = 0.75 each
    assert np.all(centres == 0.75) and np.all(np.diff(plain[0][:80], axis=1) > 0)  # equal d2: rising index
    if form == "shifted":  # leaves the lattice differences exact
        q, t = q + np.array([1e6, -1e6, 0.5]), t + np.array([1e6, -1e6, 0.5])
    elif form == "negative":
        q, t = -q, -t
    want = oracle.knn_all_pairs(q, t, k)
    assert np.array_equal(want[0], plain[0][:, :k]) and np.array_equal(want[1], plain[1][:, :k])  # k = 5 cuts the ties: the five smallest indices
    tree = oracle.knn(q, t, k)
    assert np.array_equal(tree[0], want[0]) and np.array_equal(tree[1], want[1])
    check(q, t, k, gpu_device, want=want)


# ---- 4: duplicates and degenerate clouds ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["copies", "line", "diagonal", "plane"])
def test_degenerate_targets(gpu_device, shape):
    rng = np.random.default_rng(34)
    s = rng.uniform(0.0, 10.0, size=400)
    if shape == "copies":
        t = np.tile([[1.25, -2.5, 0.75]], (300, 1))
    elif shape == "line":
        t = np.stack([s, np.full(400, 2.0), np.full(400, -1.0)], axis=1)
    elif shape == "diagonal":
        t = np.stack([s, s, s], axis=1)
    else:
        t = np.stack([s, rng.uniform(0.0, 10.0, size=400), np.full(400, 3.0)], axis=1)
    t = np.ascontiguousarray(t)
    lo, hi = t.min(axis=0), t.max(axis=0)
    q = np.ascontiguousarray(rng.uniform(lo - 3.0, hi + 3.0, size=(300, 3)))  # inside the box and around it
    index, d2, _ = check(q, t, 10, gpu_device, want=oracle.knn_all_pairs(q, t, 10))
    if shape == "copies":
        assert np.array_equal(index, np.tile(np.arange(10, dtype=np.int32), (300, 1)))  # 300-way ties: indices 0..9
    check(q, t, 10, gpu_device, max_distance=1.5, want=oracle.knn_all_pairs(q, t, 10, 1.5))
    check(t[:100], t, 10, gpu_device, want=oracle.knn_all_pairs(t[:100], t, 10))


@pytest.mark.gpu
def test_row_crosses_to_a_far_cluster(gpu_device):
    rng = np.random.default_rng(35)
    # 2040 targets: at k = 64 the grid is planned for 2040 / 8 of them, 7 cells per axis over the diagonal between the
    # clusters (with 240 targets it would have 4, and ring 3 would reach the far faces: nothing would go far).  The
    # near cluster lies in the corner cell, the other one six cells away: rings 0..3 hold 40 targets, fewer than k.
    near, other = rng.uniform(0.0, 1.0, size=(40, 3)), 1e4 + rng.uniform(0.0, 1.0, size=(2000, 3))
    t = np.ascontiguousarray(np.concatenate([near, other])[rng.permutation(2040)])
    q = np.ascontiguousarray(rng.uniform(0.0, 1.0, size=(70, 3)))
    want = oracle.knn_all_pairs(q, t, 64)
    assert np.all(want[1][:, 39] < 3.0) and np.all(want[1][:, 40] > 1e7)  # 40 near places, then the far cluster
    _, _, far = check(q, t, 64, gpu_device, want=want)
    assert far > 0  # four rings around a query do not hold 64 targets: the pass over all targets took them


# ---- 5: max_distance ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_max_distance_is_strict(gpu_device):
    below, above = np.nextafter(2.0, 0.0), np.nextafter(2.0, 3.0)
    t = np.array([[2.0, 0, 0], [0, below, 0], [0, 0, above], [0, 1.0, 0], [0, 0, -1.5], [-2.0, 0, 0], [9.0, 9, 9]])
    q = np.array([[0.0, 0, 0], [9.0, 9, 8], [50.0, 50, 50]])
    want = oracle.knn_all_pairs(q, t, 4, 2.0)
    assert want[0].tolist() == [[3, 4, 1, -1], [6, -1, -1, -1], [-1, -1, -1, -1]]  # exactly 2.0 and beyond: not counted
    assert want[1][0].tolist() == [1.0, 2.25, below * below, np.inf]
    check(q, t, 4, gpu_device, 2.0, want=want)
    free = oracle.knn_all_pairs(q, t, 4)
    assert free[0][0].tolist() == [3, 4, 1, 0] and free[1][0, 3] == 4.0  # unbounded: the target at exactly 2.0, the smaller index of two
    check(q, t, 4, gpu_device, want=free)
    lattice = np.argwhere(np.ones((6, 6, 6), dtype=bool)).astype(np.float64)  # spacing 1: six targets at exactly 2.0 of an inner point
    rng = np.random.default_rng(36)
    q = np.ascontiguousarray(np.concatenate([lattice[rng.integers(0, 216, size=60)], rng.uniform(0.0, 5.0, size=(60, 3))]))
    want = oracle.knn_all_pairs(q, lattice, 40, 2.0)
    used = (want[0] >= 0).sum(axis=1)
    assert 7 <= used.min() and used[:60].max() == 27 and used.max() < 40 and np.all(want[1][want[0] >= 0] < 4.0)  # partly filled rows
    assert np.array_equal(oracle.knn(q, lattice, 40, 2.0)[0], want[0])
    check(q, lattice, 40, gpu_device, 2.0, want=want)


# ---- 6: self-search -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_self_search(gpu_device):
    cloud = dbscan_oracle.blobs_cloud()[:1200].copy()
    cloud[700:760] = cloud[100:160]  # duplicates with larger indices
    index, d2, _ = check(cloud, cloud, 7, gpu_device)
    first = np.arange(1200)
    first[700:760] = np.arange(100, 160)
    assert np.array_equal(index[:, 0], first) and np.all(d2[:, 0] == 0.0)  # itself, or the smaller index of a duplicate
    assert np.array_equal(index[100:160, 1], np.arange(700, 760)) and np.all(d2[100:160, 1] == 0.0)


# ---- 7: the stem walk's shape, and the largest k ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_k_300_of_one_query_and_k_max(gpu_device):
    rng = np.random.default_rng(37)
    stem = np.ascontiguousarray(rng.normal(size=(5000, 3)) * np.array([2.0, 2.0, 40.0]))
    point = stem[1234]
    index, d2, _ = check(point[None], stem, 300, gpu_device, want=oracle.knn_all_pairs(point[None], stem, 300))
    assert index[0, 0] == 1234 and np.all(np.diff(d2[0]) >= 0.0) and len(set(index[0].tolist())) == 300
    assert nat.SC_KNN_MAX == 512
    q = np.ascontiguousarray(rng.uniform(-1.0, 11.0, size=(70, 3)))
    t = np.ascontiguousarray(rng.uniform(0.0, 10.0, size=(3000, 3)))
    check(q, t, nat.SC_KNN_MAX, gpu_device, want=oracle.knn_all_pairs(q, t, nat.SC_KNN_MAX))
    check(q, t[:700], nat.SC_KNN_MAX, gpu_device, 4.0, want=oracle.knn_all_pairs(q, t[:700], nat.SC_KNN_MAX, 4.0))
    with pytest.raises(ValueError, match="k must be"):
        proc3d.knn_points(q, t, nat.SC_KNN_MAX + 1, device=gpu_device)


# ---- 8: past the cap of the far pass (the rings launch is not capped) ----------------------------------------------------------
@pytest.mark.gpu
def test_far_list_longer_than_the_far_pass_has_wavefronts(gpu_device):
    waves = source_constant("nearest.hip", "kFarBlocks") * (source_constant("nearest.hip", "kB") // 64)
    rng = np.random.default_rng(38)
    t = rng.uniform(0.0, 1.0, size=(nearest_oracle.FAR_P, 3))
    extent = (t.max(axis=0) - t.min(axis=0)).max()
    q = t.mean(axis=0) + 1e3 * extent * np.array([1.0, -0.5, 0.25]) + rng.uniform(-1.0, 1.0, size=(nearest_oracle.FAR_Q, 3))
    near = np.arange(nearest_oracle.FAR_Q) % nearest_oracle.FAR_NEAR_EVERY == 0  # interleaved: the far list has gaps
    q[near] = rng.uniform(0.0, 1.0, size=(int(near.sum()), 3))
    q = np.ascontiguousarray(q)
    assert len(q) - int(near.sum()) > waves
    want = oracle.knn(q, t, 3)
    _, _, far = check(q, t, 3, gpu_device, want=want)
    print(f"far {far} of {len(q)}, wavefronts {waves}")
    assert far > waves


# ---- 9: streams, repeated runs, work buffers ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_streams_runs_and_work_buffers(gpu_device):
    import torch
    rng = np.random.default_rng(39)
    sq, st = rng.uniform(0.0, 5.0, size=(300, 3)), rng.uniform(0.0, 5.0, size=(200, 3))
    lq, lt = rng.uniform(0.0, 12.0, size=(4000, 3)), rng.uniform(0.0, 12.0, size=(6000, 3))
    ws, wl = oracle.knn(sq, st, 6, 0.9), oracle.knn(lq, lt, 20)
    assert (ws[0] == -1).any() and (ws[0][:, 0] >= 0).any()
    nat.backend().call("sc_nearest_release")  # whatever earlier tests left: the first call allocates
    tsq, tst, tlq, tlt = (torch.from_numpy(a).cuda(gpu_device) for a in (sq, st, lq, lt))
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))  # the uploads
    r1 = proc3d.knn_points(tsq, tst, 6, 0.9)
    with torch.cuda.stream(side):
        r2 = proc3d.knn_points(tlq, tlt, 20)  # a second stream; grows the buffers behind the first call
    r3 = proc3d.knn_points(tsq, tst, 6, 0.9)
    n1 = proc3d.nearest_points(tsq, tst, 0.9)  # the other entry of the same slot
    side.synchronize()
    torch.cuda.current_stream(gpu_device).synchronize()
    for got, want in ((r1, ws), (r2, wl), (r3, ws)):
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    assert np.array_equal(n1[0].cpu().numpy(), ws[0][:, 0]) and np.array_equal(n1[1].cpu().numpy(), ws[1][:, 0])
    runs = [proc3d.knn_points(lq, lt, 20, device=gpu_device) for _ in range(3)]  # the same bits on three runs
    assert all(np.array_equal(r[0], wl[0]) and r[1].tobytes() == runs[0][1].tobytes() for r in runs) and np.array_equal(runs[0][1], wl[1])
    proc3d.release_device_buffers()  # sc_nearest_release gives sc_knn's buffers back
    check(sq, st, 6, gpu_device, 0.9, want=ws)
    check(lq, lt, 20, gpu_device, want=wl)


# ---- 10: refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(gpu_device):
    import torch
    rng = np.random.default_rng(40)
    q, t = rng.uniform(0.0, 5.0, size=(3000, 3)), rng.uniform(0.0, 5.0, size=(2500, 3))
    want = oracle.knn(q, t, 4)
    for bad in (np.nan, np.inf):  # host arrays: refused before any device call, naming the point
        broken = q.copy()
        broken[17, 1] = bad
        with pytest.raises(ValueError, match="non-finite coordinate in query 17"):
            proc3d.knn_points(broken, t, 4, device=gpu_device)
        broken = t.copy()
        broken[-1, 2] = bad
        with pytest.raises(ValueError, match="non-finite coordinate in target 2499"):
            proc3d.knn_points(q, broken, 4, device=gpu_device)
    tq, tt = torch.from_numpy(q).cuda(gpu_device), torch.from_numpy(t).cuda(gpu_device)
    for bad in (float("nan"), float("-inf")):  # device tensors: the last element, the first kernels are the judge
        broken = tq.clone()
        broken[-1, 2] = bad
        with pytest.raises(ValueError, match="non-finite coordinate in the device queries"):
            proc3d.knn_points(broken, tt, 4)
        broken = tt.clone()
        broken[-1, 2] = bad
        with pytest.raises(ValueError, match="non-finite coordinate in the device targets"):
            proc3d.knn_points(tq, broken, 4)
        index, d2 = proc3d.knn_points(tq, tt, 4)  # the call after a refused one is a whole one
        assert np.array_equal(index.cpu().numpy(), want[0]) and np.array_equal(d2.cpu().numpy(), want[1])
    with pytest.raises(ValueError, match="float64 CUDA tensor"):
        proc3d.knn_points(tq.float(), tt, 4)
    with pytest.raises(ValueError, match="max_distance"):
        proc3d.knn_points(tq, tt, 4, 1e-200)


# ---- 11: the virtual plant ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_virtual_plant_mesh_vertices(gpu_device):
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    verts = np.ascontiguousarray(np.load(os.path.join(gold, "virtual_plant_mesh.npz"))["vertices"].astype(np.float64))
    assert verts.shape == (31411, 3)
    index, d2, far = check(verts, verts, 16, gpu_device)
    assert np.all(d2[:, 0] == 0.0) and np.all(index >= 0)
    print(f"virtual plant: 31 411 vertices, k = 16: {far} queries went to the pass over all targets")


# ---- 12: the graph -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_knn_edges_and_graph(gpu_device):
    import networkx as nx
    rng = np.random.default_rng(41)
    pts = rng.uniform(0.0, 6.0, size=(500, 3))
    pts[400:430] = pts[10:40]  # duplicates
    pts = np.ascontiguousarray(pts)
    nodes, want = oracle.reference_knn_graph(pts, 6)
    assert all((i, i) in want and want[(i, i)] == 0.0 for i in range(500)) and len(want) > 500 * 3
    _, d2 = oracle.knn_all_pairs(pts, pts, 6)
    edges, weights = proc3d.knn_edges(pts, 6, device=gpu_device)
    assert edges.dtype == np.int32 and edges.shape == (len(want), 2) and weights.dtype == np.float64 and weights.shape == (len(want),)
    assert [tuple(e) for e in edges.tolist()] == sorted(want)  # deduplicated, lexicographic
    assert set(weights.tolist()) <= set(np.sqrt(d2).reshape(-1).tolist())  # sqrt of a d2 of the search, bit for bit
    ref = np.array([want[tuple(e)] for e in edges.tolist()])
    # the reference's weight is np.linalg.norm of the difference: the same three squares added in whatever order and
    # rounding the dot product takes, then one square root.  Either sum is within 3 u of the exact one (u = 2^-53), so
    # the two are within 6 u of each other, their roots within 3 u, and a rounding each: 5 u.  The test takes 8 u.
    assert np.all(np.abs(weights - ref) <= 2.0 ** -50 * ref)
    g = proc3d.knn_graph(proc3d.PointCloud(pts, None), 6, device=gpu_device)
    assert isinstance(g, nx.Graph) and not g.is_directed()
    assert sorted(g.nodes) == sorted(nodes) and all(np.array_equal(g.nodes[i]["center"], nodes[i]) for i in nodes)
    assert sorted((min(a, b), max(a, b)) for a, b in g.edges) == sorted(want)
    assert [g.edges[tuple(e)]["weight"] for e in edges.tolist()] == weights.tolist()
