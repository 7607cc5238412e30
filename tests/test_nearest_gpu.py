"""GPU: ``proc3d.nearest_points`` (``sc_nearest``, csrc/nearest.hip) and the cloud metrics over it against the checker
(tests/nearest_oracle.py): ``index`` and ``d2`` with ``np.array_equal``, no tolerance; the three sums within N6's
derived bound ``(Q + 8) 2^-52`` of ``math.fsum``; the confusion counts and everything derived from them exactly.
Where a case is meant to exercise something, it first asserts by the CHECKER's account that it does."""
import math
import os

import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import metrics, proc3d
from plant3dvision_amd.tasks.evaluation import point_cloud_evaluation_run, segmented_point_cloud_evaluation_run
from tests import dbscan_oracle
from tests import nearest_oracle as oracle

LDS_MAX_LABELS = 32  # L * L <= 1024 is counted in LDS tables (include/spacecarve.h)


def check(queries, targets, device, max_distance=None, tensors=False, want=None):
    """Run the kernels, compare with the checker (or ``want``), return the checker's ``(index, d2)``."""
    if want is None:
        want = oracle.nearest(queries, targets, max_distance)[:2]
    if tensors:
        import torch
        tq = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 3)).cuda(device)
        tt = torch.from_numpy(np.ascontiguousarray(targets, dtype=np.float64).reshape(-1, 3)).cuda(device)
        index, d2 = proc3d.nearest_points(tq, tt, max_distance)
        assert index.is_cuda and index.dtype == torch.int32 and d2.is_cuda and d2.dtype == torch.float64
        index, d2 = index.cpu().numpy(), d2.cpu().numpy()
    else:
        index, d2 = proc3d.nearest_points(queries, targets, max_distance, device=device)
        assert isinstance(index, np.ndarray) and index.dtype == np.int32 and d2.dtype == np.float64
    assert index.shape == (len(queries),) and d2.shape == (len(queries),)
    print(f"Q {len(queries)} P {len(targets)} max_distance {max_distance} tensors {tensors}: index differs at "
          f"{int(np.count_nonzero(index != want[0]))}, d2 at {int(np.count_nonzero(d2 != want[1]))}")
    assert np.array_equal(index, want[0]) and np.array_equal(d2, want[1])
    return want


@pytest.fixture(scope="module")
def blobs():
    """Case 1's clouds with the checker's answers in both directions, computed once."""
    q = dbscan_oracle.blobs_cloud()
    t = oracle.blob_targets(q)
    return dict(q=q, t=t, qt=oracle.nearest(q, t), tq=oracle.nearest(t, q))


# ---- 1: blobs, both directions, permuted again ------------------------------------------------------------------------
@pytest.mark.gpu
def test_blobs_both_directions_and_permuted(gpu_device, blobs):
    q, t = blobs["q"], blobs["t"]
    assert q.shape == (1900, 3) and t.shape == (2500, 3)
    assert len(np.unique(blobs["qt"][0])) > 1000 and blobs["qt"][1].max() > 4.0 > 0.25 > blobs["qt"][1].min()
    check(q, t, gpu_device, want=blobs["qt"])
    check(t, q, gpu_device, want=blobs["tq"])
    perm = np.random.default_rng(5).permutation(len(t))
    check(q, np.ascontiguousarray(t[perm]), gpu_device)  # its own checker run, not permuted indices
    check(np.ascontiguousarray(t[perm]), q, gpu_device)


# ---- 2: ties -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "shifted", "negative"])
def test_lattice_ties(gpu_device, form):
    q, t = oracle.tie_clouds()
    index, d2, ties = oracle.nearest(q, t, return_ties=True)
    assert ties >= 150 and (d2 == 0.0).sum() >= 50 and (d2 == 0.75).sum() == 80 and (d2 == 0.25).sum() == 70
    dup = index[150:154]  # the four lattice points that have copies at the end: the smaller index wins
    assert np.all(dup < 216)
    if form == "shifted":  # leaves the lattice differences exact
        q, t = q + np.array([1e6, -1e6, 0.5]), t + np.array([1e6, -1e6, 0.5])
    elif form == "negative":
        q, t = -q, -t
    got = oracle.nearest(q, t, return_ties=True)
    assert got[2] == ties and np.array_equal(got[0], index) and np.array_equal(got[1], d2)
    check(q, t, gpu_device, want=got[:2])
    check(q, t, gpu_device, tensors=True, want=got[:2])


# ---- 3: sizes around the wavefront and the block ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tensors", [False, True])
def test_sizes(gpu_device, tensors):
    rng = np.random.default_rng(100)
    for Q in (1, 63, 64, 65, 257):
        for P in (1, 63, 64, 65, 257):
            q, t = rng.uniform(0.0, 4.0, size=(Q, 3)), rng.uniform(0.0, 4.0, size=(P, 3))
            check(q, t, gpu_device, tensors=tensors, want=oracle.nearest_all_pairs(q, t))
    t = rng.uniform(0.0, 4.0, size=(65, 3))
    index, d2 = check(np.zeros((0, 3)), t, gpu_device, tensors=tensors)
    assert index.shape == (0,)
    index, d2 = check(t, np.zeros((0, 3)), gpu_device, tensors=tensors)
    assert index.tolist() == [-1] * 65 and np.all(np.isinf(d2))


# ---- 4: degenerate targets ---------------------------------------------------------------------------------------------------
def _around(targets, rng, n=300):
    """Queries inside the targets' box and outside it on each side."""
    lo, hi = targets.min(axis=0), targets.max(axis=0)
    ext = np.maximum(hi - lo, 1.0)
    inside = rng.uniform(lo, np.maximum(hi, lo + 1e-9), size=(n, 3))
    outside = [inside[: n // 6].copy() for _ in range(6)]
    for k in range(6):
        a = k // 2
        outside[k][:, a] = (lo[a] - rng.uniform(0.1, 3.0, size=n // 6) * ext[a]) if k % 2 == 0 else (hi[a] + rng.uniform(0.1, 3.0, size=n // 6) * ext[a])
    return np.ascontiguousarray(np.concatenate([inside] + outside))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["copies", "line", "diagonal", "plane", "two_clusters"])
def test_degenerate_targets(gpu_device, shape):
    rng = np.random.default_rng(33)
    s = rng.uniform(0.0, 10.0, size=400)
    if shape == "copies":
        t = np.tile([[1.25, -2.5, 0.75]], (300, 1))
    elif shape == "line":
        t = np.stack([s, np.full(400, 2.0), np.full(400, -1.0)], axis=1)
    elif shape == "diagonal":
        t = np.stack([s, s, s], axis=1)
    elif shape == "plane":
        t = np.stack([s, rng.uniform(0.0, 10.0, size=400), np.full(400, 3.0)], axis=1)
    else:
        t = np.concatenate([rng.uniform(0.0, 1.0, size=(200, 3)), 1e4 + rng.uniform(0.0, 1.0, size=(200, 3))])
    t = np.ascontiguousarray(t)
    q = _around(t, rng)
    if shape == "two_clusters":
        q = np.concatenate([q, 5000.5 + rng.uniform(-1.0, 1.0, size=(100, 3))])  # midway between the clusters
    index, d2 = check(q, t, gpu_device)
    if shape == "copies":
        assert np.all(index == 0)  # 300-way ties: the smallest index
    if shape == "two_clusters":
        assert (index[-100:] < 200).any() and (index[-100:] >= 200).any()
    check(q, t, gpu_device, max_distance=1.5)


# ---- 5: far and collapsed ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_far_queries_and_collapsed_grid(gpu_device, blobs):
    rng = np.random.default_rng(8)
    t = np.ascontiguousarray(blobs["t"][:600])
    extent = (t.max(axis=0) - t.min(axis=0)).max()
    far = t.mean(axis=0) + 1e3 * extent * np.array([1.0, -0.5, 0.25]) + rng.uniform(-1.0, 1.0, size=(500, 3))
    index, d2 = check(far, t, gpu_device)  # every query 10^3 extents away: the far-query path
    assert d2.min() > (900.0 * extent) ** 2
    check(far, t, gpu_device, tensors=True, want=(index, d2))
    index, d2 = check(far, t, gpu_device, max_distance=2.0)
    assert np.all(index == -1)
    # one target at 1e12 collapses the grid to a busy cell: exact still
    outlier = np.ascontiguousarray(np.roll(np.concatenate([t, [[1e12, -1e12, 1e12]]]), 7, axis=0))
    q = np.ascontiguousarray(np.concatenate([blobs["q"][:500], [[9e11, -9e11, 9e11]]]))
    index, d2 = check(q, outlier, gpu_device)
    assert index[-1] == 6 and (index[:-1] != 6).all()
    check(q, outlier, gpu_device, max_distance=0.5)


# ---- 6: max_distance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_max_distance_is_strict(gpu_device):
    lattice = np.argwhere(np.ones((5, 5, 5), dtype=bool)).astype(np.float64) * 5.0  # spacing 5: a query 2.0 from one point is 3.0 from the next
    rng = np.random.default_rng(12)
    q = lattice[rng.integers(0, len(lattice), size=90)]
    axis = rng.integers(0, 3, size=90)
    step = np.concatenate([np.full(30, 2.0), np.full(30, np.nextafter(2.0, 0.0)), np.full(30, np.nextafter(2.0, 3.0))])
    q[np.arange(90), axis] = step  # from the lattice point with 0 on that axis: the difference is the step itself, exactly
    free_i, free_d2 = oracle.nearest(q, lattice)
    index, d2 = oracle.nearest(q, lattice, 2.0)
    exactly, inside, outside = free_d2 == 4.0, free_d2 < 4.0, free_d2 > 4.0
    assert exactly.sum() >= 10 and inside.sum() >= 10 and outside.sum() >= 10
    assert np.all(index[exactly] == -1) and np.all(np.isinf(d2[exactly])) and np.all(index[outside] == -1)
    assert np.array_equal(index[inside], free_i[inside]) and np.array_equal(d2[inside], free_d2[inside])
    check(q, lattice, gpu_device, want=(free_i, free_d2))
    check(q, lattice, gpu_device, max_distance=2.0, want=(index, d2))
    check(q, lattice, gpu_device, max_distance=2.0, tensors=True, want=(index, d2))


# ---- 7: sums and metrics ---------------------------------------------------------------------------------------------------------
def _close(got, want, Q):
    print(f"sum {got!r} against fsum {want!r}: relative {abs(got - want) / want if want else 0.0:.3e}, bound {oracle.sums_tolerance(Q):.3e}")
    return abs(got - want) <= oracle.sums_tolerance(Q) * want


@pytest.mark.gpu
def test_sums_and_metrics(gpu_device, blobs):
    import torch
    q, t = blobs["q"], blobs["t"]
    tq_, tt_ = torch.from_numpy(q).cuda(gpu_device), torch.from_numpy(t).cuda(gpu_device)
    for md in (None, 0.5, 2):
        d2 = oracle._bound(*blobs["qt"][:2], md)[1]
        n, s2, s1 = oracle.sums(d2)
        assert 0 < n and (md is None or n < len(q))  # matched and unmatched queries both exist
        runs = [proc3d.nearest_sums(q, t, md, device=gpu_device) for _ in range(3)] + [proc3d.nearest_sums(tq_, tt_, md)]
        assert runs[0][0] == n and _close(runs[0][1], s2, len(q)) and _close(runs[0][2], s1, len(q))
        assert all(r == runs[0] for r in runs[1:])  # the same bits, from host arrays and from tensors
    want = oracle.sums(blobs["qt"][1])[2] / len(q) + oracle.sums(blobs["tq"][1])[2] / len(t)
    got = [metrics.chamfer_distance(q, t, device=gpu_device) for _ in range(3)]
    print("chamfer", got[0], want)
    # each mean is within its sum's bound plus a division, their sum within the larger of the two plus an addition
    assert abs(got[0] - want) <= 2 * oracle.sums_tolerance(len(t)) * want and got[0] == got[1] == got[2]
    assert metrics.chamfer_distance(proc3d.PointCloud(q, None), proc3d.PointCloud(t, None), device=gpu_device) == got[0]
    for md in (0.5, 2):
        d2 = oracle._bound(*blobs["qt"][:2], md)[1]
        n, s2, _ = oracle.sums(d2)
        fit, rmse = metrics.point_cloud_registration_fitness(q, t, md, device=gpu_device)
        print("fitness", md, fit, rmse)
        assert fit == n / len(q) and abs(rmse - math.sqrt(s2 / n)) <= oracle.sums_tolerance(len(q)) * rmse
        assert metrics.point_cloud_registration_fitness(tq_, tt_, md) == (fit, rmse)
    assert metrics.point_cloud_registration_fitness(q + 100.0, t, 0.5, device=gpu_device) == (0.0, 0.0)  # nothing matched


# ---- 8: labels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_compare_segmented_point_clouds(gpu_device, blobs):
    import torch
    gt, pred = blobs["q"], blobs["t"]
    gt_labels = ["leaf"] * 700 + ["stem"] * 700 + ["fruit"] * 500  # by blob: 350 each, then the noise
    near = blobs["tq"][0]  # each predicted point takes the name of its nearest ground-truth point, except:
    pred_labels = [gt_labels[k] for k in near]
    pred_labels = ["flower" if name == "fruit" else name for name in pred_labels]  # fruit: no predicted point; flower: only predicted
    pred_labels = [("stem" if k % 7 == 0 and name == "leaf" else name) for k, name in enumerate(pred_labels)]  # some errors
    want = oracle.compare_segmented(gt, gt_labels, pred, pred_labels)
    assert "flower" in pred_labels and "fruit" not in pred_labels and 0 < want["miou"]["leaf"] < 1.0 and want["miou"]["fruit"] == 0.0
    got = metrics.CompareSegmentedPointClouds(proc3d.PointCloud(gt, None), gt_labels, proc3d.PointCloud(pred, None), pred_labels,
                                              device=gpu_device)
    assert got.results == want
    assert segmented_point_cloud_evaluation_run(pred, pred_labels, gt, gt_labels) == want
    # points as tensors: the indices never leave the device
    tg, tp = torch.from_numpy(gt).cuda(gpu_device), torch.from_numpy(pred).cuda(gpu_device)
    assert metrics.CompareSegmentedPointClouds(tg, gt_labels, tp, pred_labels).results == want
    # L = 1
    one = metrics.CompareSegmentedPointClouds(gt, ["a"] * len(gt), pred, ["a"] * len(pred), device=gpu_device).results
    assert one == oracle.compare_segmented(gt, ["a"] * len(gt), pred, ["a"] * len(pred)) and one["miou"] == {"a": 1.0}
    # the largest table the LDS path takes, and the first the global path takes
    rng = np.random.default_rng(4)
    index = blobs["qt"][0]
    for L in (LDS_MAX_LABELS, LDS_MAX_LABELS + 1):
        ql, tl = rng.integers(0, L, size=len(gt)).astype(np.int32), rng.integers(0, L, size=len(pred)).astype(np.int32)
        ql[:2], tl[index[:2]] = L - 1, L - 1  # the last cell is used
        table = np.zeros((L, L), dtype=np.int64)
        np.add.at(table, (ql, tl[index]), 1)
        assert table[L - 1, L - 1] >= 2 and table.sum() == len(gt)
        assert np.array_equal(proc3d.nearest_confusion(index, ql, tl, L, device=gpu_device), table)
        dev = [torch.from_numpy(a).cuda(gpu_device) for a in (index, ql, tl)]
        assert np.array_equal(proc3d.nearest_confusion(*dev, L), table)
        unmatched = index.copy()
        unmatched[::3] = -1  # not counted
        table = np.zeros((L, L), dtype=np.int64)
        np.add.at(table, (ql[unmatched >= 0], tl[unmatched[unmatched >= 0]]), 1)
        assert np.array_equal(proc3d.nearest_confusion(unmatched, ql, tl, L, device=gpu_device), table)


# ---- 9: streams and buffers ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_streams_and_work_buffers(gpu_device, blobs):
    """A small call, a larger one on a side stream that has to replace the work buffers, the small one again, a
    refused call, the release, and the small one in buffers allocated anew: each the checker's answer."""
    import torch
    rng = np.random.default_rng(41)
    sq, st = rng.uniform(0.0, 5.0, size=(300, 3)), rng.uniform(0.0, 5.0, size=(200, 3))
    lq, lt = rng.uniform(0.0, 12.0, size=(7000, 3)), rng.uniform(0.0, 12.0, size=(6000, 3))
    ws, wl = oracle.nearest(sq, st, 0.5), oracle.nearest(lq, lt, 0.5)
    assert (ws[0] == -1).any() and (ws[0] >= 0).any() and (wl[0] == -1).any() and (wl[0] >= 0).any()
    nat.backend().call("sc_nearest_release")  # whatever earlier tests left: the first call allocates
    tsq, tst, tlq, tlt = (torch.from_numpy(a).cuda(gpu_device) for a in (sq, st, lq, lt))
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))  # the uploads
    r1 = proc3d.nearest_points(tsq, tst, 0.5)
    with torch.cuda.stream(side):
        r2 = proc3d.nearest_points(tlq, tlt, 0.5)  # grows: waits for the first call before it frees its buffers
    r3 = proc3d.nearest_points(tsq, tst, 0.5)
    with pytest.raises(ValueError, match="max_distance"):
        proc3d.nearest_points(tsq, tst, 1e-200)
    with pytest.raises(ValueError, match="float64 CUDA tensor"):
        proc3d.nearest_points(tsq.float(), tst)
    r4 = proc3d.nearest_points(tsq, tst, 0.5)
    side.synchronize()
    torch.cuda.current_stream(gpu_device).synchronize()
    for got, want in ((r1, ws), (r2, wl), (r3, ws), (r4, ws)):
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    nat.backend().call("sc_nearest_release")
    r5 = proc3d.nearest_points(tsq, tst, 0.5)
    assert np.array_equal(r5[0].cpu().numpy(), ws[0]) and np.array_equal(r5[1].cpu().numpy(), ws[1])
    check(sq, st, gpu_device, max_distance=0.5, want=ws[:2])  # the host route
    proc3d.release_device_buffers()  # calls sc_nearest_release too
    check(sq, st, gpu_device, max_distance=0.5, want=ws[:2])


# ---- 10: what only the device can find ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_on_the_device(gpu_device, blobs):
    import torch
    q, t = blobs["q"], blobs["t"]
    tq, tt = torch.from_numpy(q).cuda(gpu_device), torch.from_numpy(t).cuda(gpu_device)

    def whole():  # the call after a refused one is a whole one
        index, d2 = proc3d.nearest_points(tq, tt)
        assert np.array_equal(index.cpu().numpy(), blobs["qt"][0]) and np.array_equal(d2.cpu().numpy(), blobs["qt"][1])

    for bad in (float("nan"), float("inf")):
        broken = tq.clone()
        broken[1234, 1] = bad
        with pytest.raises(ValueError, match="non-finite coordinate in the device queries"):
            proc3d.nearest_points(broken, tt)
        whole()
        broken = tt.clone()
        broken[2345, 2] = bad
        with pytest.raises(ValueError, match="non-finite coordinate in the device targets"):
            proc3d.nearest_points(tq, broken)
        whole()
    index = torch.from_numpy(blobs["qt"][0]).cuda(gpu_device)
    ql, tl = torch.zeros(len(q), dtype=torch.int32, device=index.device), torch.ones(len(t), dtype=torch.int32, device=index.device)
    want = np.array([[0, len(q)], [0, 0]])
    assert np.array_equal(proc3d.nearest_confusion(index, ql, tl, 2), want)
    for which, at, value in ((ql, 77, 2), (ql, 77, -1), (tl, 2499, 2), (index, 5, len(t)), (index, 5, -2)):
        keep = int(which[at])
        which[at] = value
        with pytest.raises(ValueError, match="outside"):
            proc3d.nearest_confusion(index, ql, tl, 2)
        which[at] = keep
        assert np.array_equal(proc3d.nearest_confusion(index, ql, tl, 2), want)
    whole()


# ---- 11: the virtual plant ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_virtual_plant_cloud_against_its_mesh(gpu_device):
    """The hull carved from the reference's own pictures (tests/test_virtual_plant_mesh.py's fixtures, voxel size
    0.25), its ``vol2pcd`` cloud searched against the mesh's 31 411 vertices, both ways."""
    from plant3dvision_amd.cl import Backprojection
    from plant3dvision_amd.tasks.cl import grid_from_bounding_box
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    d, mesh = np.load(os.path.join(gold, "virtual_plant_inputs.npz")), np.load(os.path.join(gold, "virtual_plant_mesh.npz"))
    verts = np.ascontiguousarray(mesh["vertices"].astype(np.float64))
    assert verts.shape == (31411, 3)
    bbox = {"x": list(d["bbox"][0]), "y": list(d["bbox"][1]), "z": list(d["bbox"][2])}
    shape, origin = grid_from_bounding_box(bbox, 0.25)
    bp = Backprojection(list(shape), origin, 0.25, device=gpu_device)
    for q in range(d["masks_background"].shape[0]):
        bp._submit_view(d["K_background"][q].astype(np.float32), d["R_background"][q].reshape(9).astype(np.float32),
                        d["t_background"][q].astype(np.float32), d["masks_background"][q], invert=True)
    pcd = proc3d.vol2pcd(bp, np.array(origin), 0.25, 1.0, device=gpu_device, as_open3d=False)
    bp.close()
    cloud = np.ascontiguousarray(np.asarray(pcd.points, dtype=np.float64))
    assert 2000 < len(cloud) < 100000
    a = check(cloud, verts, gpu_device)
    b = check(verts, cloud, gpu_device)
    check(cloud, verts, gpu_device, max_distance=0.5, tensors=True, want=oracle._bound(a[0], a[1], 0.5))
    height = float(np.median(verts[:, 2]))
    labels = ["low" if z < height else "high" for z in cloud[:, 2]]
    labels_gt = ["low" if z < height else "high" for z in verts[:, 2]]
    got = point_cloud_evaluation_run(pcd, verts, labels, labels_gt, max_distance=0.5, task_id="PointCloud")
    want = point_cloud_evaluation_run(cloud, verts, labels, labels_gt, max_distance=0.5, task_id="PointCloud",
                                      registration_fn=oracle.registration_fitness)
    assert set(got) == {"id", "all", "low", "high"}
    for key in ("all", "low", "high"):
        n = len(cloud) if key == "all" else labels.count(key)
        assert got[key]["fitness"] == want[key]["fitness"] and 0.0 < got[key]["fitness"] <= 1.0
        assert abs(got[key]["inlier_rmse"] - want[key]["inlier_rmse"]) <= oracle.sums_tolerance(n) * want[key]["inlier_rmse"]
    chamfer = metrics.chamfer_distance(pcd, verts, device=gpu_device)
    want_chamfer = oracle.sums(a[1])[2] / len(cloud) + oracle.sums(b[1])[2] / len(verts)
    assert abs(chamfer - want_chamfer) <= 2 * oracle.sums_tolerance(len(verts)) * want_chamfer
    print(f"virtual plant: {len(cloud)} points against {len(verts)} vertices: fitness {got['all']['fitness']:.6f}, "
          f"inlier_rmse {got['all']['inlier_rmse']:.6f} at max_distance 0.5, chamfer distance {chamfer:.6f}")


# ---- 12: past the capped grids ---------------------------------------------------------------------------------------
# Every launch of nearest.hip but the one-thread-per-point ones has a capped grid and a grid-stride loop; the clouds
# above are all small enough for one trip.  tests/test_unit_plans_host.py pins the caps' replica and these sizes; each
# case below first shows from its INPUTS and the checker that it goes past its cap.
@pytest.mark.gpu
def test_far_list_longer_than_the_far_pass_has_wavefronts(gpu_device):
    rng = np.random.default_rng(108)
    t = rng.uniform(0.0, 1.0, size=(oracle.FAR_P, 3))
    extent = (t.max(axis=0) - t.min(axis=0)).max()
    q = t.mean(axis=0) + 1e3 * extent * np.array([1.0, -0.5, 0.25]) + rng.uniform(-1.0, 1.0, size=(oracle.FAR_Q, 3))
    near = np.arange(oracle.FAR_Q) % oracle.FAR_NEAR_EVERY == 0  # interleaved: the far list has gaps
    q[near] = rng.uniform(0.0, 1.0, size=(int(near.sum()), 3))
    q = np.ascontiguousarray(q)
    assert near.sum() == 300
    index, d2 = oracle.nearest(q, t)
    far = oracle.certainly_far(q, t, d2)
    print(f"certainly far {far} of {len(q)}, wavefronts {oracle.far_waves(len(q))}")
    assert far > oracle.far_waves(len(q)) and oracle.certainly_far(q[near], t, d2[near]) == 0
    assert d2[~near].min() > (900.0 * extent) ** 2 and d2[near].max() < 1.0
    check(q, t, gpu_device, want=(index, d2))
    check(q, t, gpu_device, tensors=True, want=(index, d2))


@pytest.mark.gpu
def test_sums_past_the_partial_blocks(gpu_device):
    import torch
    rng = np.random.default_rng(109)
    q, t = rng.uniform(0.0, 4.0, size=(oracle.SUMS_Q, 3)), rng.uniform(0.0, 4.0, size=(oracle.SUMS_P, 3))
    Q = len(q)
    assert Q > oracle.sums_stride(Q)  # the last queries are added on a second trip
    free = oracle.nearest_in_pieces(q, t)
    tq_, tt_ = torch.from_numpy(q).cuda(gpu_device), torch.from_numpy(t).cuda(gpu_device)
    for md in (None, 0.5):
        d2 = oracle._bound(*free, md)[1]
        n, s2, s1 = oracle.sums(d2)
        late = int(np.isfinite(d2[oracle.sums_stride(Q):]).sum())
        print(f"max_distance {md}: matched {n} of {Q}, {late} of them past the first trip")
        assert late > 0 and (n == Q if md is None else 0 < n < Q)  # matched and unmatched queries both exist
        runs = [proc3d.nearest_sums(q, t, md, device=gpu_device) for _ in range(3)] + [proc3d.nearest_sums(tq_, tt_, md)]
        assert runs[0][0] == n and _close(runs[0][1], s2, Q) and _close(runs[0][2], s1, Q)
        assert all(r == runs[0] for r in runs[1:])  # the same bits, from host arrays and from tensors
        check(q, t, gpu_device, max_distance=md, tensors=True, want=oracle._bound(*free, md))


@pytest.fixture(scope="module")
def late_targets():
    """65 836 targets whose box only the last 300 span: its eight corners lie among the indices >= 65 536, the others
    well inside.  3000 queries inside and around the box, with the checker's answer."""
    rng = np.random.default_rng(110)
    P = oracle.LATE_P
    first_late = oracle.box_stride(P)
    assert 0 < first_late < P - 8
    t = rng.uniform(1.0, 9.0, size=(P, 3))
    corners = np.array([[x, y, z] for x in (0.0, 10.0) for y in (0.0, 10.0) for z in (0.0, 10.0)])
    t[first_late + 3 + 37 * np.arange(8)] = corners
    t = np.ascontiguousarray(t)
    assert t[:first_late].min() >= 1.0 and t[:first_late].max() <= 9.0 and t.min() == 0.0 and t.max() == 10.0
    q = _around(t, rng, n=1500)
    assert q.shape == (3000, 3)
    return dict(q=q, t=t, qt=oracle.nearest(q, t))


@pytest.mark.gpu
def test_targets_past_the_partial_blocks(gpu_device, late_targets):
    q, t, want = late_targets["q"], late_targets["t"], late_targets["qt"]
    first_late = oracle.box_stride(len(t))
    assert (want[0] >= first_late).any() and (want[0] < first_late).any()  # late targets are answers too
    check(q, t, gpu_device, want=want)
    check(q, t, gpu_device, tensors=True, want=want)
    bounded = oracle._bound(*want, 0.75)
    assert (bounded[0] == -1).any() and (bounded[0] >= 0).any()
    check(q, t, gpu_device, max_distance=0.75, want=bounded)
    check(q, t, gpu_device, max_distance=0.75, tensors=True, want=bounded)


@pytest.mark.gpu
def test_refusals_on_the_device_in_a_late_trip(gpu_device, late_targets):
    """The judges of device points are grid-stride loops under a cap: a bad value in the LAST point is found by a late
    trip only (the box launch's second, the fourth of the judge of the queries)."""
    import torch
    q, t, want = late_targets["q"], late_targets["t"], late_targets["qt"]
    tq, tt = torch.from_numpy(q).cuda(gpu_device), torch.from_numpy(t).cuda(gpu_device)
    assert len(t) - 1 >= oracle.box_stride(len(t))
    for bad in (float("nan"), float("inf")):
        broken = tt.clone()
        broken[-1, 2] = bad
        with pytest.raises(ValueError, match="non-finite coordinate in the device targets"):
            proc3d.nearest_points(tq, broken)
        index, d2 = proc3d.nearest_points(tq, tt)  # the call after a refused one is a whole one
        assert np.array_equal(index.cpu().numpy(), want[0]) and np.array_equal(d2.cpu().numpy(), want[1])
    rng = np.random.default_rng(111)
    lq, st = rng.uniform(0.0, 4.0, size=(oracle.LATE_Q, 3)), rng.uniform(0.0, 4.0, size=(64, 3))
    assert (3 * len(lq) - 1) // oracle.finite_stride(len(lq)) == 3
    lwant = oracle.nearest_in_pieces(lq, st)
    tlq, tst = torch.from_numpy(lq).cuda(gpu_device), torch.from_numpy(st).cuda(gpu_device)
    for bad in (float("nan"), float("-inf")):
        broken = tlq.clone()
        broken[-1, 2] = bad
        with pytest.raises(ValueError, match="non-finite coordinate in the device queries"):
            proc3d.nearest_points(broken, tst)
        index, d2 = proc3d.nearest_points(tlq, tst)
        assert np.array_equal(index.cpu().numpy(), lwant[0]) and np.array_equal(d2.cpu().numpy(), lwant[1])


@pytest.mark.gpu
@pytest.mark.parametrize("L", [LDS_MAX_LABELS, LDS_MAX_LABELS + 1])
def test_confusion_past_the_label_blocks(gpu_device, L):
    import torch
    rng = np.random.default_rng(112 + L)
    Q, P = oracle.CONFUSION_Q, oracle.CONFUSION_P
    first_late = oracle.labels_stride(Q, P)
    assert 0 < first_late < Q - 5 and (L * L <= oracle.launch_caps()["kLdsTable"]) == (L == LDS_MAX_LABELS)  # the LDS table, the global one
    index = rng.integers(0, P, size=Q).astype(np.int32)
    index[rng.integers(0, Q - 5, size=Q // 10)] = -1  # unmatched: not counted
    tl = rng.integers(0, L, size=P).astype(np.int32)
    ql = np.concatenate([rng.integers(0, L - 1, size=first_late), rng.integers(0, L, size=Q - first_late)]).astype(np.int32)
    ql[-5:], tl[index[-5:]] = L - 1, L - 1  # the last cell is used, and only by queries of a second trip
    table, early = np.zeros((L, L), dtype=np.int64), np.zeros((L, L), dtype=np.int64)
    ok = index >= 0
    np.add.at(table, (ql[ok], tl[index[ok]]), 1)
    np.add.at(early, (ql[:first_late][ok[:first_late]], tl[index[:first_late][ok[:first_late]]]), 1)
    assert table[L - 1, L - 1] >= 5 and early[L - 1].sum() == 0 and table.sum() == ok.sum() < Q
    assert np.array_equal(proc3d.nearest_confusion(index, ql, tl, L, device=gpu_device), table)
    dev = [torch.from_numpy(a).cuda(gpu_device) for a in (index, ql, tl)]
    assert np.array_equal(proc3d.nearest_confusion(*dev, L), table)
    dev[1][Q - 1] = L  # one bad query label, where only the second trip of the judge looks
    with pytest.raises(ValueError, match="outside"):
        proc3d.nearest_confusion(*dev, L)
    dev[1][Q - 1] = L - 1
    assert np.array_equal(proc3d.nearest_confusion(*dev, L), table)  # the call after a refused one is a whole one
