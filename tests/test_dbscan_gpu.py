"""GPU: ``proc3d.cluster_dbscan`` (``sc_dbscan``, csrc/dbscan.hip) against the checker (tests/dbscan_oracle.py: the
literal sequential loop), label for label: ``np.array_equal``, no tolerance."""
import numpy as np
import pytest

from plant3dvision_amd import proc3d, scenes
from plant3dvision_amd.cl import Backprojection
from tests import dbscan_oracle as oracle


def check(points, eps, min_points, device):
    """Run the kernels on ``points``, compare with the checker, return the labels."""
    got = proc3d.cluster_dbscan(points, eps, min_points, device=device)
    want = oracle.labels(points, eps, min_points)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == (len(points),)
    diff = int(np.count_nonzero(got != want))
    print(f"P {len(points)} eps {eps} min_points {min_points}: clusters {int(want.max()) + 1 if len(want) else 0}, "
          f"noise {int((want == -1).sum())}, different {diff}")
    assert np.array_equal(got, want)
    return got


@pytest.fixture(scope="module")
def blobs():
    cloud = oracle.blobs_cloud()
    return cloud, oracle.structure(cloud, **oracle.BLOBS)


# ---- 1: blobs, as given and permuted ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_blobs_and_their_permutation(gpu_device, blobs):
    cloud, st = blobs
    want = st["labels"]
    assert cloud.shape == (1900, 3)
    # the cloud exercises what it is meant to, by the CHECKER's account
    assert want.max() + 1 >= 2 and (want == -1).sum() >= 1 and st["border"].sum() >= 1 and st["contested"].sum() >= 1
    assert st["ties"] == 0
    got = proc3d.cluster_dbscan(cloud, device=gpu_device, **oracle.BLOBS)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    perm = np.random.default_rng(5).permutation(len(cloud))
    check(np.ascontiguousarray(cloud[perm]), device=gpu_device, **oracle.BLOBS)  # its own checker run, not permuted labels


# ---- 2: lattice: pairs at exactly eps ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "shifted", "negative"])
def test_lattice_ties(gpu_device, form):
    cloud = oracle.lattice_cloud()
    st = oracle.structure(cloud, **oracle.LATTICE)
    assert st["ties"] > 0 and st["labels"].max() >= 1
    if form == "shifted":  # leaves the lattice differences exact
        cloud = cloud + np.array([1e6, -1e6, 0.5])
    elif form == "negative":
        cloud = -cloud - 3.0
    assert oracle.structure(cloud, **oracle.LATTICE)["ties"] == st["ties"]
    got = check(cloud, device=gpu_device, **oracle.LATTICE)
    if form != "negative":
        assert np.array_equal(got, st["labels"])


# ---- 3: a border point between two groups -----------------------------------------------------------------------
def _two_groups():
    a = np.array([[-0.125 * k, 0.0, 0.0] for k in range(6)])        # six points within 0.625: all core at min_points 6
    b = np.array([[1.75 + 0.125 * k, 0.0, 0.0] for k in range(6)])
    mid = np.array([[0.875, 0.0, 0.0]])  # 0.875 from the nearest of each group, exactly 1.0 from their second
    return a, b, mid


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["a_b_mid", "b_a_mid", "mid_b_a"])
def test_border_point_follows_the_smaller_index(gpu_device, order):
    a, b, mid = _two_groups()
    parts = {"a": a, "b": b, "mid": mid}
    names = order.split("_")
    cloud = np.ascontiguousarray(np.concatenate([parts[n] for n in names]))
    got = check(cloud, 1.0, 6, gpu_device)
    at = {n: sum(len(parts[m]) for m in names[:k]) for k, n in enumerate(names)}
    first = [n for n in names if n != "mid"][0]  # the group with the smaller smallest index is cluster 0
    second = [n for n in names if n != "mid"][1]
    assert set(got[at[first]:at[first] + 6]) == {0} and set(got[at[second]:at[second] + 6]) == {1}
    assert got[at["mid"]] == 0


# ---- 4: sizes around the wavefront and the block ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257])
def test_sizes_and_min_points(gpu_device, P):
    rng = np.random.default_rng(100 + P)
    spread = rng.uniform(0.0, 4.0, size=(P, 3))
    tight = rng.uniform(0.0, 0.5, size=(P, 3))  # every point within eps of every other: min_points = P is reached
    for mp in (0, 1, P, P + 1):
        check(spread, 1.0, mp, gpu_device)
        got = check(tight, 1.0, mp, gpu_device)
        assert np.all(got == (-1 if mp == P + 1 else 0))


@pytest.mark.gpu
def test_empty_cloud(gpu_device):
    import torch
    got = proc3d.cluster_dbscan(np.zeros((0, 3)), 1.0, 5, device=gpu_device)
    assert got.dtype == np.int32 and got.shape == (0,)
    dev = proc3d.cluster_dbscan(torch.zeros((0, 3), dtype=torch.float64, device=f"cuda:{gpu_device}"), 1.0, 5)
    assert dev.is_cuda and dev.dtype == torch.int32 and tuple(dev.shape) == (0,)


# ---- 5: the union-find's worst case -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_chain_is_one_cluster(gpu_device):
    eps = 0.5
    n = 5000
    perm = np.random.default_rng(9).permutation(n)
    cloud = np.zeros((n, 3))
    cloud[:, 0] = perm * (0.9 * eps)  # neighbours on the line are far apart in index
    got = check(cloud, eps, 2, gpu_device)
    assert np.all(got == 0)


@pytest.mark.gpu
def test_min_points_one_counts_components(gpu_device):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    cloud = np.random.default_rng(21).uniform(0.0, 10.0, size=(2000, 3))
    eps = 0.7
    i, j = oracle.neighbour_pairs(cloud, eps)
    ncomp, _ = connected_components(coo_matrix((np.ones(len(i), dtype=np.int8), (i, j)), shape=(2000, 2000)), directed=False)
    assert 100 < ncomp < 2000
    got = check(cloud, eps, 1, gpu_device)
    assert got.min() == 0 and got.max() + 1 == ncomp


# ---- 6: one heavy cell; one far outlier -------------------------------------------------------------------------
@pytest.mark.gpu
def test_heavy_cell(gpu_device):
    rng = np.random.default_rng(33)
    cloud = np.concatenate([np.tile([[1.25, -2.5, 0.75]], (300, 1)), [1.25, -2.5, 0.75] + rng.uniform(-1.5, 1.5, size=(50, 3))])
    cloud = np.ascontiguousarray(cloud[rng.permutation(len(cloud))])
    check(cloud, 0.4, 5, gpu_device)
    check(cloud, 0.4, 301, gpu_device)  # the copies alone are 300: core only with a neighbour beside them


@pytest.mark.gpu
@pytest.mark.parametrize("eps", [0.9, 1e-3])
def test_far_outlier(gpu_device, blobs, eps):
    """One point at 1e12 stretches the grid to ~1e12 (eps 0.9) or ~1e15 (eps 1e-3) cells per axis: beyond 32 bits and
    beyond the clamp of the cell coordinates."""
    cloud = np.concatenate([blobs[0][:600], [[1e12, -1e12, 1e12]]])
    cloud = np.ascontiguousarray(np.roll(cloud, 7, axis=0))
    got = check(cloud, eps, 5 if eps > 0.1 else 1, gpu_device)
    assert got.max() >= 1


# ---- 7: determinism ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_three_runs_are_identical(gpu_device, blobs):
    cloud, st = blobs
    runs = [proc3d.cluster_dbscan(cloud, device=gpu_device, **oracle.BLOBS) for _ in range(3)]
    assert np.array_equal(runs[0], st["labels"])
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


# ---- 8: device in, device out -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_tensor_and_side_stream(gpu_device, blobs):
    import torch
    cloud, st = blobs
    lattice = oracle.lattice_cloud()
    want_lattice = oracle.labels(lattice, **oracle.LATTICE)
    ta = torch.from_numpy(cloud).cuda(gpu_device)
    tb = torch.from_numpy(lattice).cuda(gpu_device)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))  # the uploads
    la = proc3d.cluster_dbscan(ta, **oracle.BLOBS)
    with torch.cuda.stream(side):  # another stream of the same device, right behind: the work buffers are reused in order
        lb = proc3d.cluster_dbscan(tb, **oracle.LATTICE)
    la2 = proc3d.cluster_dbscan(ta, **oracle.BLOBS)
    side.synchronize()
    torch.cuda.current_stream(gpu_device).synchronize()
    assert la.is_cuda and la.dtype == torch.int32 and tuple(la.shape) == (1900,)
    assert np.array_equal(la.cpu().numpy(), st["labels"])
    assert np.array_equal(lb.cpu().numpy(), want_lattice)
    assert np.array_equal(la2.cpu().numpy(), st["labels"])
    assert np.array_equal(proc3d.cluster_dbscan(cloud, device=gpu_device, **oracle.BLOBS), la.cpu().numpy())  # the host route
    with pytest.raises(ValueError):
        proc3d.cluster_dbscan(ta.float(), **oracle.BLOBS)


# ---- 9: the cloud of a carve ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_carved_cloud(gpu_device):
    shape, origin, vs, views = scenes.make_scene(48, 8, "plant")
    bp = Backprojection(shape, origin, vs, device=gpu_device)
    for K, R, t, m in views:
        bp.process_view(K, R, t, m)
    pcd = proc3d.vol2pcd(bp, np.array(origin), vs, 1.0, device=gpu_device, as_open3d=False)
    bp.close()
    P = len(pcd)
    print("carved cloud:", P, "points")
    assert 500 < P <= 20000
    got = check(np.asarray(pcd.points), 2.0 * vs, 5, gpu_device)
    assert np.array_equal(proc3d.cluster_dbscan(pcd, 2.0 * vs, 5, device=gpu_device), got)  # anything with .points
    assert got.max() >= 0


# ---- 10: what only the device can find --------------------------------------------------------------------------
@pytest.mark.gpu
def test_non_finite_in_device_points(gpu_device, blobs):
    import torch
    cloud, st = blobs
    for bad in (float("nan"), float("inf")):
        t = torch.from_numpy(cloud).cuda(gpu_device)
        t[1234, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            proc3d.cluster_dbscan(t, **oracle.BLOBS)
    with pytest.raises(ValueError, match="non-finite coordinate in point 7"):
        broken = cloud.copy()
        broken[7, 2] = np.nan
        proc3d.cluster_dbscan(broken, device=gpu_device, **oracle.BLOBS)
    # the call after a refused one is a whole one
    assert np.array_equal(proc3d.cluster_dbscan(torch.from_numpy(cloud).cuda(gpu_device), **oracle.BLOBS).cpu().numpy(), st["labels"])


# ---- 11: the life of the work buffers ---------------------------------------------------------------------------
def _blobs(P, seed):
    """``oracle.blobs_cloud``'s form with P points: four Gaussian blobs of P / 5 and P / 5 points of uniform noise."""
    rng = np.random.default_rng(seed)
    centres = np.array([[0.0, 0.0, 0.0], [6.5, 0.0, 0.0], [0.0, 12.0, 3.0], [10.0, 10.0, -4.0]])
    parts = [c + rng.normal(scale=1.3, size=(P // 5, 3)) for c in centres]
    parts.append(rng.uniform(-6.0, 16.0, size=(P - 4 * (P // 5), 3)))
    return np.ascontiguousarray(np.concatenate(parts))


@pytest.mark.gpu
def test_work_buffers_grow_are_released_and_come_back(gpu_device):
    """A small cloud, a larger one on another stream that has to replace the work buffers, the small one in the larger
    buffers, a refused call, the release, and the small one in buffers allocated anew: each the checker's labels."""
    import torch
    from plant3dvision_amd import _native as nat
    small, large = _blobs(300, 41), _blobs(6000, 42)
    ws, wl = oracle.labels(small, **oracle.BLOBS), oracle.labels(large, **oracle.BLOBS)
    assert ws.max() >= 0 and (ws == -1).any() and wl.max() >= 1 and (wl == -1).any()
    nat.backend().call("sc_dbscan_release")  # whatever earlier tests left: the first call allocates
    ts, tl = torch.from_numpy(small).cuda(gpu_device), torch.from_numpy(large).cuda(gpu_device)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))  # the uploads
    l1 = proc3d.cluster_dbscan(ts, **oracle.BLOBS)
    with torch.cuda.stream(side):
        l2 = proc3d.cluster_dbscan(tl, **oracle.BLOBS)  # grows: waits for the first call before it frees its buffers
    l3 = proc3d.cluster_dbscan(ts, **oracle.BLOBS)
    with pytest.raises(ValueError, match="eps must be finite"):
        proc3d.cluster_dbscan(ts, -1.0, 5)
    l4 = proc3d.cluster_dbscan(ts, **oracle.BLOBS)
    side.synchronize()
    torch.cuda.current_stream(gpu_device).synchronize()
    assert np.array_equal(l1.cpu().numpy(), ws)
    assert np.array_equal(l2.cpu().numpy(), wl)
    assert np.array_equal(l3.cpu().numpy(), ws)
    assert np.array_equal(l4.cpu().numpy(), ws)
    nat.backend().call("sc_dbscan_release")
    assert np.array_equal(proc3d.cluster_dbscan(ts, **oracle.BLOBS).cpu().numpy(), ws)
    assert np.array_equal(proc3d.cluster_dbscan(small, device=gpu_device, **oracle.BLOBS), ws)  # the host route
