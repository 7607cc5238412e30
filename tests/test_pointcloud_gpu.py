"""GPU: the multiclass ``PointCloud`` task -- ``proc3d.select_classes`` (``sc_select_classes``, csrc/class_select.hip),
``proc3d.vol2pcd_class`` (``sc_vol2pcd_class``) and ``tasks.proc3d.point_cloud_run`` against the checkers
(tests/pointcloud_oracle.py: the reference's lines as written, and oracle/vol2pcd_oracle.py).  Winner bytes and counts
are integers: they are compared for equality.  A class's cloud is compared bit for bit with ``vol2pcd`` of the same
occupancy, and with the oracle at the tolerances of tests/test_vol2pcd.py::_check."""
import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import proc3d
from plant3dvision_amd.tasks import proc3d as task
from tests import pointcloud_oracle as oracle
from tests.evaluation_oracle import LONG_SHAPES, SLAB_PLANES, SLAB_SHAPE, quad_plan  # the run plan's replica

SHAPE = (6, 5, 7)
DEFAULT = (1.0, 10.0, 0.2)
ORIGIN, VS = np.array([1.5, -2.0, 7.0]), 0.5


def check_select(voxels, params, device, want=None):
    """Winner bytes, labels and counts of the device against the literal lines; returns the device's winner."""
    got, labels, counts = proc3d.select_classes(voxels, *params, device=device)
    if want is None:
        want = oracle.literal_winner(voxels, *params)
    if not isinstance(got, np.ndarray):
        got = got.cpu().numpy()
    print(params, counts.tolist(), want[2].tolist())
    assert labels == want[1] == list(voxels.keys())
    assert got.dtype == np.uint8 and got.shape == want[0].shape and np.array_equal(got, want[0])
    assert counts.dtype == np.int64 and np.array_equal(counts, want[2])
    return got


# ---- the rule ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.uint8, np.bool_])
def test_adversarial_pool_every_dtype_and_parameter_set(gpu_device, dtype):
    owned = none = 0
    for q, bg in enumerate([None, 0, 2, 4]):  # the background absent, first, in the middle, last
        stack = oracle.adversarial_stack(SHAPE, 5, seed=31 + q, dtype=dtype, background_at=bg)
        for params in oracle.PARAMETER_SETS:
            got = check_select(stack, params, gpu_device)
            owned += int((got != oracle.NONE).sum())
            none += int((got == oracle.NONE).sum())
    assert owned > 0 and none > 0  # the pool exercises both outcomes, by the CHECKER's account


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 3, 1), (3, 5, 3), (3, 5, 67), (2, 3, 64), (2, 130, 129)])
def test_row_tails_and_misaligned_rows(gpu_device, shape):
    """nz of 1, 3, 67, 129: quads that end a row early and rows that start at every misalignment (byte stores and
    scalar loads); nz = 64: every quad whole and aligned; 130 x 129: more than one block per plane."""
    for dtype in (np.float32, np.float64, np.uint8):
        stack = oracle.adversarial_stack(shape, 3, seed=sum(shape), dtype=dtype, background_at=1)
        check_select(stack, DEFAULT, gpu_device)
        check_select(stack, (0.5, 1.0, 0.2), gpu_device)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.uint8])
def test_aligned_rows_with_every_class_count(gpu_device, dtype):
    """nz a multiple of 4 and aligned buffers: the launch that takes its wide loads three classes at a time, with
    0, 1 and 2 classes left over, on host arrays (through the slab) and on device tensors."""
    import torch
    for L in (2, 3, 4, 5, 6, 7, 8):
        stack = oracle.adversarial_stack((3, 5, 8), L, seed=200 + L, dtype=dtype, background_at=(L - 1 if L % 2 else None))
        for params in (DEFAULT, (0.5, 1.0, 0.2)):
            want = oracle.literal_winner(stack, *params)
            check_select(stack, params, gpu_device, want)
            check_select({k: torch.from_numpy(v).cuda(gpu_device) for k, v in stack.items()}, params, gpu_device, want)


@pytest.mark.gpu
def test_views_with_an_odd_base_address(gpu_device):
    """Volumes that start 1 element into their buffers, on the host and on the device: no wide load is aligned; a
    winner volume that starts 1 byte into its buffer (the device route writes it in place): no 4-byte store is."""
    import torch
    shape, n = (4, 6, 16), 4 * 6 * 16
    for dtype, rem in ((np.float32, 4), (np.float64, 8), (np.uint8, 1)):
        stack = oracle.adversarial_stack(shape, 3, seed=41, dtype=dtype, background_at=0)
        want = oracle.literal_winner(stack, *DEFAULT)
        host, dev = {}, {}
        for k, v in stack.items():
            buf = np.zeros(n + 1, dtype)
            buf[1:] = v.reshape(-1)
            host[k] = buf[1:].reshape(shape)
            assert host[k].flags["C_CONTIGUOUS"] and host[k].ctypes.data % 16 == rem
            dev[k] = torch.from_numpy(buf).cuda(gpu_device)[1:].view(shape)
            assert dev[k].is_contiguous() and dev[k].data_ptr() % 16 == rem
        check_select(host, DEFAULT, gpu_device, want)
        check_select(dev, DEFAULT, gpu_device, want)
    # the library itself, with a winner pointer that is odd
    stack = {k: torch.from_numpy(v).cuda(gpu_device) for k, v in oracle.adversarial_stack(shape, 3, seed=42, dtype=np.float32).items()}
    want = oracle.literal_winner({k: t.cpu().numpy() for k, t in stack.items()}, *DEFAULT)
    wbuf = torch.full((n + 2,), 77, dtype=torch.uint8, device=f"cuda:{gpu_device}")
    pp, counts = np.array([t.data_ptr() for t in stack.values()], dtype=np.uintp), np.zeros(3, np.int64)
    torch.cuda.synchronize(gpu_device)
    nat.check(nat.backend().call("sc_select_classes", nat.addr(pp), nat.SC_EVAL_F32, 3, -1, 4, 6, 16, 1.0, 10.0, 0.2, 1, gpu_device,
                                 0, wbuf.data_ptr() + 1, nat.addr(counts)), "sc_select_classes", "sc_select_last_error")
    out = wbuf.cpu().numpy()
    assert out[0] == 77 and out[-1] == 77 and np.array_equal(out[1:-1].reshape(shape), want[0]) and np.array_equal(counts, want[2])


@pytest.mark.gpu
def test_two_classes_without_background_and_thirty_two(gpu_device):
    for dtype in (np.float32, np.float64):
        two = oracle.adversarial_stack(SHAPE, 2, seed=51, dtype=dtype)
        for params in oracle.PARAMETER_SETS:
            check_select(two, params, gpu_device)
    got, labels, counts = proc3d.select_classes(two, *DEFAULT, background="c1", device=gpu_device)  # another label as the background
    renamed = {("background" if k == "c1" else k): v for k, v in two.items()}
    want = oracle.literal_winner(renamed, *DEFAULT)
    assert np.array_equal(got, want[0]) and np.array_equal(counts, want[2]) and labels == ["c0", "c1"]
    for bg in (None, 31, 17):
        many = oracle.adversarial_stack((3, 4, 9), 32, seed=52, dtype=np.float32, background_at=bg)
        got = check_select(many, (1.0, 1.0, 0.2), gpu_device)
        check_select(many, DEFAULT, gpu_device)
    assert len(np.unique(got)) > 16  # high class indices are winners too
    # other dtypes are converted on the host
    rng = np.random.default_rng(53)
    ints = {k: rng.integers(-3, 40, size=SHAPE).astype(np.int32) for k in ("a", "background", "c")}
    check_select(ints, (1.0, 1.0, 0.2), gpu_device)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.uint8, np.bool_])
def test_device_tensors_equal_host_arrays(gpu_device, dtype):
    import torch
    stack = oracle.adversarial_stack(SHAPE, 4, seed=61, dtype=dtype, background_at=1)
    host = check_select(stack, DEFAULT, gpu_device)
    tens = {k: torch.from_numpy(v).cuda(gpu_device) for k, v in stack.items()}
    winner, labels, counts = proc3d.select_classes(tens, *DEFAULT)
    assert winner.is_cuda and winner.dtype == torch.uint8 and winner.device.index == gpu_device
    assert np.array_equal(winner.cpu().numpy(), host) and isinstance(counts, np.ndarray)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):  # read and written in place on torch's current stream
        again = proc3d.select_classes(tens, *DEFAULT)[0]
    side.synchronize()
    assert np.array_equal(again.cpu().numpy(), host)
    with pytest.raises(ValueError, match="all NumPy arrays or all CUDA tensors"):
        proc3d.select_classes(dict(tens, extra=stack["c0"]))
    with pytest.raises(ValueError, match="contiguous"):
        proc3d.select_classes({k: t.transpose(0, 2) for k, t in tens.items()})


@pytest.mark.gpu
def test_slabs_equal_one_piece_and_calls_repeat(gpu_device):
    shape = (40, 33, 35)
    stack = oracle.adversarial_stack(shape, 3, seed=71, dtype=np.float32, background_at=0)
    want = oracle.literal_winner(stack, *DEFAULT)
    one = check_select(stack, DEFAULT, gpu_device, want)
    check_select(stack, DEFAULT, gpu_device, want)  # two identical calls agree
    per_plane = 3 * 33 * 35 * 4 + 33 * 35  # one x-plane of every volume and of the winners
    try:
        # room for 13 planes (and the counters and the buffers' padding): slabs of 13, 13, 13 and 1
        proc3d.set_select_chunk_bytes(256 + 4 * 256 + 13 * per_plane + per_plane // 2)
        assert np.array_equal(check_select(stack, DEFAULT, gpu_device, want), one)
        proc3d.set_select_chunk_bytes(1)  # less than one plane: one plane per slab
        assert np.array_equal(check_select(stack, DEFAULT, gpu_device, want), one)
    finally:
        proc3d.set_select_chunk_bytes(0)  # the default again
    assert np.array_equal(check_select(stack, DEFAULT, gpu_device, want), one)


# ---- several x-planes per block -----------------------------------------------------------------------------------
# Every volume above gives a block ONE x-plane (tests/test_unit_plans_host.py pins the plan's replica and these
# shapes): the loop over the planes of a run, its short last run and the LDS counters across planes run here.
@pytest.mark.gpu
@pytest.mark.parametrize("shape", LONG_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.uint8])
@pytest.mark.parametrize("L", [3, 4, 5])
def test_long_volumes_counts_add_up_over_a_run_of_planes(gpu_device, shape, dtype, L):
    """(4099, 2, 8): the launch of whole aligned quads, 252 threads of the block beyond the plane; (10000, 3, 7): row
    tails, three planes per run; (2100, 17, 61) and (2049, 17, 64): two tiles, the second with 16 live threads."""
    import torch
    plan = quad_plan(*shape)
    assert plan["xc"] >= 2 and shape[0] % plan["xc"] == plan["last"] % plan["xc"]
    stack = oracle.adversarial_stack(shape, L, seed=300 + L + sum(shape), dtype=dtype, background_at=L // 2)
    tens = {k: torch.from_numpy(v).cuda(gpu_device) for k, v in stack.items()}
    assert all(t.data_ptr() % 16 == 0 for t in tens.values())
    for params in (DEFAULT, (0.5, 1.0, 0.2)):
        want = oracle.literal_winner(stack, *params)
        # by the CHECKER's account: owned and unowned voxels, and more voxels in one counter than a plane holds and than
        # a block adds in one plane -- the planes of a run added up
        assert (want[0] != oracle.NONE).any() and (want[0] == oracle.NONE).any()
        assert want[2].max() > max(shape[1] * shape[2], 4 * plan["threads"]) and want[2][L // 2] == 0
        check_select(stack, params, gpu_device, want)
        check_select(tens, params, gpu_device, want)


@pytest.mark.gpu
def test_slabs_of_a_long_volume_walk_runs_of_two_planes(gpu_device):
    shape = SLAB_SHAPE
    nx, ny, nz = shape
    stack = oracle.adversarial_stack(shape, 3, seed=72, dtype=np.float32, background_at=1)
    want = oracle.literal_winner(stack, *DEFAULT)
    one = check_select(stack, DEFAULT, gpu_device, want)
    per_plane = 3 * ny * nz * 4 + ny * nz  # one x-plane of every volume and of the winners
    laid, pad = 256, 4 * 256  # the counters; the buffers' padding
    limit = laid + pad + SLAB_PLANES * per_plane + per_plane // 2
    # room for 4100 planes: slabs of 4100, 4100 and 1800 planes, in runs of 2, 2 and 1 planes per block
    assert (limit - laid - pad) // per_plane == SLAB_PLANES == 4100
    assert [quad_plan(p, ny, nz)["xc"] for p in (4100, 4100, 1800)] == [2, 2, 1] and quad_plan(nx, ny, nz)["xc"] == 3
    try:
        proc3d.set_select_chunk_bytes(limit)
        assert np.array_equal(check_select(stack, DEFAULT, gpu_device, want), one)
    finally:
        proc3d.set_select_chunk_bytes(0)  # the default again
    assert np.array_equal(check_select(stack, DEFAULT, gpu_device, want), one)


# ---- a class of a winner volume as a cloud ------------------------------------------------------------------------
def _bits_equal(a, b):
    return (len(a.points) == len(b.points) and np.array_equal(np.asarray(a.points).view(np.uint64), np.asarray(b.points).view(np.uint64))
            and np.array_equal(np.asarray(a.normals).view(np.uint64), np.asarray(b.normals).view(np.uint64)))


@pytest.fixture(scope="module")
def scenes():
    return {shape: oracle.organ_scene(shape, seed=7, dtype=np.float32) for shape in [(37, 41, 29), (24, 20, 33)]}


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [0, 1], ids=["whole", "scratch-limit-1"])
def test_vol2pcd_class_bit_equal_to_vol2pcd_of_the_occupancy(gpu_device, scenes, limit):
    import torch
    winner = oracle.literal_winner(scenes[(37, 41, 29)], 1.0, 1.0, 0.2)[0]
    resident = torch.from_numpy(winner).cuda(gpu_device)
    try:
        proc3d.set_scratch_limit(limit)
        for c in (1, 2, 3, 4):
            want = proc3d.vol2pcd((winner == c).astype(np.uint8), ORIGIN, VS, 1.0, device=gpu_device, as_open3d=False)
            assert len(want.points) > 100
            assert _bits_equal(proc3d.vol2pcd_class(winner, c, ORIGIN, VS, 1.0, device=gpu_device, as_open3d=False), want), c
            assert _bits_equal(proc3d.vol2pcd_class(resident, c, ORIGIN, VS, 1.0, as_open3d=False), want), c
        for c in (5, 200):  # a class index no voxel has: an empty cloud
            for w in (winner, resident):
                got = proc3d.vol2pcd_class(w, c, ORIGIN, VS, 1.0, device=gpu_device, as_open3d=False)
                assert got.points.shape == (0, 3) and got.normals.shape == (0, 3)
        none = proc3d.vol2pcd_class(winner, 255, ORIGIN, VS, 1.0, device=gpu_device, as_open3d=False)  # the voxels of no class
        assert _bits_equal(none, proc3d.vol2pcd((winner == 255).astype(np.uint8), ORIGIN, VS, 1.0, device=gpu_device, as_open3d=False))
    finally:
        proc3d.set_scratch_limit(8 << 30)


@pytest.mark.gpu
def test_vol2pcd_class_in_real_slabs(gpu_device):
    """70 planes under the smallest scratch limit: at level_set_value 0 a slab is 52 planes with its halo, so the volume
    goes through in 9 slabs (the 37 planes of the case above fit into one whatever the limit)."""
    import torch
    rng = np.random.default_rng(81)
    shape = (70, 21, 19)
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1)
    winner = np.full(shape, 255, np.uint8)
    for q in range(14):
        c = rng.uniform(0, 1, 3) * np.array(shape)
        r = rng.uniform(2, 6)
        winner[((g - c) ** 2).sum(-1) < r * r] = 1 + q % 3
    winner[20:60, 9:11, 4:15] = 2  # a sheet along x, across slab borders
    resident = torch.from_numpy(winner).cuda(gpu_device)
    try:
        for c in (1, 2, 3):
            proc3d.set_scratch_limit(0)
            whole = proc3d.vol2pcd((winner == c).astype(np.uint8), ORIGIN, VS, 0.0, device=gpu_device, as_open3d=False)
            assert len(whole.points) > 300
            proc3d.set_scratch_limit(1)
            assert _bits_equal(proc3d.vol2pcd_class(winner, c, ORIGIN, VS, 0.0, device=gpu_device, as_open3d=False), whole), c
            assert _bits_equal(proc3d.vol2pcd_class(resident, c, ORIGIN, VS, 0.0, as_open3d=False), whole), c
    finally:
        proc3d.set_scratch_limit(8 << 30)


# ---- end to end -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(37, 41, 29), (24, 20, 33)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("bp,mc,ms,lsv", [(1.0, 10.0, 0.2, 1.0), (1.0, 1.0, 0.2, 0.0), (0.25, 1.5, 0.2, 1.0)])
def test_point_cloud_run_end_to_end(gpu_device, scenes, shape, bp, mc, ms, lsv):
    """By the checker's account (tests/pointcloud_oracle.py::organ_scene, seed 7) every organ owns 132..1431 voxels and
    yields 460..1614 points under every parameter set on both shapes -- asserted below: no class is silently empty."""
    import torch
    scene = scenes[shape]
    assert list(scene) == ["background", "stem", "leaf", "flower", "fruit"]
    pts, nrm, cols, labels, per_class = oracle.literal_run(scene, ORIGIN, VS, lsv, bp, mc, ms, colors=task.POINT_CLOUD_COLORS)
    print(per_class)
    assert all(460 <= per_class[k] <= 1614 for k in oracle.ORGANS)
    cloud, meta = task.point_cloud_run(scene, ORIGIN, VS, lsv, bp, mc, ms, device=gpu_device)
    got_labels = meta["labels"]
    assert list(meta) == ["labels"]
    assert {k: got_labels.count(k) for k in oracle.ORGANS} == per_class  # the point count per class
    assert got_labels == labels
    gp, gn, gc = np.asarray(cloud.points), np.asarray(cloud.normals), np.asarray(cloud.colors)
    assert gp.shape == pts.shape
    np.testing.assert_allclose(gp, pts, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(gn, nrm, rtol=1e-12, atol=1e-12)
    assert np.array_equal(gc, cols)
    tens = {k: torch.from_numpy(v).cuda(gpu_device) for k, v in scene.items()}
    tcloud, tmeta = task.point_cloud_run(tens, ORIGIN, VS, lsv, bp, mc, ms)
    assert tmeta == meta and np.array_equal(np.asarray(tcloud.colors), gc)
    assert np.array_equal(np.asarray(tcloud.points).view(np.uint64), gp.view(np.uint64))
    assert np.array_equal(np.asarray(tcloud.normals).view(np.uint64), gn.view(np.uint64))


@pytest.mark.gpu
def test_single_volume_branch_on_the_device(gpu_device, scenes):
    vol = (scenes[(24, 20, 33)]["stem"] > 4).astype(np.uint8)
    want = proc3d.vol2pcd(vol, ORIGIN, VS, 1.0, device=gpu_device, as_open3d=False)
    assert len(want.points) > 100
    for voxels in (vol, {"only": vol}):
        cloud, meta = task.point_cloud_run(voxels, ORIGIN, VS, device=gpu_device)
        assert meta == {"voxel_size": VS}
        assert np.array_equal(np.asarray(cloud.points), want.points) and np.array_equal(np.asarray(cloud.normals), want.normals)


# ---- the life of the work buffers -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_work_buffers_grow_are_released_and_come_back(gpu_device):
    """A small call, a larger one on another stream that has to replace the work buffers, the small one in the larger
    buffers, a refused call, the release, and the small one in buffers allocated anew: each the checker's winners."""
    import torch
    small = oracle.adversarial_stack((6, 5, 9), 3, seed=91, dtype=np.float32, background_at=2)
    large = oracle.adversarial_stack((12, 33, 35), 4, seed=92, dtype=np.float64, background_at=0)
    ws, wl = oracle.literal_winner(small, *DEFAULT), oracle.literal_winner(large, *DEFAULT)
    nat.backend().call("sc_select_release")  # whatever earlier tests left: the first call allocates
    tsmall = {k: torch.from_numpy(v).cuda(gpu_device) for k, v in small.items()}
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))  # the uploads
    check_select(tsmall, DEFAULT, gpu_device, ws)
    with torch.cuda.stream(side):
        check_select(large, DEFAULT, gpu_device, wl)  # host volumes: the slabs grow the buffers
    check_select(tsmall, DEFAULT, gpu_device, ws)
    check_select(small, DEFAULT, gpu_device, ws)
    with pytest.raises(ValueError, match="L must be 2..32"):
        pp = np.array([t.data_ptr() for t in tsmall.values()], dtype=np.uintp)
        nat.check(nat.backend().call("sc_select_classes", nat.addr(pp), nat.SC_EVAL_F32, 1, -1, 6, 5, 9, 1.0, 10.0, 0.2, 1, gpu_device, 0,
                                     tsmall["c0"].data_ptr(), nat.addr(np.zeros(4, np.int64))), "sc_select_classes", "sc_select_last_error")
    check_select(tsmall, DEFAULT, gpu_device, ws)
    proc3d.release_device_buffers()  # calls sc_select_release
    check_select(tsmall, DEFAULT, gpu_device, ws)
    check_select(small, DEFAULT, gpu_device, ws)  # the host route
    check_select(large, DEFAULT, gpu_device, wl)
