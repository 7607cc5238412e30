"""GPU: ``plant3dvision_amd.metrics`` (``sc_eval_voxels`` / ``sc_eval_masks``, csrc/evaluate.hip) and the two
``tasks.evaluation`` functions against the checkers (tests/evaluation_oracle.py).  Every result is an integer count:
every comparison is exact equality, no tolerance."""
import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import metrics, proc3d
from plant3dvision_amd.tasks import evaluation as task
from tests import evaluation_oracle as oracle

SHAPE, GSHAPE = (9, 7, 13), (10, 7, 15)


def check_voxels(voxels, gts, device, background="background", **kw):
    """Counts and projections of the device against the checker's; returns the device's pair."""
    got, proj = metrics.voxel_confusion(voxels, gts, background=background, projections=True, device=device, **kw)
    want, wproj = oracle.voxel_histograms(voxels, gts, background=background, projections=True,
                                          min_contrast=kw.get("min_contrast", 10))
    print({k: (got[k], want[k]) for k in want})
    assert got == want and list(got) == list(want)
    assert all(type(x) is int for h in got.values() for x in h.values())
    assert list(proj) == list(want)
    for k in want:
        assert proj[k].dtype == np.uint8 and np.array_equal(proj[k], wproj[k]), k
    assert metrics.voxel_confusion(voxels, gts, background=background, device=device, **kw) == want  # without projections
    return got, proj


def _rename(d, old, new):
    return {(new if k == old else k): v for k, v in d.items()}


@pytest.fixture(scope="module")
def pool64():
    return oracle.adversarial_volumes(SHAPE, GSHAPE, 4, seed=11)


# ---- volumes ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pred_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("gt_dtype", [np.float64, np.float32, np.uint8, np.bool_])
def test_adversarial_pool_every_dtype(gpu_device, pred_dtype, gt_dtype):
    v, g = oracle.adversarial_volumes(SHAPE, GSHAPE, 4, seed=11, pred_dtype=pred_dtype, gt_dtype=gt_dtype)
    got, _ = check_voxels(v, g, gpu_device, background=None)
    # the volumes exercise what they are meant to, by the CHECKER's account
    assert all(h["tp"] > 0 and h["fp"] > 0 and h["tn"] > 0 and h["fn"] > 0 for h in got.values())
    if gt_dtype == np.float64:
        n = int(np.prod(SHAPE))
        assert all(h["tp"] + h["fp"] + h["tn"] + h["fn"] < n for h in got.values())  # 0.5 and NaN count nowhere


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "middle", "absent", "last"])
def test_background_position(gpu_device, pool64, where):
    v, g = pool64
    old = {"first": "c0", "middle": "c2", "last": "c3"}.get(where)
    if old:
        v, g = _rename(v, old, "background"), _rename(g, old, "background")
    got, proj = check_voxels(v, g, gpu_device)
    assert len(got) == (4 if where == "absent" else 3) and "background" not in got and "background" not in proj


@pytest.mark.gpu
def test_two_classes_contrast_and_int_volumes(gpu_device):
    v, g = oracle.adversarial_volumes(SHAPE, GSHAPE, 2, seed=12)
    check_voxels(v, g, gpu_device, background=None)
    check_voxels(v, g, gpu_device, background="c1")
    check_voxels(v, g, gpu_device, background=None, min_contrast=1.0)
    check_voxels(v, g, gpu_device, background=None, min_contrast=0.0)
    # other dtypes are converted on the host: int32 predictions, int16 ground truths
    rng = np.random.default_rng(13)
    vi = {k: rng.integers(-3, 40, size=SHAPE).astype(np.int32) for k in ("a", "b", "c")}
    gi = {k: rng.integers(0, 2, size=GSHAPE).astype(np.int16) for k in ("a", "b", "c")}
    check_voxels(vi, gi, gpu_device, background="a")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,gshape", [((1, 1, 1), (1, 1, 1)), ((5, 3, 1), (5, 3, 1)), ((3, 5, 67), (3, 5, 67)),
                                          ((2, 130, 129), (2, 130, 129)), ((3, 5, 64), (4, 6, 67)), ((4, 6, 16), (4, 7, 18))])
def test_vector_tails_and_misaligned_rows(gpu_device, shape, gshape):
    """nz of 1, 67, 129: quads that end a row early; 129 x 130: more than one block per plane; gz = 67 / 18 under
    nz = 64 / 16: every prediction row aligned, ground-truth rows at every misalignment."""
    for pred_dtype, gt_dtype in ((np.float32, np.uint8), (np.float64, np.float32), (np.float32, np.float64)):
        v, g = oracle.adversarial_volumes(shape, gshape, 3, seed=sum(shape), pred_dtype=pred_dtype, gt_dtype=gt_dtype)
        check_voxels(v, g, gpu_device, background="c1")


@pytest.mark.gpu
def test_views_with_an_odd_base_address(gpu_device):
    """Volumes that start 1 element into their buffers: no wide load is aligned."""
    v, g = oracle.adversarial_volumes((4, 6, 16), (4, 6, 16), 3, seed=14, pred_dtype=np.float32, gt_dtype=np.uint8)
    n = 4 * 6 * 16
    v2, g2 = {}, {}
    for k in v:
        pb, gb = np.zeros(n + 1, np.float32), np.zeros(n + 1, np.uint8)
        pb[1:], gb[1:] = v[k].reshape(-1), g[k].reshape(-1)
        v2[k], g2[k] = pb[1:].reshape(v[k].shape), gb[1:].reshape(g[k].shape)
        assert v2[k].flags["C_CONTIGUOUS"] and v2[k].ctypes.data % 16 == 4
    assert check_voxels(v2, g2, gpu_device, background=None)[0] == oracle.voxel_histograms(v, g, background=None)


@pytest.mark.gpu
@pytest.mark.parametrize("pred_dtype,gt_dtype", [(np.float32, np.uint8), (np.float64, np.float64), (np.float32, np.bool_)])
def test_device_tensors_equal_host_arrays(gpu_device, pred_dtype, gt_dtype):
    import torch
    v, g = oracle.adversarial_volumes(SHAPE, GSHAPE, 4, seed=15, pred_dtype=pred_dtype, gt_dtype=gt_dtype)
    want, wproj = check_voxels(v, g, gpu_device, background="c0")
    dev = f"cuda:{gpu_device}"
    tv, tg = {k: torch.from_numpy(a).to(dev) for k, a in v.items()}, {k: torch.from_numpy(a).to(dev) for k, a in g.items()}
    got, proj = metrics.voxel_confusion(tv, tg, background="c0", projections=True)
    assert got == want and all(np.array_equal(proj[k], wproj[k]) for k in wproj)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):  # read in place on torch's current stream
        assert metrics.voxel_confusion(tv, tg, background="c0") == want
    with pytest.raises(ValueError, match="all NumPy arrays or all CUDA tensors"):
        metrics.voxel_confusion(tv, g, background="c0")
    with pytest.raises(ValueError, match="contiguous"):
        metrics.voxel_confusion({k: t.transpose(0, 2) for k, t in tv.items()}, tg)


@pytest.mark.gpu
def test_slabs_equal_one_piece_and_calls_repeat(gpu_device):
    shape, gshape = (40, 33, 35), (41, 34, 37)
    v, g = oracle.adversarial_volumes(shape, gshape, 3, seed=16, pred_dtype=np.float32, gt_dtype=np.uint8)
    one, one_proj = metrics.voxel_confusion(v, g, background=None, projections=True, device=gpu_device)
    again, again_proj = metrics.voxel_confusion(v, g, background=None, projections=True, device=gpu_device)
    assert again == one and all(np.array_equal(one_proj[k], again_proj[k]) for k in one_proj)  # two identical calls agree
    want, wproj = oracle.voxel_histograms(v, g, background=None, projections=True)
    assert one == want and all(np.array_equal(one_proj[k], wproj[k]) for k in wproj)
    per_plane = 3 * 33 * 35 * 4 + 3 * 34 * 37  # one x-plane of every volume
    try:
        # room for 13 planes (and the counters, the projection and the volumes' padding): slabs of 13, 13, 13 and 1
        metrics.set_chunk_bytes(1024 + 3 * 33 * 35 + 256 + 6 * 256 + 13 * per_plane + per_plane // 2)
        got, proj = metrics.voxel_confusion(v, g, background=None, projections=True, device=gpu_device)
        assert got == one and all(np.array_equal(proj[k], one_proj[k]) for k in one_proj)
        metrics.set_chunk_bytes(1)  # less than one plane: one plane per slab
        assert metrics.voxel_confusion(v, g, background=None, device=gpu_device) == one
    finally:
        metrics.set_chunk_bytes(0)  # the default again
    assert metrics.voxel_confusion(v, g, background=None, device=gpu_device) == one


# ---- several x-planes per block ---------------------------------------------------------------------------------
# Every volume above gives a block ONE x-plane (tests/test_unit_plans_host.py): its loop over the planes of a run, the
# short last run, the LDS counters and seen[] across planes run here.  Each case first asserts, by the plan's replica
# and the CHECKER's account, that it is such a case.  Ground truths are one longer on every axis: their own pitches.
def _ids(shape):
    return "%dx%dx%d" % shape


def _longer(shape):
    return tuple(s + 1 for s in shape)


def _device_route(v, g, device, want, wproj, **kw):
    import torch
    tv, tg = ({k: torch.from_numpy(a).cuda(device) for k, a in d.items()} for d in (v, g))
    got, proj = metrics.voxel_confusion(tv, tg, projections=True, **kw)
    assert got == want and all(np.array_equal(proj[k], wproj[k]) for k in wproj)
    assert metrics.voxel_confusion(tv, tg, **kw) == want


@pytest.mark.gpu
@pytest.mark.parametrize("shape", oracle.LONG_SHAPES, ids=_ids)
@pytest.mark.parametrize("pred_dtype,gt_dtype", [(np.float32, np.uint8), (np.float32, np.float64), (np.float64, np.uint8),
                                                 (np.float64, np.float64)])
def test_long_volumes_counts_add_up_over_a_run_of_planes(gpu_device, shape, pred_dtype, gt_dtype):
    plan = oracle.quad_plan(*shape)
    assert plan["xc"] >= 2 and shape[0] % plan["xc"] == plan["last"] % plan["xc"]  # (the last run: short on three of the four)
    v, g = oracle.adversarial_volumes(shape, _longer(shape), 3, seed=sum(shape), pred_dtype=pred_dtype, gt_dtype=gt_dtype)
    got, proj = check_voxels(v, g, gpu_device, background="c1")
    # more voxels in one counter than a plane holds, and than a block adds in one plane: the planes of a run added up
    more = max(shape[1] * shape[2], 4 * plan["threads"])
    assert all(h["tp"] > 0 and h["fp"] > 0 and h["tn"] > more and h["fn"] > more for h in got.values())
    _device_route(v, g, gpu_device, got, proj, background="c1")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", oracle.LONG_SHAPES, ids=_ids)
def test_long_volumes_projection_of_single_planes(gpu_device, shape):
    """The adversarial pool predicts every class in every column of a long volume: its projection is all ones whatever
    ``seen[]`` does.  Here a column predicts its class in ONE plane or in none: the first, the last or a middle plane
    of a run, or a plane of the short last run."""
    pred_dtype, gt_dtype = ((np.float32, np.uint8), (np.float64, np.float64))[oracle.LONG_SHAPES.index(shape) % 2]
    v, g, at, placed = oracle.needle_volumes(shape, _longer(shape), 4, seed=5 + sum(shape), pred_dtype=pred_dtype, gt_dtype=gt_dtype)
    print(placed)
    assert set(placed) == set(oracle.needle_planes(shape[0], oracle.quad_plan(*shape))) and all(n > 0 for n in placed.values())
    want, wproj = oracle.voxel_histograms(v, g, background=None, projections=True)
    for c, k in enumerate(v):  # by the CHECKER's account: neither empty nor full, and exactly the needles
        assert 0 < wproj[k].sum() < wproj[k].size and np.array_equal(wproj[k], (at[c] >= 0).astype(np.uint8))
        assert want[k]["tp"] + want[k]["fp"] > 0
    got, proj = check_voxels(v, g, gpu_device, background=None)  # the host route
    _device_route(v, g, gpu_device, got, proj, background=None)
    v, g = _rename(v, "c2", "background"), _rename(g, "c2", "background")
    got, proj = check_voxels(v, g, gpu_device)
    _device_route(v, g, gpu_device, got, proj)


@pytest.mark.gpu
def test_slabs_of_a_long_volume_walk_runs_of_two_planes(gpu_device):
    shape, gshape = oracle.SLAB_SHAPE, _longer(oracle.SLAB_SHAPE)
    nx, ny, nz = shape
    v, g, at, placed = oracle.needle_volumes(shape, gshape, 3, seed=23, pred_dtype=np.float32, gt_dtype=np.uint8)
    want, wproj = oracle.voxel_histograms(v, g, background=None, projections=True)
    assert all(0 < wproj[k].sum() < wproj[k].size for k in wproj)
    one, one_proj = metrics.voxel_confusion(v, g, background=None, projections=True, device=gpu_device)
    assert one == want and all(np.array_equal(one_proj[k], wproj[k]) for k in wproj)
    per_plane = 3 * ny * nz * 4 + 3 * gshape[1] * gshape[2]  # one x-plane of every volume
    laid, pad = 1024 + 256 * ((3 * ny * nz + 255) // 256), 6 * 256  # the counters and the projection; the volumes' padding
    limit = laid + pad + oracle.SLAB_PLANES * per_plane + per_plane // 2
    # room for 4100 planes: slabs of 4100, 4100 and 1800 planes, in runs of 2, 2 and 1 planes per block
    assert (limit - laid - pad) // per_plane == oracle.SLAB_PLANES == 4100
    assert [oracle.quad_plan(p, ny, nz)["xc"] for p in (4100, 4100, 1800)] == [2, 2, 1]
    try:
        metrics.set_chunk_bytes(limit)
        got, proj = metrics.voxel_confusion(v, g, background=None, projections=True, device=gpu_device)
        assert got == one and all(np.array_equal(proj[k], one_proj[k]) for k in one_proj)
    finally:
        metrics.set_chunk_bytes(0)  # the default again
    assert metrics.voxel_confusion(v, g, background=None, projections=True, device=gpu_device)[0] == one


# ---- masks ------------------------------------------------------------------------------------------------------
# (n, 33, 577): two tile rows (a tile has 32) and two tile columns (10 words against a tile's 8), a last word of one bit
PICTURES = [(1, 1, 1), (3, 1, 1), (1, 37, 41), (3, 37, 41), (1, 64, 130), (3, 64, 130), (1, 33, 577), (2, 33, 577)]


@pytest.fixture(scope="module")
def pictures():
    return {key: oracle.border_pictures(*key, seed=21 + q) for q, key in enumerate(PICTURES)}


@pytest.mark.gpu
@pytest.mark.parametrize("key", PICTURES, ids=lambda k: "n%d_%dx%d" % k)
@pytest.mark.parametrize("amount", [0, 1, 2, 5, 40])
def test_mask_stacks_host_and_device(gpu_device, pictures, key, amount):
    import torch
    gt, pred = pictures[key]
    assert set(np.unique(pred)) <= {0, 1, 7, 255}
    if key[1] > 1:
        assert pred[:, 0].any() and pred[:, -1].any() and pred[:, :, 0].any() and pred[:, :, -1].any()
        assert all(pred[v, y, x] for v in range(key[0]) for y in (0, -1) for x in (0, -1))
    want = oracle.mask_stack_counts(gt, pred, amount)
    got = metrics.compare_mask_stacks(gt, pred, amount, device=gpu_device)
    print(got.tolist(), want.tolist())
    assert got.dtype == np.int64 and got.shape == (key[0], 4) and np.array_equal(got, want)
    assert (got.sum(axis=1) == key[1] * key[2]).all()
    dev = metrics.compare_mask_stacks(torch.from_numpy(gt).cuda(gpu_device), torch.from_numpy(pred).cuda(gpu_device), amount)
    assert isinstance(dev, np.ndarray) and np.array_equal(dev, want)


@pytest.mark.gpu
def test_mask_batches_under_the_chunk_limit(gpu_device, pictures):
    gt, pred = pictures[(3, 37, 41)]
    want = oracle.mask_stack_counts(gt, pred, 2)
    try:
        metrics.set_chunk_bytes(1)  # one picture per batch
        assert np.array_equal(metrics.compare_mask_stacks(gt, pred, 2, device=gpu_device), want)
    finally:
        metrics.set_chunk_bytes(0)
    assert np.array_equal(metrics.compare_mask_stacks(gt.astype(bool), pred.astype(bool), 2, device=gpu_device), want)
    # a dilation far larger than the picture: everything is set wherever a pixel was
    huge = metrics.compare_mask_stacks(gt, pred, 10 ** 6, device=gpu_device)
    assert np.array_equal(huge, oracle.mask_stack_counts(gt, pred, 37 + 41))
    empty = np.zeros_like(pred)
    assert np.array_equal(metrics.compare_mask_stacks(gt, empty, 10 ** 6, device=gpu_device), oracle.mask_stack_counts(gt, empty, 3))


@pytest.mark.gpu
def test_compare_masks_end_to_end(gpu_device, pictures):
    gt, pred = pictures[(3, 64, 130)]
    for amount in (0, 3):
        m = metrics.CompareMasks(gt[0], pred[0], amount)
        rows = [oracle.mask_counts(gt[0], pred[0], amount)]
        assert m.as_dict() == oracle.metrics_dict(rows)
        for q in (1, 2):
            m.add(gt[q], pred[q])
            rows.append(oracle.mask_counts(gt[q], pred[q], amount))
        assert m.as_dict() == oracle.metrics_dict(rows) and m.miou() is not None
        assert metrics.MaskEvaluator(amount, device=gpu_device).evaluate(gt[1], pred[1]) == rows[1]


class _File:
    def __init__(self, fid, array, channel, shot_id):
        self.id, self.array = fid, array
        self._md = {"channel": channel, "shot_id": shot_id}

    def get_metadata(self, key=None, default=None):
        return self._md if key is None else self._md.get(key, default)


@pytest.mark.gpu
def test_the_two_run_functions_end_to_end(gpu_device, pictures, pool64):
    gts, preds, rows = [], [], {"leaf": [], "stem": []}
    want = {"evaluation-results": {}}
    for label, keys in (("leaf", [(3, 37, 41), (1, 64, 130)]), ("stem", [(3, 64, 130)])):
        shot = 0
        for key in keys:
            gt, pred = pictures[key]
            for q in range(key[0]):
                gts.append(_File(f"{shot:05d}_{label}", gt[q], label, f"{shot:05d}"))
                preds.append(_File(f"{shot:05d}_{label}_pred", pred[q], label, f"{shot:05d}"))
                row = oracle.mask_counts(gt[q], pred[q], 2)
                want["evaluation-results"][preds[-1].id] = oracle.metrics_dict([row])
                rows[label].append(row)
                shot += 1
        want[label] = oracle.metrics_dict(rows[label])
    got = task.segmentation2d_evaluation_run(gts, preds, ["leaf", "stem"], dilation_amount=2)
    assert got == want
    v, g = pool64
    v, g = _rename(v, "c1", "background"), _rename(g, "c1", "background")
    assert task.voxels_evaluation_run(v, g) == oracle.voxel_histograms(v, g)


# ---- the life of the work buffers -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_work_buffers_grow_are_released_and_come_back(gpu_device, pictures):
    """A small call, a larger one on another stream that has to replace the work buffers, the small one in the larger
    buffers, a refused call, the release, and the small one in buffers allocated anew: each the checker's counts."""
    import torch
    gs, ps = pictures[(1, 37, 41)]
    gl, pl = pictures[(3, 64, 130)]
    ws, wl = oracle.mask_stack_counts(gs, ps, 5), oracle.mask_stack_counts(gl, pl, 5)
    v, g = oracle.adversarial_volumes((6, 5, 9), (6, 5, 9), 3, seed=17, pred_dtype=np.float32, gt_dtype=np.uint8)
    wv = oracle.voxel_histograms(v, g, background=None)
    nat.backend().call("sc_eval_release")  # whatever earlier tests left: the first call allocates
    tgs, tps, tgl, tpl = (torch.from_numpy(a).cuda(gpu_device) for a in (gs, ps, gl, pl))
    tv, tg = ({k: torch.from_numpy(a).cuda(gpu_device) for k, a in d.items()} for d in (v, g))
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))  # the uploads
    c1 = metrics.compare_mask_stacks(tgs, tps, 5)
    with torch.cuda.stream(side):
        c2 = metrics.compare_mask_stacks(tgl, tpl, 5)  # grows: waits for the first call before it frees its buffers
    c3 = metrics.compare_mask_stacks(tgs, tps, 5)
    h1 = metrics.voxel_confusion(tv, tg, background=None)  # the other entry shares the buffers
    with pytest.raises(ValueError, match="dilation_amount must not be negative"):
        nat.check(nat.backend().call("sc_eval_masks", tgs.data_ptr(), tps.data_ptr(), 1, 1, 37, 41, -1, gpu_device, 0,
                                     nat.addr(np.zeros(4, np.int64))), "sc_eval_masks", "sc_eval_last_error")
    c4 = metrics.compare_mask_stacks(tgs, tps, 5)
    assert np.array_equal(c1, ws) and np.array_equal(c2, wl) and np.array_equal(c3, ws) and np.array_equal(c4, ws) and h1 == wv
    proc3d.release_device_buffers()  # calls sc_eval_release
    assert np.array_equal(metrics.compare_mask_stacks(tgs, tps, 5), ws)
    assert metrics.voxel_confusion(v, g, background=None, device=gpu_device) == wv  # the host route
    assert np.array_equal(metrics.compare_mask_stacks(gs, ps, 5, device=gpu_device), ws)
