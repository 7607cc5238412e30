"""GPU: the `average` kernel (backprojection.c:36-55) at the sizes the project benchmarks and shards it, every voxel
against the C oracle, bit for bit (the contract is the reference's float32 sum in the order the views are given).

* the bench's four forms at 512^3 x 72 (bench.py ``average_forms``: uint8 binary, uint8 grey, float32 binary,
  float32 grey, masks resident on the device), with and without log, by every schedule the engine offers, host masks
  through ``Backprojection``, a second batch over the stored sums and a permuted view order;
* the dense scene at 512^3 x 72 (most footprints mixed);
* the reference's literal grid (301 x 301 x 561 x 60) with a default value, a third of it seen by no view;
* ragged pictures (1434 x 1077) under a close ring at 256^3 x 36;
* rank 3 of 8 of the 1024^3 x 72 grid, both partitions.

Committed digests (tests/golden/make_golden.py average) pin what the oracle computed when they were made.
"""
import json
import os

import numpy as np
import pytest

from oracle import oracle_c
from plant3dvision_amd import _native as nat
from plant3dvision_amd import scenes
from plant3dvision_amd.cl import EPS, Backprojection, averaging_table, img_as_float32
from plant3dvision_amd.sharded import rank_planes
from tests.helpers import grey_masks, scene, sha256, table_views

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 8)  # a GPU host grants 16 CPUs; os.cpu_count() counts the whole machine
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synthetic_digests.json")))


def _poses(views):
    return (np.stack([v[0] for v in views]), np.stack([v[1] for v in views]), np.stack([v[2] for v in views]))


def _same(got, want):
    """Bit for bit (-0.0 is not 0.0, every NaN payload counts)."""
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _float_masks(stack, log):
    """What cl.py:205-208 hands the kernel for uint8 masks: img_as_float32, then log(EPS + .) when asked."""
    f = img_as_float32(stack)
    if log:
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.log(EPS + f)
    return np.ascontiguousarray(f, dtype=np.float32)


class _Batch:
    """An averaging engine over a stack of masks resident on the device, run by the schedules it offers."""

    def __init__(self, shape, origin, vs, views, log, default_value=0.0, **kw):
        self.eng = nat.Engine(shape, origin, vs, nat.SC_MODE_AVERAGE, default_value=default_value, **kw)
        self.eng.set_lut(averaging_table(log))
        self.K, self.R, self.t = _poses(views)
        self.V, self.H, self.W = len(views), *views[0][3].shape
        self.ptr = self.eng.dev_alloc(self.V * self.H * self.W * 4)  # room for the float32 form

    def upload(self, stack):
        assert stack.shape == (self.V, self.H, self.W) and stack.flags["C_CONTIGUOUS"]
        self.code = nat.SC_MASK_F32 if stack.dtype == np.float32 else nat.SC_MASK_U8_LUT
        self.eng.dev_upload(self.ptr, stack)

    def run(self, vpl=0, brick=1, tile=1, order=None, again=False):
        """clear + the batch (views in ``order``, one call each, when given; a second whole batch over the stored sums
        when ``again``), launched ``vpl`` views at a time (0: all at once)."""
        e = self.eng
        e.set_option(nat.SC_OPT_VIEWS_PER_LAUNCH, vpl)
        e.set_option(nat.SC_OPT_AVG_BRICK, brick)
        e.set_option(nat.SC_OPT_AVG_TILE_F32, tile)
        e.clear()
        step = self.H * self.W * (4 if self.code == nat.SC_MASK_F32 else 1)
        if order is None:
            e.process_views_device(self.K, self.R, self.t, self.ptr, self.V, self.H, self.W, self.code)
        else:
            for q in order:
                e.process_views_device(self.K[q:q + 1], self.R[q:q + 1], self.t[q:q + 1], self.ptr + int(q) * step, 1,
                                       self.H, self.W, self.code)
        if again:
            e.flush()  # the second batch reads the sums the first one stored
            e.process_views_device(self.K, self.R, self.t, self.ptr, self.V, self.H, self.W, self.code)
        return e.get_values()

    def close(self):
        self.eng.dev_free(self.ptr)
        self.eng.close()


def _host_masks(shape, origin, vs, views, log, masks, as_float, default_value=0):
    """The class, fed host masks one by one like the reference's file loop (cl.py:282-303)."""
    bp = Backprojection(shape, origin, vs, type="averaging", log=log, default_value=default_value)
    for q, (K, R, t, _) in enumerate(views):
        bp.process_view(K, R, t, img_as_float32(masks[q]) if as_float else masks[q])
    got = bp.get_values().copy()
    bp.close()
    return got


# -- the bench's four forms at 512^3 x 72 --------------------------------------------------------------------------
@pytest.mark.parametrize("log", [False, True], ids=["nolog", "log"])
@pytest.mark.parametrize("masks", ["binary", "grey"])
def test_average_bench_forms_512_cubed_72_views_whole_grid(gpu_device, masks, log):
    """bench.py --full's averaging rows (uint8 and float32 forms of the binary masks and of the grey bytes of
    default_rng(4321)): the whole grid against the oracle -- one oracle run for both forms, since table[m] is
    img_as_float32(m) (and its log) bit for bit -- and the committed digest; then the same grid by one launch per
    view, launches of 10 views (the last holds 2), the voxel form instead of bricks, row-major float32 masks, and
    host masks through Backprojection.  Grey without log also: a second batch over the stored sums (FRESH = false)
    and the views submitted in a seeded permutation, each against the oracle fed the same views."""
    shape, origin, vs, views = scene(512, 72, "plant")
    stack = np.ascontiguousarray(np.stack([m for _, _, _, m in views]))
    if masks == "grey":
        stack = grey_masks(stack.shape)
    table = averaging_table(log)
    fstack = _float_masks(stack, log)
    assert _same(table[stack], fstack)
    want = oracle_c.average(shape, origin, vs, table_views(views, table, stack), nthreads=THREADS)
    key = f"average_plant_512_72_u8_{masks}" + ("_log" if log else "")
    gold = None if (masks, log) == ("grey", True) else GOLD[key]["sha256_float32"]  # (no digest for grey with log)
    if gold is not None:
        assert sha256(want) == gold, key
    b = _Batch(shape, origin, vs, views, log)
    try:
        for form, data in (("u8", stack), ("f32", fstack)):
            b.upload(data)
            got = b.run()
            assert _same(got, want), (form, "fused")
            if gold is not None:
                assert sha256(got) == gold, key
            for label, kw in (("per view", {"vpl": 1}), ("10 a launch", {"vpl": 10}), ("voxel form", {"brick": 0})):
                assert _same(b.run(**kw), want), (form, label)
            if form == "f32":
                assert _same(b.run(tile=0), want), (form, "row-major")
                assert _same(b.run(tile=0, vpl=10), want), (form, "row-major, 10 a launch")
            del got, data
        del fstack
        for as_float in (False, True):
            assert _same(_host_masks(shape, origin, vs, views, log, stack, as_float), want), ("host masks", as_float)
        if masks == "grey" and not log:
            b.upload(stack)
            # a second batch of the same 72 views over the stored sums
            oracle_c.average_planes(shape, origin, vs, table_views(views, table, stack), 0, 1, shape[0], values=want,
                                    nthreads=THREADS)
            assert _same(b.run(again=True), want), "second batch"
            assert _same(b.run(again=True, brick=0), want), "second batch, voxel form"
            # the order of the sum is part of the contract
            perm = np.random.default_rng(77).permutation(len(views))
            del want
            want = oracle_c.average(shape, origin, vs, table_views([views[q] for q in perm], table, stack[perm]),
                                    nthreads=THREADS)
            assert _same(b.run(order=perm), want), "permuted"
            assert _same(b.run(order=perm, vpl=10), want), "permuted, 10 a launch"
    finally:
        b.close()


# -- the dense scene ---------------------------------------------------------------------------------------------------
def test_average_dense_512_cubed_72_views_whole_grid(gpu_device):
    """The bench's dense scene (close cameras, an object that fills a third of every picture): most (brick, view)
    footprints are mixed, so most of the work is projected voxel by voxel.  uint8 table with log."""
    shape, origin, vs, views = scene(512, 72, "dense")
    table = averaging_table(True)
    want = oracle_c.average(shape, origin, vs, table_views(views, table), nthreads=THREADS)
    b = _Batch(shape, origin, vs, views, True)
    try:
        b.upload(np.ascontiguousarray(np.stack([m for _, _, _, m in views])))
        assert _same(b.run(), want)
        assert _same(b.run(vpl=10), want)
        assert _same(b.run(brick=0), want)
    finally:
        b.close()


# -- the reference's literal grid ---------------------------------------------------------------------------------------
def test_average_literal_grid_301x301x561_60_views_default_value(gpu_device):
    """configs/test_geom_pipe_real.toml's grid (301 x 301 x 561: rows of neither 16 nor 64 voxels) under the scan's 60
    views, default_value 0.5, uint8 binary masks with and without log: the whole grid.  The lower part of the box
    leaves every picture: a real share of voxels keeps exactly 0.5, and bricks straddle the picture edge."""
    shape, origin, vs, views = scenes.literal_real_plant_scene(60, "plant")
    assert shape == [301, 301, 561]
    stack = np.ascontiguousarray(np.stack([m for _, _, _, m in views]))
    unseen = None
    for log in (False, True):
        want = oracle_c.average(shape, origin, vs, table_views(views, averaging_table(log)), default_value=0.5,
                                nthreads=THREADS)
        # a view that sees a voxel adds table[0] / table[255]: 0.0 / 1.0 without log, log(EPS) / 0.0 with it -- only
        # a voxel no view sees keeps 0.5 in both
        unseen = (want == 0.5) if unseen is None else unseen & (want == 0.5)
        b = _Batch(shape, origin, vs, views, log, default_value=0.5)
        try:
            b.upload(stack)
            assert _same(b.run(), want), log
            assert _same(b.run(vpl=7), want), log
            assert _same(b.run(brick=0), want), log
        finally:
            b.close()
        assert _same(_host_masks(shape, origin, vs, views, log, stack, False, default_value=0.5), want), log
        del want
    assert 0.2 < unseen.mean() < 0.8, unseen.mean()
    # 1 x 16 x 64-voxel bricks (the brick form's unit) holding voxels no view sees beside voxels some view sees
    pad = np.pad(unseen, ((0, 0), (0, -shape[1] % 16), (0, -shape[2] % 64)), mode="edge")
    per = pad.reshape(shape[0], pad.shape[1] // 16, 16, pad.shape[2] // 64, 64)
    straddle = per.any(axis=(2, 4)) & ~per.all(axis=(2, 4))
    assert straddle.sum() > 100, straddle.sum()


# -- ragged pictures --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [False, True], ids=["nolog", "log"])
def test_average_ragged_pictures_256_cubed_36_views(gpu_device, log):
    """cfg 2's size with 1434 x 1077 pictures (W % 16, W % 4 and H % 32 not 0: the last uint8 strip, float32 tile
    and 32-row band are partial) and the ring close enough that the grid overflows every picture: uint8 table and
    float32, every schedule, the whole grid."""
    W, H = 1434, 1077
    assert W % 16 and W % 4 and H % 32
    shape, origin, vs, views = scene(256, 36, "plant", width=W, height=H, radius_factor=1.1, cx=W / 2, cy=H / 2)
    stack = np.ascontiguousarray(np.stack([m for _, _, _, m in views]))
    assert stack.shape == (36, H, W)
    rng = np.random.default_rng(8)
    ijk = np.stack([rng.integers(0, s, 20000) for s in shape], axis=1).astype(np.int32)
    _, _, ok = oracle_c.project(ijk, origin, vs, *views[0][:3], W, H)
    assert 0.05 < ok.mean() < 0.95, ok.mean()  # the grid overflows the picture
    table = averaging_table(log)
    want = oracle_c.average(shape, origin, vs, table_views(views, table), nthreads=THREADS)
    assert (want != 0).mean() > 0.05
    b = _Batch(shape, origin, vs, views, log)
    try:
        for form, data in (("u8", stack), ("f32", _float_masks(stack, log))):
            b.upload(data)
            for kw in ({}, {"vpl": 1}, {"vpl": 10}, {"brick": 0}) + (({"tile": 0},) if form == "f32" else ()):
                assert _same(b.run(**kw), want), (form, kw)
    finally:
        b.close()
    for as_float in (False, True):
        assert _same(_host_masks(shape, origin, vs, views, log, stack, as_float), want), ("host masks", as_float)


# -- cfg 4: a rank's planes of 1024^3 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("partition", ["cyclic", "slab"])
def test_average_1024_cubed_rank_3_of_8(gpu_device, partition):
    """BASELINE cfg 4's grid averaged by rank 3 of 8 (128 planes, global x up to 1023 when cyclic): every voxel against
    the oracle over the same planes with GLOBAL coordinates, and its committed digest.  uint8 binary masks, log."""
    shape, origin, vs, views = scene(1024, 72, "plant")
    planes = rank_planes(shape[0], 8, 3, partition)
    kw = {"cyclic": (3, 8)} if partition == "cyclic" else {"slab": (planes.start, planes.stop)}
    table = averaging_table(True)
    want = oracle_c.average_planes(shape, origin, vs, table_views(views, table), planes.start, planes.step,
                                   len(planes), nthreads=THREADS)
    key = f"average_plant_1024_72_{partition}_rank3of8_u8_binary_log"
    assert sha256(want) == GOLD[key]["sha256_float32"], key
    b = _Batch(shape, origin, vs, views, True, **kw)
    try:
        assert b.eng.slab_shape == (128, 1024, 1024)
        b.upload(np.ascontiguousarray(np.stack([m for _, _, _, m in views])))
        got = b.run()
        assert _same(got, want), partition
        assert sha256(got) == GOLD[key]["sha256_float32"], key
        del got
        assert _same(b.run(vpl=10), want), partition
    finally:
        b.close()
