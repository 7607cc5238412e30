"""CPU: the replicas of the stand-alone units' launch plans (tests/evaluation_oracle.py::quad_plan for csrc/sc_quads.h,
tests/nearest_oracle.py::launch_caps and its strides for csrc/nearest.hip and csrc/sc_points.h), and the sizes the GPU
tests chose by them.  Every outer loop of those kernels is bounded by a cap -- blocks that fill the device, 256
partials, 2048 far blocks, 1024 blocks -- and goes round a second time only past it.  A constant that leaves the
sources, or is retuned so that a chosen size no longer passes its cap, fails here, on a machine without a GPU, and
says which GPU test lost its reason."""
import numpy as np
import pytest

from tests import evaluation_oracle as ev
from tests import nearest_oracle as nn


# ---- the quad walk ------------------------------------------------------------------------------------------------
def test_the_constants_are_read_from_the_sources():
    assert ev.source_constant("sc_quads.h", "kQuadThreads") == 256
    assert ev.source_constant("sc_quads.h", "kFillBlocks") == 4096
    assert ev.source_constant("sc_quads.h", "kRunPlanesLog2") == 20
    caps = nn.launch_caps()
    assert caps == {"kB": 256, "kPartials": 256, "kFarBlocks": 2048, "kLdsTable": 1024, "kNearRings": 3,
                    "label_blocks": 1024, "finite_blocks": 1024}
    with pytest.raises(AssertionError, match="kNoSuchConstant was expected once"):  # a constant that left the source
        ev.source_constant("sc_quads.h", "kNoSuchConstant")
    with pytest.raises(AssertionError, match="found 0 times"):
        ev.source_constant("sc_points.h", "a cap that is not there", r"std::min<int64_t>\(\(n \+ 1023\) / 1024,\s*(\d+)\)")


def test_the_suites_old_shapes_walk_one_plane_and_the_benchmarks_32():
    """The gap: the longest and the widest volume the unit tests had, against the size the tools measure."""
    assert ev.quad_plan(40, 33, 35) == {"tiles": 2, "xc": 1, "runs": 40, "last": 1, "threads": 256}
    assert ev.quad_plan(2, 130, 129) == {"tiles": 17, "xc": 1, "runs": 2, "last": 1, "threads": 256}
    for planes, ny, nz in ((9, 7, 13), (6, 5, 7), (3, 5, 67), (12, 33, 35), (37, 41, 29), (4, 6, 16)):
        assert ev.quad_plan(planes, ny, nz)["xc"] == 1
    assert ev.quad_plan(512, 512, 512) == {"tiles": 256, "xc": 32, "runs": 16, "last": 32, "threads": 256}


def test_the_long_shapes_walk_several_planes():
    plans = {shape: ev.quad_plan(*shape) for shape in ev.LONG_SHAPES}
    assert [(p["tiles"], p["xc"], p["last"]) for p in plans.values()] == [(1, 2, 1), (1, 3, 1), (2, 2, 2), (2, 2, 1)]
    for (nx, ny, nz), p in plans.items():
        assert (p["runs"] - 1) * p["xc"] + p["last"] == nx and 1 <= p["last"] <= p["xc"]
        assert (p["tiles"] - 1) * p["threads"] < ny * ((nz + 3) // 4) <= p["tiles"] * p["threads"]
        # a class count above this is more than a plane holds and more than a block adds in one: planes have added up
        assert max(ny * nz, 4 * p["threads"]) * 8 < nx * ny * nz
    # (4099, 2, 8): whole aligned quads, 4 live threads of 256; (2100, 17, 61): the second tile has 16 live threads
    assert 2 * (8 // 4) == 4 and 17 * 16 - 256 == 16
    kinds = {shape: set(ev.needle_planes(shape[0], p)) for shape, p in plans.items()}
    assert kinds[(4099, 2, 8)] == {"first", "last", "short"} and kinds[(10000, 3, 7)] == {"first", "last", "middle", "short"}
    assert kinds[(2100, 17, 61)] == {"first", "last"} and kinds[(2049, 17, 64)] == {"first", "last", "short"}
    for shape, p in plans.items():  # the kinds are disjoint and cover every plane
        planes = np.concatenate(list(ev.needle_planes(shape[0], p).values()))
        assert np.array_equal(np.sort(planes), np.arange(shape[0]))


def test_the_slabs_of_the_long_host_volume():
    """10000 planes in slabs of 4100: 4100 and 4100 planes in runs of 2, then 1800 planes one by one."""
    nx, ny, nz = ev.SLAB_SHAPE
    slabs = [min(ev.SLAB_PLANES, nx - xa) for xa in range(0, nx, ev.SLAB_PLANES)]
    assert slabs == [4100, 4100, 1800]
    assert [ev.quad_plan(s, ny, nz)["xc"] for s in slabs] == [2, 2, 1] and ev.quad_plan(nx, ny, nz)["xc"] == 3


def test_needle_volumes_place_what_they_say():
    shape, gshape = (10000, 3, 7), (10001, 4, 8)
    v, g, at, placed = ev.needle_volumes(shape, gshape, 4, seed=3)
    assert set(placed) == {"first", "last", "middle", "short"} and all(n > 0 for n in placed.values())
    assert sum(placed.values()) == int((at >= 0).sum())
    _, proj = ev.voxel_histograms(v, g, background=None, projections=True)
    for c, k in enumerate(v):  # the checker predicts a class exactly in the columns that have a needle
        assert np.array_equal(proj[k], (at[c] >= 0).astype(np.uint8)) and 0 < proj[k].sum() < proj[k].size
        assert v[k].shape == shape and g[k].shape == gshape


# ---- nearest ------------------------------------------------------------------------------------------------------
def test_the_old_sizes_stay_inside_the_capped_grids():
    """The gap: the largest clouds the suite had (31 411 mesh vertices, 1900 labelled queries, 500 far queries)."""
    assert nn.box_stride(31411) >= 31411 and nn.sums_stride(31411) >= 31411
    assert nn.labels_stride(1900, 2500) >= 2500
    assert nn.far_waves(500) >= 500
    assert nn.finite_stride(31411) * 3 >= 3 * 31411  # an uncapped grid takes the 3 n coordinates in 3 trips


def test_the_new_sizes_pass_the_caps():
    caps = nn.launch_caps()
    # the far list: more certainly-far queries (the GPU test counts them) than wavefronts can be had only if Q - near is
    assert nn.far_waves(nn.FAR_Q) == 8192 and nn.FAR_Q - nn.FAR_Q // nn.FAR_NEAR_EVERY == 9000 > nn.far_waves(nn.FAR_Q)
    # sums: the queries past the first trip
    assert nn.sums_stride(nn.SUMS_Q) == 65536 and nn.SUMS_Q - nn.sums_stride(nn.SUMS_Q) == 464
    # box: the last 300 targets are seen on a second trip only
    assert nn.box_stride(nn.LATE_P) == 65536 and nn.LATE_P - nn.box_stride(nn.LATE_P) == 300
    # the judge of device queries: the last coordinate on the fourth trip, one more than any uncapped grid takes
    stride = nn.finite_stride(nn.LATE_Q)
    assert stride == 262144 and (3 * nn.LATE_Q - 1) // stride == 3
    assert (3 * 31411 - 1) // nn.finite_stride(31411) == 2
    # labels and confusion: the last 777 queries on a second trip; both tables' forms
    assert nn.labels_stride(nn.CONFUSION_Q, nn.CONFUSION_P) == 262144 and nn.CONFUSION_Q - 262144 == 777
    assert 32 * 32 <= caps["kLdsTable"] < 33 * 33


def test_the_grid_plan_and_the_far_count():
    """The port of ``nn::plan_grid``: 600 targets in the unit box get a grid of about 600 cells whose farthest ring
    lies beyond the near rings; queries 10^3 extents away are certainly far, queries inside are not."""
    rng = np.random.default_rng(1)
    t = rng.uniform(0.0, 1.0, size=(600, 3))
    lo, h, n = nn.plan_grid(t)
    assert np.array_equal(lo, t.min(axis=0)) and 300 <= n.prod() <= 1200 and n.min() > 2 * nn.launch_caps()["kNearRings"]
    assert np.array_equal(nn.cell_of(t.max(axis=0), lo, h, n), n - 1) and np.array_equal(nn.cell_of(lo - 1e300, lo, h, n), [0, 0, 0])
    far = t.mean(axis=0) + 1e3 * np.array([1.0, -0.5, 0.25]) + rng.uniform(-1.0, 1.0, size=(50, 3))
    assert nn.certainly_far(far, t, nn.nearest_all_pairs(far, t)[1]) == 50
    assert nn.ring_bound(h, 3) > 0.1 * 0.1
    assert nn.certainly_far(far, t, nn.nearest_all_pairs(far, t)[1], max_distance=0.1) == 0  # the bound passes md2: settled
    assert nn.certainly_far(t[:50], t, np.zeros(50)) == 0
    one = np.tile([[1.0, 2.0, 3.0]], (5, 1))  # no extent: one cell
    assert nn.plan_grid(one)[1:][0] == 1.0 and nn.plan_grid(one)[2].tolist() == [1, 1, 1]
