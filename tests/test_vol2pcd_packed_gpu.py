"""vol2pcd on the packed labels of a sharded run, in one process: a ``PackedGrid`` packed by hand by the contract of
``include/spacecarve.h`` -- the word-at-once path, the per-voxel path, several ranks in both partitions, and slabs."""
import functools

import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import proc3d, sharded

_ORIGIN = np.array([1.5, -2.0, 7.0])
_VS = 0.5
_WHOLE = 8 << 30  # the default scratch limit


@functools.lru_cache(maxsize=None)
def _labels(shape):
    """A ball of 1 in random -1 / 0."""
    rng = np.random.default_rng(sum(shape))
    lab = rng.integers(-1, 1, size=shape).astype(np.int8)
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    c = [(s - 1) / 2 for s in shape]
    lab[(x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= (min(shape) / 2 - 0.6) ** 2] = 1
    assert set(np.unique(lab)) == {-1, 0, 1}
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def _dense(shape):
    """The cloud of the same occupancy as a uint8 volume, in one piece."""
    return proc3d.vol2pcd((_labels(shape) == 1).astype(np.uint8), _ORIGIN, _VS, 0.0, as_open3d=False)


def _pack(lab, bits, partition, world):
    """Rank r's planes flattened; voxel j at bit bits * (j % (32 / bits)) of little-endian word j // (32 / bits)."""
    import torch
    nx, ny, nz = lab.shape
    per = 32 // bits
    rank_bytes = nat.packed_bytes(-(-nx // world) * ny * nz, bits)
    assert rank_bytes % 4 == 0
    words = np.zeros((world, rank_bytes // 4), dtype=np.uint32)
    for r in range(world):
        own = lab[list(sharded.rank_planes(nx, world, r, partition))].reshape(-1)
        val = (own & 3).astype(np.uint32) if bits == 2 else (own == 1).astype(np.uint32)
        j = np.arange(own.size)
        np.bitwise_or.at(words[r], j // per, val << (bits * (j % per)).astype(np.uint32))
    recv = torch.from_numpy(words.view(np.uint8).reshape(-1).copy()).cuda()
    return sharded.PackedGrid(recv, rank_bytes, world, partition, lab.shape, bits, 0)


def _bits_equal(a, b):
    return (a.points.shape == b.points.shape and np.array_equal(a.points.view(np.uint64), b.points.view(np.uint64))
            and np.array_equal(a.normals.view(np.uint64), b.normals.view(np.uint64)))


def _grid(shape, bits, partition, world):
    lab = _labels(shape)
    pg = _pack(lab, bits, partition, world)
    got = pg.unpack().cpu().numpy()
    assert np.array_equal(got, lab if bits == 2 else (lab == 1)), "the test packed the labels wrongly"
    return pg


_CASES = [(bits, partition, world) for bits in (1, 2) for partition in ("cyclic", "slab") for world in (1, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("bits,partition,world", _CASES)
@pytest.mark.parametrize("shape", [(9, 8, 12), (7, 5, 9)], ids=["plane96-word-at-once", "plane45-per-voxel"])
def test_packed_grid_gives_the_cloud_of_its_occupancy(gpu_device, shape, bits, partition, world):
    """A plane of 96 voxels is whole words at 1 and 2 bits (one word located per 16 voxels; nx = 9 is no multiple of
    world = 3); a plane of 45 voxels is not (every voxel located, and n = 315 is no multiple of 16)."""
    pg = _grid(shape, bits, partition, world)
    cloud = proc3d.vol2pcd(pg, _ORIGIN, _VS, 0.0, as_open3d=False)
    print(f"{shape} {bits} bit {partition} world {world}: {len(cloud.points)} points")
    assert len(cloud.points) > 0
    assert _bits_equal(cloud, _dense(shape))


@pytest.mark.gpu
@pytest.mark.parametrize("bits,partition,world", _CASES)
def test_packed_grid_in_slabs(gpu_device, bits, partition, world):
    """(70, 7, 9) under a scratch limit of one byte: slabs of the least size (52 planes), whose first plane is not
    plane 0 -- the cloud of the grid in one piece and of the uint8 occupancy."""
    shape = (70, 7, 9)
    pg = _grid(shape, bits, partition, world)
    try:
        proc3d.set_scratch_limit(1)
        slabs = proc3d.vol2pcd(pg, _ORIGIN, _VS, 0.0, as_open3d=False)
    finally:
        proc3d.set_scratch_limit(_WHOLE)
    whole = proc3d.vol2pcd(pg, _ORIGIN, _VS, 0.0, as_open3d=False)
    print(f"{shape} {bits} bit {partition} world {world}: slabs {len(slabs.points)} points, one piece {len(whole.points)}")
    assert len(slabs.points) > 0
    assert _bits_equal(slabs, _dense(shape))
    assert _bits_equal(slabs, whole)
