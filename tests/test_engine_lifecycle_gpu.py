"""GPU: an engine's whole life, twenty times over -- create, reach every buffer and event the host side makes lazily
(staging slots and their growth, host-bit arenas, descriptor ring, control block, survivor lists rebuilt, dead bytes, the
padded-row snapshot, every read-back form, both sparse paths, averaging verdicts, timers, spans, the self-test's
temporaries, gathers through a communicator of one), close.  Every read-back of every cycle equals the first cycle's
bit for bit, and the first cycle's volumes equal the C oracle's.  Free device memory is not asserted (the device is
shared): that nothing is freed twice or kept is the owners' business (csrc/sc_own.h, tools/own_rehearsal.cpp)."""
import types

import numpy as np
import pytest

from oracle import oracle_c
from plant3dvision_amd import _native as nat
from plant3dvision_amd import scenes
from tests.helpers import pack_labels_np, scene, unpack_sparse_np

pytestmark = pytest.mark.gpu

SHAPE = (12, 20, 70)  # nz is no multiple of 64: the state's rows are padded, read-backs go through the snapshot
VIEWS = 8             # the fused brick form: at least kMinFusedViews, more than dense_views
CYCLES = 20


def _pictures(height, width):
    # the scanner's camera scaled to the small picture, on a ring close enough that the volume holds all three labels
    # (voxels outside a picture keep 0) and every brick is mixed
    s = width / scenes.WIDTH
    return scene(SHAPE, VIEWS, "plant", width=width, height=height, fx=scenes.FX * s, fy=scenes.FY * s, cx=width / 2.0,
                 cy=height / 2.0, radius_factor=0.8)


@pytest.fixture(scope="module")
def setting():
    shape, origin, vs, small = _pictures(48, 64)
    _, _, _, large = _pictures(96, 128)  # a second, larger mask: the staging slots grow
    S = types.SimpleNamespace(shape=list(shape), origin=origin, vs=vs, small=small, large=large)
    S.K, S.R, S.t = (np.stack([v[q] for v in small]) for q in range(3))
    S.stack = np.ascontiguousarray(np.stack([m for _, _, _, m in small]))
    S.table = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    S.fstack = np.ascontiguousarray(np.sqrt(S.table)[S.stack])
    S.carve_host = oracle_c.carve(S.shape, origin, vs, small + large, nthreads=4)
    S.carve_dev = oracle_c.carve(S.shape, origin, vs, small + small, nthreads=4)
    S.average = oracle_c.average(S.shape, origin, vs, [(K, R, t, S.table[m]) for K, R, t, m in small] +
                                 [(K, R, t, S.fstack[q]) for q, (K, R, t, _) in enumerate(small)], nthreads=4)
    try:
        S.comm = nat.Comm.available()
    except nat.SpaceCarveError:
        S.comm = False
    return S


def _download(eng, ptr, nbytes, dtype=np.uint8):
    out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
    eng.dev_download(out, ptr)
    return out


def _cycle(dev, S, comm):
    got = {}
    nvox, nbricks = int(np.prod(S.shape)), nat.sparse_bricks(*S.shape)
    V, H, W = S.stack.shape

    # host masks: through the staging slots (which grow at the first larger mask), then through the host-bit arenas
    eng = nat.Engine(S.shape, S.origin, S.vs, nat.SC_MODE_CARVE, device=dev)
    for host_pack in (0, 1):
        eng.set_option(nat.SC_OPT_HOST_PACK, host_pack)
        for K, R, t, m in S.small + S.large:
            eng.process_view(K, R, t, m, nat.SC_MASK_U8)
        got["host masks, host_pack %d" % host_pack] = eng.get_values() if host_pack else eng.get_values_i8()
        eng.clear()
    eng.close()

    # a device batch in the fused brick form, under timers and a span; a second one with the lists rebuilt
    eng = nat.Engine(S.shape, S.origin, S.vs, nat.SC_MODE_CARVE, device=dev)
    eng.set_option(nat.SC_OPT_TIME_KERNELS, 1)
    eng.set_option(nat.SC_OPT_RESERVE_EVENTS, 64)
    ptr = eng.dev_alloc(S.stack.nbytes)
    eng.dev_upload(ptr, S.stack)
    eng.span_begin()
    eng.process_views_device(S.K, S.R, S.t, ptr, V, H, W, nat.SC_MASK_U8)
    eng.flush()
    assert eng.span_end() > 0.0
    got["fused counts"] = np.array(eng.fused_counts())
    assert got["fused counts"][0] > 0  # live bricks: the brick form ran
    got["sparse, fresh fused batch"] = unpack_sparse_np(eng.get_values_sparse(nbricks), nat.sparse_rank_bytes(nbricks, nbricks), 1, S.shape)
    assert eng.kernel_stats(nat.SC_KERNEL_FLAGS)[0] == 1 and eng.kernel_stats(nat.SC_KERNEL_STEP)[0] == 1
    eng.reset_kernel_stats()
    assert eng.kernel_stats(nat.SC_KERNEL_FLAGS) == (0, 0.0)
    eng.set_option(nat.SC_OPT_LIST_CAP, 4096)
    eng.process_views_device(S.K, S.R, S.t, ptr, V, H, W, nat.SC_MASK_U8)
    eng.flush()
    got["fused counts, second batch"] = np.array(eng.fused_counts())
    got["get_values"] = eng.get_values()
    got["get_values_i8"] = eng.get_values_i8()
    pptr, pbytes = eng.values_packed(2)
    eng.synchronize()
    got["values_packed"] = _download(eng, pptr, pbytes, np.uint32)[:(nvox + 15) // 16]
    got["get_values_wire2"] = eng.get_values_wire2(np.empty(S.shape, dtype=np.int32))
    got["get_values_packed 2"] = eng.get_values_packed(2)
    got["get_values_packed 1"] = eng.get_values_packed(1)
    got["sparse, second batch"] = unpack_sparse_np(eng.get_values_sparse(nbricks), nat.sparse_rank_bytes(nbricks, nbricks), 1, S.shape)
    dptr = eng.values_device_ptr()
    eng.synchronize()
    got["values_device_ptr"] = _download(eng, dptr, nvox * 4, np.int32).reshape(S.shape)
    got["selftest_division"] = np.array(eng.selftest_division(1024))
    if comm is not None:  # a communicator of one: the engine's pack, the collective, the event behind it
        stride = nat.sparse_rank_bytes(nbricks, nbricks)
        recv = eng.dev_alloc(stride)
        eng.all_gather_sparse(comm, nbricks, recv, stride)
        eng.synchronize()
        got["all_gather_sparse"] = unpack_sparse_np(_download(eng, recv, stride), stride, 1, S.shape)
        eng.dev_free(recv)
        stride = nat.packed_bytes(nvox, 2)
        recv = eng.dev_alloc(stride)
        eng.all_gather_packed(comm, 2, recv, stride)
        eng.synchronize()
        got["all_gather_packed"] = _download(eng, recv, stride, np.uint32)[:(nvox + 15) // 16]
        eng.dev_free(recv)
    eng.dev_free(ptr)
    eng.close()

    # averaging: bytes through the table, then float32 masks (the brick form's two verdict buffers)
    avg = nat.Engine(S.shape, S.origin, S.vs, nat.SC_MODE_AVERAGE, device=dev)
    avg.set_lut(S.table)
    for stack, dtype in ((S.stack, nat.SC_MASK_U8_LUT), (S.fstack, nat.SC_MASK_F32)):
        ptr = avg.dev_alloc(stack.nbytes)
        avg.dev_upload(ptr, stack)
        avg.process_views_device(S.K, S.R, S.t, ptr, V, H, W, dtype)
        avg.synchronize()
        avg.dev_free(ptr)
    got["average"] = avg.get_values()
    avg.close()

    # engines whose device half comes up on a thread: closed without a call, and straight after a clear
    nat.Engine(S.shape, S.origin, S.vs, nat.SC_MODE_CARVE, device=dev, deferred=True).close()
    eng = nat.Engine(S.shape, S.origin, S.vs, nat.SC_MODE_CARVE, device=dev, deferred=True)
    eng.clear()
    eng.close()
    return got


def test_twenty_lives_of_an_engine_read_back_the_same_bits(gpu_device, setting):
    S = setting
    # (ONE communicator for all the cycles: ncclCommInitRank + ncclCommDestroy take half a second, forty times what the
    # rest of a cycle takes; what the engine keeps for a gather -- send buffers, header landing place, the events behind
    # the collectives -- is made anew in every cycle all the same)
    comm = nat.Comm(nat.Comm.unique_id(), 1, 0, gpu_device) if S.comm else None
    try:
        _twenty_lives(gpu_device, S, comm)
    finally:
        if comm is not None:
            comm.close()


def _twenty_lives(dev, S, comm):
    first = _cycle(dev, S, comm)
    assert np.array_equal(first["host masks, host_pack 0"], S.carve_host)
    assert np.array_equal(first["host masks, host_pack 1"], S.carve_host)
    assert np.array_equal(first["sparse, fresh fused batch"], oracle_c.carve(S.shape, S.origin, S.vs, S.small, nthreads=4))
    for key in ("get_values", "get_values_i8", "get_values_wire2", "sparse, second batch", "values_device_ptr", "all_gather_sparse"):
        if key in first:
            assert np.array_equal(first[key], S.carve_dev), key
    for key in ("values_packed", "get_values_packed 2", "all_gather_packed"):
        if key in first:
            assert np.array_equal(first[key], pack_labels_np(S.carve_dev, 2)), key
    assert np.array_equal(first["get_values_packed 1"], pack_labels_np(S.carve_dev, 1))
    assert np.array_equal(first["average"], S.average)
    assert first["selftest_division"][0] == 0
    assert len(np.unique(S.carve_dev)) == 3  # (a volume with every label in it)
    for k in range(1, CYCLES):
        again = _cycle(dev, S, comm)
        assert again.keys() == first.keys()
        for key, want in first.items():
            assert again[key].dtype == want.dtype and np.array_equal(again[key], want), (k, key)
