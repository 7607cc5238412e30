"""CPU: the operand layer of the device units' Python wrappers (``_operands.py``), ``_native.unit_call`` and
``proc3d.release_device_buffers``.  Every refusal is compared with the whole message the wrappers raise; tensors are CPU
tensors (refused as "not CUDA") or stand-ins, so no device is touched."""
import os
import subprocess
import sys

import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import _operands as ops
from plant3dvision_amd import proc3d

RGB_SHAPE = "pictures must be [V, H, W, 3] or [H, W, 3] (RGB; RGBA and grey pictures take the reference's CPU route)"
MIXED = "volumes must be all NumPy arrays or all CUDA tensors"
F3 = (nat.SC_EVAL_F32, nat.SC_EVAL_F64, nat.SC_EVAL_U8)


def refused(message, fn, *args):
    with pytest.raises(ValueError) as info:
        fn(*args)
    assert type(info.value) is ValueError and str(info.value) == message


class Tagged(np.ndarray):
    """An ndarray subclass that happens to carry ``data_ptr``: an array all the same."""

    def data_ptr(self):
        return 0


def test_is_tensor_and_ptr_of():
    import torch
    a = np.zeros((2, 3))
    assert not ops.is_tensor(a) and not ops.is_tensor(a.view(Tagged)) and not ops.is_tensor([1, 2]) and not ops.is_tensor(None)
    t = torch.zeros(3)
    assert ops.is_tensor(t) and ops.ptr_of(t) == t.data_ptr() and ops.ptr_of(a) == a.ctypes.data
    out = ops.empty_uint8((2, 5))
    assert type(out) is np.ndarray and out.dtype == np.uint8 and out.shape == (2, 5)


def test_picture_batch():
    import torch
    for shape, vhw in [((2, 4, 5, 3), (2, 4, 5)), ((4, 5, 3), (1, 4, 5)), ((1, 1, 1, 3), (1, 1, 1))]:
        img = np.arange(int(np.prod(shape)), dtype=np.uint8).reshape(shape)
        p = ops.picture_batch(img, device=3)
        assert p.vhw == vhw and p.shape == shape and (p.on_device, p.device, p.stream, p.tdevice) == (0, 3, 0, None)
        assert p.data is img and p.ptr == img.ctypes.data
        out = ops.empty_uint8(p.shape[:-1], p.tdevice)
        assert type(out) is np.ndarray and out.dtype == np.uint8 and out.shape == shape[:-1]
    wide = np.zeros((2, 4, 5, 6), dtype=np.uint8)
    p = ops.picture_batch(wide[..., ::2])  # a view that is not contiguous: a contiguous copy, kept in the record
    assert p.data.flags["C_CONTIGUOUS"] and p.ptr == p.data.ctypes.data and p.data.shape == (2, 4, 5, 3)
    for dtype in (np.bool_, np.int8, np.uint16, np.int32, np.float32, np.float64):
        refused("pictures must be uint8 (float pictures take the reference's CPU route)", ops.picture_batch, np.zeros((4, 5, 3), dtype))
    refused("pictures must be uint8 (float pictures take the reference's CPU route)", ops.picture_batch, [[[1, 2, 3]]])  # (int64)
    for shape in [(5,), (4, 5), (4, 5, 4), (4, 5, 1), (2, 4, 5, 4), (1, 2, 4, 5, 3)]:
        refused(RGB_SHAPE, ops.picture_batch, np.zeros(shape, np.uint8))
    for t in (torch.zeros((4, 5, 3), dtype=torch.uint8), torch.zeros((4, 5, 3), dtype=torch.float32), torch.zeros((4, 5), dtype=torch.uint8)):
        refused("a tensor of pictures must be a contiguous CUDA uint8 tensor", ops.picture_batch, t)


def test_empty_picture_batches_are_refused_by_the_wrappers():
    """The operand judges an empty batch like any other; ``masks_from_images`` and ``undistort`` refuse it."""
    from plant3dvision_amd import proc2d
    for shape in [(0, 4, 5, 3), (2, 0, 5, 3), (4, 0, 3)]:
        empty = np.zeros(shape, np.uint8)
        p = ops.picture_batch(empty)
        assert p.shape == shape and 0 in p.vhw
        refused("V, H and W must be at least 1", proc2d.masks_from_images, empty)
        refused("V, H and W must be at least 1", proc2d.undistort, empty, np.eye(3), [0, 0, 0, 0])


def test_points():
    import torch
    a = np.arange(12, dtype=np.float64).reshape(4, 3)
    p = ops.points(a, "queries")
    assert p.points is a and (p.n, p.on_device) == (4, 0) and p.ptr == a.ctypes.data
    strided = np.repeat(a, 2, axis=1)[:, ::2]
    assert not strided.flags["C_CONTIGUOUS"]
    for cloud in (a.astype(np.float32), a.astype(np.int64), a.tolist(), proc3d.PointCloud(a, None), np.asfortranarray(a), strided):
        p = ops.points(cloud, "queries")
        assert p.points.dtype == np.float64 and p.points.flags["C_CONTIGUOUS"] and np.array_equal(p.points, a)
        assert p.ptr == p.points.ctypes.data and p.keep is p.points
    p = ops.points(np.ones((4, 3), dtype=np.bool_), "queries")
    assert p.points.dtype == np.float64 and p.points.tolist() == [[1.0] * 3] * 4
    for empty in (np.zeros((0, 3)), np.zeros((0,)), [], np.zeros((0, 2)), np.zeros((3, 0))):
        p = ops.points(empty, "targets")
        assert p.points.shape == (0, 3) and p.n == 0 and p.keep.shape == (1, 3) and p.ptr == p.keep.ctypes.data != 0
        assert not p.keep.any()
    for bad in (np.zeros((3, 2)), np.zeros(6), np.zeros((2, 3, 3)), np.zeros((3, 4))):
        refused("queries must be [n, 3]", ops.points, bad, "queries")
        refused("points must be [P, 3]", ops.points, bad, "points", "[P, 3]")
    for t in (torch.zeros((3, 3), dtype=torch.float64), torch.zeros((3, 3), dtype=torch.float32), torch.zeros(3, dtype=torch.float64)):
        refused("device targets must be a contiguous float64 CUDA tensor [n, 3]", ops.points, t, "targets")
        refused("device points must be a contiguous float64 CUDA tensor [P, 3]", ops.points, t, "points", "[P, 3]")
        refused("device points must be a contiguous float64 CUDA tensor [P, 3]", ops.points, proc3d.PointCloud(t, None), "points", "[P, 3]")


def test_ids():
    import torch
    a = np.array([3, 1, 2], dtype=np.int32)
    r = ops.ids(a, "index")
    assert np.shares_memory(r.data, a) and (r.n, r.on_device, r.tdevice, r.ptr) == (3, 0, None, a.ctypes.data)
    for other in (a.astype(np.int64), a.astype(np.uint8), [3, 1, 2], a.reshape(3, 1), np.repeat(a, 2)[::2], a.astype(np.float64)):
        r = ops.ids(other, "index")
        assert r.data.dtype == np.int32 and r.data.flags["C_CONTIGUOUS"] and r.data.tolist() == [3, 1, 2] and r.ptr == r.data.ctypes.data
    assert ops.ids(np.array([True, False]), "index").data.tolist() == [1, 0]
    r = ops.ids(np.zeros(0, np.int32), "index")
    assert (r.n, r.ptr) == (0, 0)
    for t, what in ((torch.zeros(3, dtype=torch.int32), "index"), (torch.zeros(3, dtype=torch.int64), "query_labels"),
                    (torch.zeros((3, 1), dtype=torch.int32), "target_labels")):
        refused(f"device {what} must be a contiguous int32 CUDA tensor [n]", ops.ids, t, what)


def test_same():
    assert ops.same([(3, 4)] * 3, "shapes of the voxels") == (3, 4) and ops.same([None, None], "devices") is None
    refused("the shapes of the voxels differ: ['(3, 4, 5)', '(3, 4, 6)']", ops.same, [(3, 4, 6), (3, 4, 5), (3, 4, 6)], "shapes of the voxels")
    refused("the dtypes of the ground truths differ: ['float64', 'uint8']", ops.same, [np.dtype(np.uint8), np.dtype(np.float64)],
            "dtypes of the ground truths")


@pytest.mark.parametrize("dtype,accept,want,code", [
    (np.float32, F3, np.float32, nat.SC_EVAL_F32), (np.float64, F3, np.float64, nat.SC_EVAL_F64), (np.uint8, F3, np.uint8, nat.SC_EVAL_U8),
    (np.bool_, F3, np.uint8, nat.SC_EVAL_U8), (np.int32, F3, np.float64, nat.SC_EVAL_F64), (np.float16, F3, np.float64, nat.SC_EVAL_F64),
    (np.int8, F3, np.float64, nat.SC_EVAL_F64), (np.uint16, F3, np.float64, nat.SC_EVAL_F64),
    (np.float32, F3[:2], np.float32, nat.SC_EVAL_F32), (np.float64, F3[:2], np.float64, nat.SC_EVAL_F64),
    (np.uint8, F3[:2], np.float64, nat.SC_EVAL_F64), (np.bool_, F3[:2], np.float64, nat.SC_EVAL_F64),
    (np.int64, F3[:2], np.float64, nat.SC_EVAL_F64)])
def test_class_stack_dtypes(dtype, accept, want, code):
    """Accepted dtypes are read in place, bool is viewed as uint8 where uint8 is accepted, the rest becomes float64."""
    vols = [(np.arange(24).reshape(2, 3, 4) % 2 + k).astype(dtype) for k in range(3)]
    s = ops.class_stack(vols, "voxels", accept, "never", device=2)
    assert (s.shape, s.code, s.on_device, s.tdevice, s.device, s.stream) == ((2, 3, 4), code, 0, None, 2, 0)
    assert s.table.dtype == np.uintp and s.table.tolist() == [v.ctypes.data for v in s.vols]
    for kept, given in zip(s.vols, vols):
        assert kept.dtype == want and kept.flags["C_CONTIGUOUS"] and np.array_equal(kept, given.astype(want))
        same_memory = np.dtype(dtype) == want or (dtype is np.bool_ and want is np.uint8)
        assert np.shares_memory(kept, given) == same_memory


def test_class_stack_views_and_refusals():
    import torch
    big = np.arange(2 * 3 * 8, dtype=np.float32).reshape(2, 3, 8)
    vols = [big[:, :, ::2], big[:, :, 1::2]]  # views that are not contiguous: contiguous copies, kept in the record
    s = ops.class_stack(vols, "voxels", F3, "never")
    assert all(k.flags["C_CONTIGUOUS"] and np.array_equal(k, v) for k, v in zip(s.vols, vols))
    assert s.table.tolist() == [k.ctypes.data for k in s.vols] and (s.device, s.code) == (0, nat.SC_EVAL_F32)
    s = ops.class_stack([[[[1.0, 2.0]]], [[[3.0, 4.0]]]], "voxels", F3, "never")  # array-likes
    assert s.shape == (1, 1, 2) and s.code == nat.SC_EVAL_F64
    for shape in [(0, 3, 4), (2, 0, 4), (2, 3, 0)]:  # an empty stack is judged: the wrappers refuse it in their own turn
        assert ops.class_stack([np.zeros(shape, np.float32)] * 2, "voxels", F3, "never").shape == shape
    z = np.zeros((2, 3, 4), np.float32)
    refused("the shapes of the voxels differ: ['(2, 3, 4)', '(2, 3, 5)']", ops.class_stack, [z, np.zeros((2, 3, 5), np.float32)],
            "voxels", F3, "never")
    refused("the shapes of the ground truths differ: ['(2, 3, 4)', '(3, 4)']", ops.class_stack, [z, z[0]], "ground truths", F3, "never")
    refused("the dtypes of the voxels differ: ['float32', 'float64']", ops.class_stack, [z, z.astype(np.float64)], "voxels", F3, "never")
    refused("the dtypes of the ground truths differ: ['bool', 'uint8']", ops.class_stack, [z.astype(np.uint8), z.astype(np.bool_)],
            "ground truths", F3, "never")
    for shape in [(4,), (3, 4), (1, 2, 3, 4)]:
        refused("volumes must be 3-D", ops.class_stack, [np.zeros(shape, np.float32)] * 2, "voxels", F3, "never")
    t = torch.zeros((2, 3, 4), dtype=torch.float32)
    refused(MIXED, ops.class_stack, [z, t], "voxels", F3, "never")
    refused(MIXED, ops.class_stack, [t, z, t], "ground truths", F3, "never")
    refused("device volumes must be contiguous 3-D CUDA tensors", ops.class_stack, [t, t], "voxels", F3, "never")


class FakeDeviceVolume:
    """Passes for a contiguous CUDA tensor as far as ``class_stack`` looks before it asks torch for the stream."""
    is_cuda = True

    def __init__(self, dtype, shape=(2, 3, 4), device="cuda:0"):
        self.dtype, self.shape, self.device = dtype, shape, device

    def data_ptr(self): return 0
    def is_contiguous(self): return True
    def dim(self): return len(self.shape)


def test_class_stack_device_refusals():
    import torch
    f32 = FakeDeviceVolume(torch.float32)
    refused("the devices differ: ['cuda:0', 'cuda:1']", ops.class_stack, [f32, FakeDeviceVolume(torch.float32, device="cuda:1")],
            "voxels", F3, "no")
    refused("the shapes of the ground truths differ: ['(2, 3, 4)', '(2, 3, 5)']", ops.class_stack,
            [f32, FakeDeviceVolume(torch.float32, (2, 3, 5))], "ground truths", F3, "no")
    refused("the dtypes of the voxels differ: ['torch.float32', 'torch.float64']", ops.class_stack, [f32, FakeDeviceVolume(torch.float64)],
            "voxels", F3, "no")
    refused("device volumes must be contiguous 3-D CUDA tensors", ops.class_stack, [f32, FakeDeviceVolume(torch.float32, (3, 4))],
            "voxels", F3, "no")
    select = "device volumes must be float32, float64, uint8 or bool"
    evaluate = "device voxels must be float32 or float64, device ground truths float32, float64, uint8 or bool"
    for dt in (torch.int32, torch.float16, torch.int8, torch.int64):
        refused(select, ops.class_stack, [FakeDeviceVolume(dt)] * 2, "voxels", F3, select)
    for dt in (torch.uint8, torch.bool, torch.int32):  # where uint8 is not accepted, bool is not either
        refused(evaluate, ops.class_stack, [FakeDeviceVolume(dt)] * 2, "voxels", F3[:2], evaluate)


def test_the_wrappers_compare_two_stacks(monkeypatch):
    """``voxel_confusion`` judges its two stacks against each other: kind, device and size, in the wrappers' words."""
    import torch
    from plant3dvision_amd import metrics
    v = {k: np.zeros((3, 4, 5), np.float32) for k in ("background", "leaf")}
    t = {k: torch.zeros((3, 4, 5), dtype=torch.float32) for k in v}
    refused(MIXED, metrics.voxel_confusion, t, v)  # (kinds are compared across both stacks before either is judged)
    refused(MIXED, metrics.voxel_confusion, dict(v, leaf=np.zeros((3, 4, 6), np.float32)), t)
    refused("device volumes must be contiguous 3-D CUDA tensors", metrics.voxel_confusion, t, t)  # (CPU tensors)
    monkeypatch.setattr(ops, "tensor_place", lambda tensor: (0, 0))  # (the stand-ins have no stream to ask for)
    fake = {k: FakeDeviceVolume(torch.float32, (3, 4, 5)) for k in v}
    refused(MIXED, metrics.voxel_confusion, v, fake)
    refused(MIXED, metrics.voxel_confusion, fake, v)
    refused("the devices differ: ['cuda:0', 'cuda:1']", metrics.voxel_confusion, fake,
            {k: FakeDeviceVolume(torch.float32, (3, 4, 5), "cuda:1") for k in v})
    refused("ground truth (3, 4, 4) smaller than the prediction (3, 4, 5)", metrics.voxel_confusion, v,
            {k: np.zeros((3, 4, 4), np.uint8) for k in v})
    refused("volumes must not be empty", metrics.voxel_confusion, {k: np.zeros((3, 0, 5), np.float32) for k in v},
            {k: np.zeros((3, 0, 5), np.uint8) for k in v})
    refused("volumes must not be empty", proc3d.select_classes, {k: np.zeros((3, 0, 5), np.float32) for k in v})


class _StubBackend:
    """Answers every entry point with a code and every error getter with its own name: no library call."""

    def __init__(self, rc=nat.SC_OK):
        self.rc, self.asked = rc, []

    def call(self, name, *args):
        self.asked.append((name,) + args)
        return f"text of {name}".encode() if name.endswith("_last_error") else self.rc

    @staticmethod
    def string(ret):
        return ret.decode()


UNITS = {"sc_vol2pcd": "vol2pcd", "sc_vol2pcd_packed": "vol2pcd", "sc_vol2pcd_class": "vol2pcd", "sc_label_points": "label_points",
         "sc_masks_from_rgb": "masks", "sc_undistort_rgb": "undistort", "sc_dbscan": "dbscan", "sc_eval_masks": "eval",
         "sc_eval_voxels": "eval", "sc_select_classes": "select", "sc_nearest": "nearest", "sc_nearest_confusion": "nearest"}


def test_the_table_lists_every_unit_entry():
    assert {e: f"sc_{u}_last_error" for e, u in UNITS.items()} == nat.UNIT_ERRORS
    assert all(e in nat.EXPORTED_SYMBOLS and g in nat.EXPORTED_SYMBOLS for e, g in nat.UNIT_ERRORS.items())
    units = {g for g in nat.EXPORTED_SYMBOLS if g.endswith("_last_error")} - {"sc_last_error", "sc_png_last_error"}
    assert units == set(nat.UNIT_ERRORS.values())  # no unit's getter is left without an entry


@pytest.mark.parametrize("entry", sorted(UNITS))
def test_unit_call_asks_the_units_own_getter(monkeypatch, entry):
    getter = f"sc_{UNITS[entry]}_last_error"
    stub = _StubBackend()
    monkeypatch.setattr(nat, "_backend", stub)
    assert nat.unit_call(entry, 1, 2.5, 3) is None and stub.asked == [(entry, 1, 2.5, 3)]  # the arguments go through as they are
    for rc, exc in [(nat.SC_ERR_INVALID, ValueError), (nat.SC_ERR_NOMEM, MemoryError), (nat.SC_ERR_DEVICE, nat.SpaceCarveError)]:
        stub.rc, stub.asked = rc, []
        with pytest.raises(exc) as info:
            nat.unit_call(entry, 7)
        assert type(info.value) is exc and str(info.value) == f"{entry}: text of {getter} (code {rc})"
        assert stub.asked == [(entry, 7), (getter,)]
        with pytest.raises(exc) as info:
            nat.unit_call(entry, what="sc_other_name")
        assert str(info.value) == f"sc_other_name: text of {getter} (code {rc})"


@pytest.mark.parametrize("entry", ["sc_get_values", "sc_vol2pcd_release", "sc_last_error", "sc_no_such_entry", ""])
def test_unit_call_refuses_an_unknown_entry(monkeypatch, entry):
    stub = _StubBackend(nat.SC_ERR_INVALID)
    monkeypatch.setattr(nat, "_backend", stub)
    with pytest.raises(KeyError):
        nat.unit_call(entry)
    assert stub.asked == []  # nothing was called, and no other unit's message was fetched


def test_release_device_buffers_calls_the_five_releases_in_order(monkeypatch):
    stub = _StubBackend()
    monkeypatch.setattr(nat, "_backend", stub)
    proc3d.release_device_buffers()
    assert stub.asked == [("sc_vol2pcd_release",), ("sc_dbscan_release",), ("sc_eval_release",), ("sc_select_release",),
                          ("sc_nearest_release",)]


def test_host_operands_do_not_import_torch():
    code = ("import sys, numpy as np\n"
            "from plant3dvision_amd import _operands as ops, proc3d\n"
            "ops.empty_uint8((2, 2), ops.picture_batch(np.zeros((2, 2, 3), np.uint8)).tdevice)\n"
            "ops.points(np.zeros((2, 3)), 'queries')\n"
            "ops.ids([1, 2], 'index'); ops.class_stack([np.zeros((1, 1, 1))] * 2, 'voxels', (2,), 'no')\n"
            "assert not ops.is_tensor(np.zeros(1)) and 'torch' not in sys.modules\n")
    subprocess.run([sys.executable, "-c", code], check=True, timeout=60, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
