"""No GPU: the checker of ``sc_graph_connect`` (tests/connect_oracle.py) against the brute force over all pairs
(tests/graph_oracle.py), and what ``proc3d.connect_edges`` and the library refuse and do without a device."""
import os
import re

import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import proc3d
from tests import connect_oracle as checker
from tests import graph_oracle as oracle


def _clouds():
    rng = np.random.default_rng(22)
    lattice = 2.0 * rng.integers(0, 9, size=(130, 3)).astype(np.float64)  # duplicates among them; neighbours are 2 apart
    sparse = 2.0 * rng.integers(0, 9, size=(65, 3)).astype(np.float64)
    uniform = rng.uniform(0.0, 1.0, size=(129, 3))
    out = {}
    for name, pts, radius, ties in (("lattice 130", lattice, 1.0, 10), ("uniform 129", uniform, 0.08, 0), ("lattice 65", sparse, 1.0, 10)):
        labels, count = checker.components_within(pts, radius)
        out[name] = (pts, labels, count, ties)
    return out


CLOUDS = _clouds()


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_checker_equals_the_brute_force(name):
    pts, labels, count, ties = CLOUDS[name]
    n = len(pts)
    assert count >= 20  # an input that is not easy: many rounds
    if name == "lattice 65":
        assert count >= n - 8  # nearly all singletons
    for root in (0, n - 1, n // 2):
        want_e, want_w = oracle.connect_edges(pts, labels, root)
        got_e, got_w = checker.connect_edges(pts, labels, root)
        assert got_e.dtype == np.int32 and got_e.shape == (count - 1, 2) and got_w.dtype == np.float64
        assert np.array_equal(got_e, want_e) and np.array_equal(got_w, want_w)
        assert len(want_w) - len(np.unique(want_w)) >= ties  # on the lattices the key's i and j decide


def test_checker_takes_any_labelling():
    pts = CLOUDS["uniform 129"][0]
    labels = np.arange(len(pts)) % 7  # interleaved, not components
    for root in (0, 128):
        want = oracle.connect_edges(pts, labels, root)
        got = checker.connect_edges(pts, labels, root)
        assert len(got[0]) == 6 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- the library's refusals (rule C3): host arrays are judged before any device call ---------------------------------
def test_argument_errors_of_the_library_need_no_device():
    b = nat.backend()
    pts = np.ascontiguousarray(np.arange(12.0).reshape(4, 3))
    lab = np.array([0, 1, 1, 2], dtype=np.int32)
    edges, weights, count = np.zeros((3, 2), np.int32), np.zeros(3), np.full(1, 7, np.int64)

    def connect(N=4, pts=pts, lab=lab, L=3, root=0, device=0, edges=nat.addr(edges), weights=nat.addr(weights), count=nat.addr(count)):
        return b.call("sc_graph_connect", N, 0 if pts is None else nat.addr(pts), 0 if lab is None else nat.addr(lab), L, root, 0, device,
                      edges, weights, count, 0)

    def refused(rc, text):
        assert rc == nat.SC_ERR_INVALID and text in b.string(b.call("sc_graph_error")), b.string(b.call("sc_graph_error"))

    refused(connect(N=-1), "N must be")
    refused(connect(N=2 ** 31), "N must be")
    refused(connect(L=0), "L must be 1 .. N")
    refused(connect(L=5), "L must be 1 .. N")
    refused(connect(lab=np.array([0, 1, 3, 2], np.int32)), "label outside")
    refused(connect(lab=np.array([0, -1, 1, 2], np.int32)), "label outside")
    refused(connect(root=4), "root")
    refused(connect(root=-1), "root")
    for bad in (np.nan, np.inf, -np.inf):
        broken = pts.copy()
        broken[2, 1] = bad
        refused(connect(pts=broken), "non-finite coordinate in point 2")
    refused(connect(pts=None), "null")
    refused(connect(lab=None), "null")
    refused(connect(count=0), "null")
    refused(connect(edges=0), "null")
    refused(connect(weights=0), "null")
    refused(connect(device=64), "device ordinal")
    refused(connect(device=-1), "device ordinal")
    assert connect(N=0, pts=None, lab=None, L=0, edges=0, weights=0) == nat.SC_OK and count[0] == 0  # no nodes: no device call


def test_header_and_symbol():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spacecarve.h")).read()
    assert "sc_graph_connect" in nat.EXPORTED_SYMBOLS and re.search(r"int sc_graph_connect\(", text)
    for rule in ("C1.", "C2.", "C3.", "C4.", "C5."):
        assert rule in text
    assert "sc_graph_connect" not in nat.UNIT_ERRORS  # read with sc_graph_error, as the unit's other entries are


# ---- the wrapper -----------------------------------------------------------------------------------------------------
class _Stub:
    def __init__(self):
        self.asked = []

    def call(self, name, *args):
        self.asked.append((name,) + args)
        return nat.SC_OK

    @staticmethod
    def string(ret):
        return ""


def _fake_tensors(device_a="cuda:0", device_b="cuda:0", n_labels=3):
    import torch

    class FakePoints:  # passes for a device tensor as far as the kind checks look
        dtype, is_cuda, shape, device = torch.float64, True, (3, 3), device_a
        def data_ptr(self): return 0
        def is_contiguous(self): return True
        def dim(self): return 2

    class FakeLabels:
        dtype, is_cuda, shape, device = torch.int32, True, (n_labels,), device_b
        def data_ptr(self): return 0
        def is_contiguous(self): return True
        def dim(self): return 1
        def numel(self): return n_labels
        def __len__(self): return n_labels

    return FakePoints(), FakeLabels()


def test_python_refusals():
    import torch
    pts = np.zeros((3, 3))
    with pytest.raises(ValueError, match="one label per point"):
        proc3d.connect_edges(pts, np.zeros(2, np.int32), 0)
    for root in (-1, 3, 10 ** 12):
        with pytest.raises(ValueError, match="root_index must be 0 .. 2"):
            proc3d.connect_edges(pts, [0, 1, 2], root)
    fake_p, fake_l = _fake_tensors()
    with pytest.raises(ValueError, match="both arrays"):  # mixed kinds
        proc3d.connect_edges(pts, fake_l, 0)
    with pytest.raises(ValueError, match="both arrays"):
        proc3d.connect_edges(fake_p, [0, 1, 2], 0)
    with pytest.raises(ValueError, match="CUDA tensor"):  # CPU tensors are refused as device operands
        proc3d.connect_edges(torch.zeros((3, 3), dtype=torch.float64), torch.zeros(3, dtype=torch.int32), 0)
    with pytest.raises(ValueError, match="int32 CUDA tensor"):
        fake_l.dtype = torch.int64
        proc3d.connect_edges(fake_p, fake_l, 0)
    with pytest.raises(ValueError, match="one label per point"):
        proc3d.connect_edges(*_fake_tensors(n_labels=2), 0)
    with pytest.raises(ValueError, match="on one device"):
        proc3d.connect_edges(*_fake_tensors("cuda:0", "cuda:1"), 0)


def test_the_call_the_wrapper_makes(monkeypatch):
    """The arguments in the header's order; no native call where there is nothing to connect."""
    stub = _Stub()
    monkeypatch.setattr(nat, "_backend", stub)
    pts = np.arange(12.0).reshape(4, 3)
    edges, weights = proc3d.connect_edges(pts, [5, 5, 9, 7], 2, device=3)
    (name, N, points, labels, L, root, on_device, device, e_ptr, w_ptr, count, stream), = stub.asked
    assert (name, N, L, root, on_device, device, stream) == ("sc_graph_connect", 4, 3, 2, 0, 3, 0)
    assert points and labels and e_ptr and w_ptr and count
    assert edges.shape == (0, 2) and edges.dtype == np.int32 and weights.shape == (0,)  # the stub reports no edge
    stub.asked = []
    for args in ((np.zeros((0, 3)), np.zeros(0, np.int32), 0), (pts, [4, 4, 4, 4], 1), (pts, np.full(4, -3), 3)):
        edges, weights = proc3d.connect_edges(*args)
        assert edges.shape == (0, 2) and edges.dtype == np.int32 and weights.shape == (0,) and weights.dtype == np.float64
    import torch
    fake_p, fake_l = _fake_tensors(torch.device("cpu"), torch.device("cpu"))  # (so that the empty results can be made here)
    for n_labels in (0, 1):  # tensors: the bound says there is one label at most
        edges, weights = proc3d.connect_edges(fake_p, fake_l, 0, n_labels=n_labels)
        assert tuple(edges.shape) == (0, 2) and edges.dtype == torch.int32 and tuple(weights.shape) == (0,) and weights.dtype == torch.float64
    assert stub.asked == []


def test_host_labels_are_compacted(monkeypatch):
    """Negative values, large values and gaps become ``0 .. L - 1`` in rising order of the values."""
    seen = {}

    class Reading(_Stub):
        def call(self, name, *args):
            import ctypes
            seen["labels"] = np.ctypeslib.as_array(ctypes.cast(args[2], ctypes.POINTER(ctypes.c_int32)), shape=(args[0],)).copy()
            seen["L"] = args[3]
            return nat.SC_OK

    monkeypatch.setattr(nat, "_backend", Reading())
    pts = np.arange(18.0).reshape(6, 3)
    proc3d.connect_edges(pts, np.array([2 ** 40, -7, 12, -7, 2 ** 40, 3]), 0)
    assert seen["labels"].tolist() == [3, 0, 2, 0, 3, 1] and seen["L"] == 4


def test_errors_are_read_with_the_units_getter(monkeypatch):
    class Refusing(_Stub):
        def call(self, name, *args):
            self.asked.append(name)
            return b"text" if name == "sc_graph_error" else nat.SC_ERR_INVALID

        @staticmethod
        def string(ret):
            return ret.decode()

    stub = Refusing()
    monkeypatch.setattr(nat, "_backend", stub)
    with pytest.raises(ValueError, match="sc_graph_connect: text"):
        proc3d.connect_edges(np.arange(9.0).reshape(3, 3), [0, 1, 2], 0)
    assert stub.asked == ["sc_graph_connect", "sc_graph_error"]


def test_no_cpu_fallback_without_device():
    try:
        n = nat.device_count()
    except nat.SpaceCarveError:
        n = 0
    if n > 0:  # with a device the call computes (tests/test_connect_gpu.py); nothing to show here
        return
    with pytest.raises(nat.SpaceCarveError):
        proc3d.connect_edges(np.arange(9.0).reshape(3, 3), [0, 1, 2], 0)
