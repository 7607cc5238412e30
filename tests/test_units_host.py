"""CPU: what the four stand-alone units (vol2pcd, label_points, masks_rgb, dbscan) share on the host side
(csrc/sc_unit.h, ``_native.check``, ``_native.build``).  The argument errors used here are judged before any device call.

No entry point can produce a message of more than 255 bytes (the longest are ``snprintf`` into 160 and 200 bytes), so
the truncation of ``UnitError::fail`` has no test."""
import importlib.util
import os
import shutil

import numpy as np
import pytest

from plant3dvision_amd import _native as nat


def _getter(name):
    b = nat.backend()
    return b.string(b.call(name))


def test_the_four_error_getters_are_independent():
    b = nat.backend()
    vol_before, lab_before = _getter("sc_vol2pcd_last_error"), _getter("sc_label_points_last_error")
    img, coefs, out = np.zeros((2, 2, 3), np.uint8), np.array([0.0, 1.0, 0.0]), np.zeros(16, np.uint8)
    rc = b.call("sc_masks_from_rgb", nat.addr(img), 0, 0, 2, 2, 0, nat.addr(coefs), 0.3, 0, 0, 0, 0, nat.addr(out), 0, 0)
    assert rc == nat.SC_ERR_INVALID and "V, H and W" in _getter("sc_masks_last_error")
    pts, lab = np.zeros((4, 3)), np.zeros(4, np.int32)
    rc = b.call("sc_dbscan", nat.addr(pts), 0, 4, -1.0, 5, 0, nat.addr(lab), 0, 0, 0)
    assert rc == nat.SC_ERR_INVALID and "eps must be finite" in _getter("sc_dbscan_last_error")
    assert "V, H and W" in _getter("sc_masks_last_error")  # still the masks unit's own
    assert _getter("sc_vol2pcd_last_error") == vol_before and _getter("sc_label_points_last_error") == lab_before
    # and the other two, the other way round
    rc = b.call("sc_label_points", 0, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0)
    assert rc == nat.SC_ERR_INVALID and "null argument" in _getter("sc_label_points_last_error")
    rc = b.call("sc_vol2pcd", 0, 0, 0, 4, 4, 4, 0, 1.0, 0.0, 0, 0, 0, 0, 0)
    assert rc == nat.SC_ERR_INVALID and _getter("sc_vol2pcd_last_error") == "null argument"
    assert "V, H and W" in _getter("sc_masks_last_error") and "eps must be finite" in _getter("sc_dbscan_last_error")


class _StubBackend:
    """Answers every error getter with its own name: no library call."""

    def __init__(self):
        self.asked = []

    def call(self, name, *args):
        self.asked.append(name)
        return f"text of {name}".encode()

    @staticmethod
    def string(ret):
        return ret.decode()


@pytest.mark.parametrize("getter", ["sc_vol2pcd_last_error", "sc_label_points_last_error", "sc_masks_last_error",
                                    "sc_dbscan_last_error", None])
def test_check_with_a_named_getter(monkeypatch, getter):
    stub = _StubBackend()
    monkeypatch.setattr(nat, "_backend", stub)
    args = ("sc_call",) if getter is None else ("sc_call", getter)
    name = getter or "sc_last_error"
    assert nat.check(nat.SC_OK, *args) is None and stub.asked == []
    for rc, exc in [(nat.SC_ERR_INVALID, ValueError), (nat.SC_ERR_NOMEM, MemoryError), (nat.SC_ERR_DEVICE, nat.SpaceCarveError)]:
        with pytest.raises(exc) as info:
            nat.check(rc, *args)
        assert type(info.value) is exc and str(info.value) == f"sc_call: text of {name} (code {rc})"
    assert (nat.SC_ERR_INVALID, nat.SC_ERR_DEVICE, nat.SC_ERR_NOMEM) == (-1, -2, -3)
    assert stub.asked == [name] * 3


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc is absent")
def test_build_follows_the_makefile(tmp_path):
    """``build(force=False)`` rebuilds the library after the units' shared header was touched, and not a second time.
    In a copy of the sources (the library, when it is there, with its time): the tree's own files stay as they are."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(nat.__file__)))
    pkg = os.path.basename(os.path.dirname(os.path.abspath(nat.__file__)))
    shutil.copytree(os.path.join(root, "include"), tmp_path / "include")
    os.mkdir(tmp_path / pkg)
    shutil.copytree(os.path.join(root, pkg, "csrc"), tmp_path / pkg / "csrc")
    shutil.copy2(os.path.join(root, pkg, "_native.py"), tmp_path / pkg / "_native.py")
    lib = tmp_path / pkg / "libspacecarve.so"
    if os.path.exists(os.path.join(root, pkg, "libspacecarve.so")):
        shutil.copy2(os.path.join(root, pkg, "libspacecarve.so"), lib)
    spec = importlib.util.spec_from_file_location("native_copy", tmp_path / pkg / "_native.py")
    copy = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(copy)
    if os.environ.get("SPACECARVE_LIB"):
        copy.LIB_PATH = str(lib)
    assert copy.LIB_PATH == str(lib)
    copy.build()  # up to date now, whatever it was
    before = os.stat(lib).st_mtime_ns
    assert copy.build() == str(lib) and os.stat(lib).st_mtime_ns == before
    header = tmp_path / pkg / "csrc" / "sc_unit.h"
    os.utime(header, ns=(before + 1_000_000_000, before + 1_000_000_000))  # "touched" after the library was built
    copy.build()
    after = os.stat(lib).st_mtime_ns
    assert after > before + 1_000_000_000  # (a build takes far longer than that second)
    copy.build()
    assert os.stat(lib).st_mtime_ns == after
