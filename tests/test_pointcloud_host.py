"""CPU: the multiclass ``PointCloud`` task without a device -- the rule of ``sc_select_classes`` (the contract in
include/spacecarve.h, restated in tests/pointcloud_oracle.py) against the reference's literal lines, the logic of
``tasks.proc3d.point_cloud_run`` with the checkers injected, and the argument errors, which are judged before any
device call (there is no device here: a call that reached one would fail with another error)."""
import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import proc3d
from plant3dvision_amd.tasks import proc3d as task
from tests import pointcloud_oracle as oracle

ORIGIN, VS = np.array([-3.0, 2.5, 10.0]), 0.75


# ---- the rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 3, 4, 5, 6])
def test_closed_form_equals_the_literal_lines(L):
    """Ties, NaN, +-inf, -0.0, negatives; the background absent / first / middle / last; the six parameter sets."""
    seen_nan = seen_none = seen_class = 0
    for q, bg in enumerate([None, 0, L // 2, L - 1]):
        for dtype in (np.float64, np.float32):
            stack = oracle.adversarial_stack((4, 3, 5), L, seed=100 * L + q, dtype=dtype, background_at=bg)
            seen_nan += int(sum(np.isnan(v).sum() for v in stack.values()))
            for params in oracle.PARAMETER_SETS:
                want, wl, wc = oracle.literal_winner(stack, *params)
                got, gl, gc = oracle.closed_form_winner(stack, *params)
                assert gl == wl and np.array_equal(got, want) and np.array_equal(gc, wc), (L, bg, params)
                seen_none += int((want == oracle.NONE).sum())
                seen_class += int((want != oracle.NONE).sum())
                if bg is not None:
                    assert wc[bg] == 0 and not (want == bg).any()
    assert seen_nan > 0 and seen_none > 0 and seen_class > 0


def test_the_rule_on_written_out_voxels():
    """One row of voxels whose winners can be worked out by hand (background first, prior 1, contrast 10, score 0.2)."""
    nan, inf = np.nan, np.inf
    #            clear a  tie a/b  bg wins  contrast fails  NaN in a  NaN in bg and b  all -inf  b over 0 and -1
    bgv = np.array([0.0, 0.0, 5.0, 0.0, 0.0, nan, -inf, -1.0])
    a = np.array([1.0, 1.0, 1.0, 1.0, nan, 3.0, -inf, 0.0])
    b = np.array([0.0, 1.0, 0.0, 0.2, 0.0, nan, -inf, 7.0])
    stack = {"background": bgv.reshape(1, 1, 8), "a": a.reshape(1, 1, 8), "b": b.reshape(1, 1, 8)}
    want = [1, 255, 255, 255, 1, 255, 255, 2]
    for fn in (oracle.literal_winner, oracle.closed_form_winner):
        winner, labels, counts = fn(stack)
        assert winner.reshape(-1).tolist() == want and labels == ["background", "a", "b"] and counts.tolist() == [0, 2, 1]
    # contrast off: every arg-max that is not the background owns its voxel, the first index at a tie, the first NaN
    winner, _, counts = oracle.literal_winner(stack, 1.0, 1.0, 0.2)
    assert winner.reshape(-1).tolist() == [1, 1, 255, 1, 1, 255, 255, 2] and counts.tolist() == [0, 4, 1]
    assert np.array_equal(oracle.closed_form_winner(stack, 1.0, 1.0, 0.2)[0], winner)


# ---- point_cloud_run --------------------------------------------------------------------------------------------
def _select(voxels, background_prior, min_contrast, min_score):
    return oracle.literal_winner(voxels, background_prior, min_contrast, min_score)


def _vol2pcd(volume, origin, voxel_size, level_set_value, index):
    return oracle.vol2pcd(np.asarray(volume) if index is None else (np.asarray(volume) == index), origin, voxel_size, level_set_value)


def _run(voxels, lsv=1.0, params=(1.0, 10.0, 0.2), **kw):
    return task.point_cloud_run(voxels, ORIGIN, VS, lsv, *params, select_fn=_select, vol2pcd_fn=_vol2pcd, **kw)


@pytest.fixture(scope="module")
def scene():
    return oracle.organ_scene((24, 20, 33), seed=7, dtype=np.float64)


@pytest.mark.parametrize("lsv,params", [(1.0, (1.0, 10.0, 0.2)), (0.0, (1.0, 1.0, 0.2)), (1.0, (0.25, 1.5, 0.2))])
def test_run_equals_the_literal_lines(scene, lsv, params):
    """Point order (class order, then C order of the shell voxels), labels and the five known colours."""
    cloud, meta = _run(scene, lsv, params)
    pts, nrm, cols, labels, per_class = oracle.literal_run(scene, ORIGIN, VS, lsv, *params, colors=task.POINT_CLOUD_COLORS)
    assert all(per_class[k] > 0 for k in oracle.ORGANS), per_class
    assert list(meta) == ["labels"] and meta["labels"] == labels and len(labels) == len(pts)
    assert [k for q, k in enumerate(labels) if q == 0 or labels[q - 1] != k] == ["stem", "leaf", "flower", "fruit"]
    assert np.array_equal(np.asarray(cloud.points), pts) and np.array_equal(np.asarray(cloud.normals), nrm)
    assert np.array_equal(np.asarray(cloud.colors), cols)
    at = 0
    _, vols = oracle.literal_class_volumes(scene, *params)
    for k in oracle.ORGANS:  # a class's points are its own cloud's: C order of the shell voxels they come from
        one = oracle.vol2pcd_oracle.vol2pcd(vols[k], ORIGIN, VS, lsv)
        assert np.array_equal(np.asarray(cloud.points)[at:at + per_class[k]], one[0])
        flat = (one[4][:, 0] * 20 + one[4][:, 1]) * 33 + one[4][:, 2]
        assert len(flat) == per_class[k] and (np.diff(flat) > 0).all(), k
        at += per_class[k]
    assert at == len(pts)


def test_reference_colours_restated():
    assert task.POINT_CLOUD_COLORS == {"stem": [1.0, 0.0, 0.0], "flower": [1.0, 1.0, 0.0], "fruit": [1.0, 0.0, 1.0],
                                       "pedicel": [1.0, 1.0, 1.0], "leaf": [0.0, 1.0, 0.0]}
    assert task.POINT_CLOUD_DEFAULTS == dict(level_set_value=1.0, background_prior=1.0, min_contrast=10.0, min_score=0.2)


def test_unknown_labels_take_injected_random_colours(scene):
    renamed = {{"leaf": "petal", "fruit": "root"}.get(k, k): v for k, v in scene.items()}
    drawn = iter([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]])
    cloud, meta = _run(renamed, random_color=lambda: next(drawn))
    drawn2 = iter([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]])
    pts, _, cols, labels, per_class = oracle.literal_run(renamed, ORIGIN, VS, colors=task.POINT_CLOUD_COLORS,
                                                         random_color=lambda: next(drawn2))
    assert meta["labels"] == labels and np.array_equal(np.asarray(cloud.colors), cols)
    got = {k: np.unique(np.asarray(cloud.colors)[np.array(labels) == k], axis=0).tolist() for k in per_class}
    assert got == {"stem": [[1.0, 0.0, 0.0]], "petal": [[0.1, 0.2, 0.3]], "flower": [[1.0, 1.0, 0.0]], "root": [[0.4, 0.5, 0.6]]}
    # colours of the caller's own; the default random colour is three numbers of [0, 1)
    cloud, _ = _run(scene, colors={"stem": [0.5, 0.5, 0.5]})
    cols = np.asarray(cloud.colors)
    assert cols.shape == (len(cloud.points), 3) and (cols >= 0).all() and (cols < 1).all()
    assert np.unique(cols[np.array(_run(scene)[1]["labels"]) == "stem"], axis=0).tolist() == [[0.5, 0.5, 0.5]]


def test_single_volume_branch(scene):
    vol = scene["stem"] > 4
    want = oracle.vol2pcd(vol, ORIGIN, VS, 1.0)
    assert len(want.points) > 0
    for voxels in (vol, {"only": vol}):
        cloud, meta = _run(voxels)
        assert meta == {"voxel_size": VS} and type(meta["voxel_size"]) is float
        assert np.array_equal(cloud.points, want.points) and np.array_equal(cloud.normals, want.normals)


def test_an_empty_class_contributes_nothing(scene):
    calls = []

    def spy(volume, origin, voxel_size, level_set_value, index):
        calls.append(index)
        return _vol2pcd(volume, origin, voxel_size, level_set_value, index)

    voxels = dict(scene)
    voxels["leaf"] = np.zeros_like(scene["leaf"])
    cloud, meta = task.point_cloud_run(voxels, ORIGIN, VS, select_fn=_select, vol2pcd_fn=spy)
    pts, nrm, cols, labels, per_class = oracle.literal_run(voxels, ORIGIN, VS, colors=task.POINT_CLOUD_COLORS)
    assert per_class["leaf"] == 0 and "leaf" not in meta["labels"] and meta["labels"] == labels
    assert np.array_equal(np.asarray(cloud.points), pts) and np.array_equal(np.asarray(cloud.colors), cols)
    assert calls == [1, 3, 4]  # the index into the keys, background first; nothing is asked of the empty class


def test_all_background_gives_an_empty_cloud(scene):
    voxels = {k: (np.full_like(v, 9.0) if k == "background" else v) for k, v in scene.items()}
    cloud, meta = _run(voxels)
    assert meta == {"labels": []}
    assert np.asarray(cloud.points).shape == (0, 3) and np.asarray(cloud.normals).shape == (0, 3) and np.asarray(cloud.colors).shape == (0, 3)


def test_point_cloud_class_takes_colours():
    p = proc3d.PointCloud(np.zeros((2, 3)), np.ones((2, 3)))
    assert p.colors is None and len(p) == 2
    assert proc3d.PointCloud(np.zeros((2, 3)), np.ones((2, 3)), np.ones((2, 3))).colors.shape == (2, 3)


# ---- argument errors: before any device call --------------------------------------------------------------------
def _raw(ptrs, L, dtype=nat.SC_EVAL_F32, background=-1, shape=(2, 2, 2), winner=True, counts=True):
    b = nat.backend()
    pp = np.array(ptrs, dtype=np.uintp)
    w, c = np.zeros(8, np.uint8), np.zeros(64, np.int64)
    rc = b.call("sc_select_classes", nat.addr(pp) if len(ptrs) else 0, dtype, L, background, shape[0], shape[1], shape[2], 1.0, 10.0,
                0.2, 0, 0, 0, nat.addr(w) if winner else 0, nat.addr(c) if counts else 0)
    return rc, b.string(b.call("sc_select_last_error"))


def test_select_classes_argument_errors_of_the_library():
    v = np.zeros(8, np.float32)
    p = nat.addr(v)
    assert _raw([p], 1) == (nat.SC_ERR_INVALID, "L must be 2..32 classes")
    assert _raw([p] * 33, 33) == (nat.SC_ERR_INVALID, "L must be 2..32 classes")
    assert _raw([], 2)[0] == nat.SC_ERR_INVALID and "null argument" in _raw([], 2)[1]
    assert _raw([p, p], 2, winner=False) == (nat.SC_ERR_INVALID, "null argument (volumes, winner, counts)")
    assert _raw([p, p], 2, counts=False) == (nat.SC_ERR_INVALID, "null argument (volumes, winner, counts)")
    assert _raw([p, 0], 2) == (nat.SC_ERR_INVALID, "null volume pointer")
    assert _raw([p, p], 2, dtype=0)[0] == nat.SC_ERR_INVALID and "dtype" in _raw([p, p], 2, dtype=0)[1]
    assert _raw([p, p], 2, background=2)[0] == nat.SC_ERR_INVALID and "background" in _raw([p, p], 2, background=2)[1]
    assert _raw([p, p], 2, shape=(2, 0, 2)) == (nat.SC_ERR_INVALID, "nx, ny and nz must be at least 1")
    assert _raw([p, p], 2, shape=(2, 2, 1 << 31))[0] == nat.SC_ERR_INVALID
    b = nat.backend()
    out, cnt, origin, gw = np.zeros(2, np.uintp), np.zeros(1, np.int64), np.zeros(3), np.ones(5)
    for cls in (-1, 256):
        rc = b.call("sc_vol2pcd_class", p, 0, cls, 2, 2, 2, nat.addr(origin), 1.0, 0.0, nat.addr(gw), 0, nat.addr(out),
                    nat.addr(out) + 8, nat.addr(cnt))
        assert rc == nat.SC_ERR_INVALID and "cls must be 0..255" in b.string(b.call("sc_vol2pcd_last_error"))
    rc = b.call("sc_vol2pcd_class", 0, 0, 1, 2, 2, 2, nat.addr(origin), 1.0, 0.0, nat.addr(gw), 0, nat.addr(out),
                nat.addr(out) + 8, nat.addr(cnt))
    assert rc == nat.SC_ERR_INVALID and b.string(b.call("sc_vol2pcd_last_error")) == "null argument"


def test_select_classes_argument_errors_of_the_binding():
    import torch
    v = np.zeros((2, 3, 4), np.float32)
    with pytest.raises(ValueError, match="at least two classes"):
        proc3d.select_classes({"a": v})
    with pytest.raises(ValueError, match="at most 32 classes"):
        proc3d.select_classes({f"c{q}": v for q in range(33)})
    with pytest.raises(ValueError, match="all NumPy arrays or all CUDA tensors"):
        proc3d.select_classes({"a": v, "b": torch.zeros(2, 3, 4)})
    with pytest.raises(ValueError, match="CUDA tensors"):
        proc3d.select_classes({"a": torch.zeros(2, 3, 4), "b": torch.zeros(2, 3, 4)})
    with pytest.raises(ValueError, match="shapes of the voxels differ"):
        proc3d.select_classes({"a": v, "b": np.zeros((2, 3, 5), np.float32)})
    with pytest.raises(ValueError, match="dtypes of the voxels differ"):
        proc3d.select_classes({"a": v, "b": v.astype(np.float64)})
    with pytest.raises(ValueError, match="3-D"):
        proc3d.select_classes({"a": v[0], "b": v[0]})
    with pytest.raises(ValueError, match="must not be empty"):
        proc3d.select_classes({"a": v[:0], "b": v[:0]})
    with pytest.raises(ValueError, match="uint8"):
        proc3d.vol2pcd_class(v, 1, [0, 0, 0], 1.0)
    with pytest.raises(ValueError, match="cls must be 0..255"):
        proc3d.vol2pcd_class(np.zeros((2, 2, 2), np.uint8), 256, [0, 0, 0], 1.0)
