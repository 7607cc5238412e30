"""SegmentedPointCloud's point scoring: GPU vs the reference's NumPy loop."""
import numpy as np
import pytest

from plant3dvision_amd import proc3d, scenes


def reference_scores(pts, cameras, masks):
    """tasks/proc3d.py:203-232, per-point loop vectorised, same arithmetic (NumPy matmul)."""
    L, V, H, W = masks.shape
    scores = np.zeros((L, len(pts)))
    for v, cam in enumerate(cameras):
        rot, tvec = np.array(cam["rotmat"]), np.array(cam["tvec"])
        k = cam["camera_model"]["params"]
        K = np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]])
        with np.errstate(all="ignore"):
            px = np.asarray(proc3d.backproject_points(pts, K, rot, tvec) + 0.5, dtype=int)
        ok = (px[:, 0] >= 0) & (px[:, 0] < W) & (px[:, 1] >= 0) & (px[:, 1] < H)
        for l in range(L):
            scores[l, ok] += masks[l, v][px[ok, 1], px[ok, 0]]
    return np.argmax(scores, axis=0).flatten(), scores


def test_backproject_points_matches_kernel_convention():
    # pixel = K (R p + t) / z ; identity pose, point on the axis -> principal point
    K = np.array([[100.0, 0, 50], [0, 100, 40], [0, 0, 1]])
    px = proc3d.backproject_points(np.array([[0.0, 0, 2], [1, 0, 2]]), K, np.eye(3), np.zeros(3))
    assert px.tolist() == [[50.0, 40.0], [100.0, 40.0]]


@pytest.mark.gpu
def test_label_points_matches_reference_loop(gpu_device):
    shape, origin, vs, views = scenes.make_scene(32, 7, "plant", width=160, height=120, fx=130.0, fy=125.0,
                                                 cx=80.0, cy=60.0)
    cams = [scenes.camera_dict(K, R, t) for K, R, t, _ in views]
    rng = np.random.default_rng(0)
    centre = np.array(origin) + (np.array(shape) - 1) * vs / 2
    pts = centre + rng.normal(size=(5000, 3)) * np.array(shape) * vs * 0.6  # some fall outside the images
    pts[:5] = [np.array([1e30, 0, 0]), centre, centre + 1e-9, np.array([np.nan, 0, 0]), -centre * 1e6]
    masks = rng.integers(0, 256, (3, len(views), 120, 160), dtype=np.uint8)
    labels, scores = proc3d.label_points(pts, cams, masks)
    want_l, want_s = reference_scores(pts, cams, masks)
    assert np.array_equal(scores, want_s)
    assert np.array_equal(labels, want_l)
    assert scores.max() > 0 and (scores.sum(axis=0) == 0).any()


@pytest.mark.gpu
def test_label_points_with_device_masks(gpu_device):
    import torch
    shape, origin, vs, views = scenes.make_scene(24, 4, "plant", width=96, height=80, fx=80.0, fy=80.0, cx=48.0, cy=40.0)
    cams = [scenes.camera_dict(K, R, t) for K, R, t, _ in views]
    rng = np.random.default_rng(1)
    centre = np.array(origin) + (np.array(shape) - 1) * vs / 2
    pts = centre + rng.normal(size=(2000, 3)) * 3.0
    masks = rng.integers(0, 256, (2, len(views), 80, 96), dtype=np.uint8)
    a = proc3d.label_points(pts, cams, masks)
    b = proc3d.label_points(pts, cams, torch.from_numpy(masks).cuda())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- exact pixel boundaries, arg-max ties, sizes ----

_W, _H, _F, _CX, _CY = 16, 8, 64.0, 8.0, 4.0
_EPS = 2.0 ** -30
_CAM = {"camera_model": {"params": [_F, _F, _CX, _CY]}, "rotmat": np.eye(3).tolist(), "tvec": [0.0, 0.0, 0.0]}


def _targets(n):
    """Values of `pixel coordinate + 0.5` on and beside every boundary of the truncation `int(x + 0.5)`."""
    return [-1.0, -1.0 + _EPS, -0.5, -_EPS, 0.0, 0.5, 1.0 - _EPS, 1.0, n - _EPS, float(n), n + 0.5]


def _boundary_case():
    """One camera looking down +z from the origin with power-of-two intrinsics, and for every pair of targets
    (uf, vf) and every depth z in {0.5, 1, 2, -1} the point whose `pixel + 0.5` is exactly (uf, vf):
    x = z (uf - 0.5 - cx) / 64 is exact, and so is every product, sum and quotient on the way back, in any order of
    summation -- BLAS, NumPy and the kernel must agree whatever the machine.  The masks name the pixel:
    masks[0][y][x] = 1 + y W + x, masks[1] = 255 - masks[0].  Expected by the rule written out here: the pixel is the
    target truncated toward zero (so a target in (-1, 0) is pixel 0), inside iff 0 <= pixel < N; a point behind the
    camera (z = -1) counts like any other, as in the reference.  Then points in the camera's plane (z = 0: inf or NaN,
    outside) and the camera centre itself."""
    pts, want = [], []
    for z in (0.5, 1.0, 2.0, -1.0):
        for uf in _targets(_W):
            for vf in _targets(_H):
                pts.append([z * (uf - 0.5 - _CX) / _F, z * (vf - 0.5 - _CY) / _F, z])
                pu, pv = int(uf), int(vf)  # int(): toward zero
                inside = 0 <= pu < _W and 0 <= pv < _H
                want.append(1 + pv * _W + pu if inside else 0)
    for p in ([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.125, -0.25, 0.0], [-0.5, 0.5, 0.0]):
        pts.append(p)
        want.append(0)
    pts, want = np.array(pts), np.array(want, dtype=np.float64)
    m0 = (1 + np.arange(_H * _W, dtype=np.int64)).reshape(_H, _W)
    masks = np.stack([m0, 255 - m0]).astype(np.uint8)[:, None]
    scores = np.stack([want, np.where(want > 0, 255 - want, 0)])
    labels = ((want > 0) & (want < 128)).astype(np.int64)  # masks[1] > masks[0] but at the last pixel: 127 < 128
    return pts, masks, scores, labels


def test_boundary_points_are_exact_and_the_reference_follows_the_rule():
    pts, masks, scores, labels = _boundary_case()
    # exact: the projection gives back the target, to the bit
    k = _CAM["camera_model"]["params"]
    K = np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]])
    back = proc3d.backproject_points(pts[:4 * 121], K, np.eye(3), np.zeros(3)) + 0.5
    want = np.array([[uf, vf] for _ in range(4) for uf in _targets(_W) for vf in _targets(_H)])
    assert np.array_equal(back, want)
    assert len(np.unique(masks[0])) == _H * _W and (masks[0] >= 1).all()
    ref_l, ref_s = reference_scores(pts, [_CAM], masks)
    assert np.array_equal(ref_s, scores)
    assert np.array_equal(ref_l, labels)
    # every boundary is hit on both sides, at every depth: inside and outside points, pixel 0 from a negative target
    inside = scores[0] > 0
    assert inside.sum() == 4 * 8 * 8 and (~inside).sum() == 4 * (121 - 64) + 5  # per axis: -1, N and N + 0.5 are outside
    assert (scores[0] == 1).sum() == 4 * 6 * 6  # pixel 0 per axis: -1 + 2^-30, -0.5, -2^-30, 0, 0.5 and 1 - 2^-30
    assert (scores[0] == _H * _W).sum() == 4 and (labels[inside] == 1).sum() == 4 * 63


@pytest.mark.gpu
def test_label_points_on_exact_pixel_boundaries(gpu_device):
    pts, masks, scores, labels = _boundary_case()
    got_l, got_s = proc3d.label_points(pts, [_CAM], masks)
    ref_l, ref_s = reference_scores(pts, [_CAM], masks)
    print(f"boundaries: {len(pts)} points, {(got_s != scores).sum()} scores differ from the rule, "
          f"{(got_s != ref_s).sum()} from the reference loop")
    assert np.array_equal(got_s, scores) and np.array_equal(got_s, ref_s)
    assert np.array_equal(got_l, labels) and np.array_equal(got_l, ref_l)
    assert got_l.dtype == np.int32 and got_s.dtype == np.float64


def _random_case(P, V, L, width=96, height=80, seed=2):
    shape, origin, vs, views = scenes.make_scene(24, max(V, 1), "plant", width=width, height=height, fx=80.0, fy=80.0,
                                                 cx=width / 2.0, cy=height / 2.0)
    cams = [scenes.camera_dict(K, R, t) for K, R, t, _ in views][:V]
    rng = np.random.default_rng(seed)
    centre = np.array(origin) + (np.array(shape) - 1) * vs / 2
    pts = centre + rng.normal(size=(P, 3)) * np.array(shape) * vs * 0.6
    masks = rng.integers(0, 256, (L, V, height, width), dtype=np.uint8)
    return pts, cams, masks


@pytest.mark.gpu
def test_argmax_ties_and_points_no_view_sees(gpu_device):
    pts, cams, masks = _random_case(600, 3, 3)
    pts[:3] = [[0, 0, 1e6], [0, 0, -1e6], [np.nan, 0, 0]]  # far along the ring's axis, and NaN: outside every view
    masks[0] = masks[0] // 2
    masks[1] = masks[0] + 1
    masks[2] = masks[1]  # labels 1 and 2 tie above label 0: the first maximum is label 1
    labels, scores = proc3d.label_points(pts, cams, masks)
    ref_l, ref_s = reference_scores(pts, cams, masks)
    assert np.array_equal(scores, ref_s) and np.array_equal(labels, ref_l)
    seen = scores[1] > 0
    assert seen.sum() > 100 and (~seen).sum() >= 3 and not seen[:3].any()
    assert np.array_equal(scores[1], scores[2]) and (scores[1][seen] > scores[0][seen]).all()
    assert (labels[seen] == 1).all() and (labels[~seen] == 0).all() and (scores[:, ~seen] == 0).all()
    # all-zero masks: every score ties at zero, label 0
    labels, scores = proc3d.label_points(pts, cams, np.zeros_like(masks))
    assert not labels.any() and not scores.any() and scores.shape == (3, 600)
    # one label: label 0 everywhere, its scores the reference's
    labels, scores = proc3d.label_points(pts, cams, masks[1:2])
    assert not labels.any() and np.array_equal(scores, ref_s[1:2]) and scores.any()


@pytest.mark.gpu
@pytest.mark.parametrize("P", [0, 1, 255, 256, 257, 513])
def test_point_counts_around_the_block_size(gpu_device, P):
    pts, cams, masks = _random_case(P, 3, 2)
    labels, scores = proc3d.label_points(pts, cams, masks)
    ref_l, ref_s = reference_scores(pts, cams, masks)
    assert labels.shape == (P,) and labels.dtype == np.int32 and scores.shape == (2, P) and scores.dtype == np.float64
    assert np.array_equal(scores, ref_s) and np.array_equal(labels, ref_l)
    assert P < 255 or (scores > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("V", [0, 1])
def test_no_view_and_one_view(gpu_device, V):
    pts, cams, masks = _random_case(300, V, 3)
    assert len(cams) == V and masks.shape == (3, V, 80, 96)
    labels, scores = proc3d.label_points(pts, cams, masks)
    ref_l, ref_s = reference_scores(pts, cams, masks)
    assert scores.shape == (3, 300) and np.array_equal(scores, ref_s) and np.array_equal(labels, ref_l)
    if V == 0:
        assert not scores.any() and not labels.any()
        labels, scores = proc3d.label_points(np.zeros((0, 3)), cams, masks)  # and no point either
        assert labels.shape == (0,) and scores.shape == (3, 0)
    else:
        assert (scores > 0).any() and labels.any()


@pytest.mark.gpu
def test_pictures_taller_than_wide_and_five_labels(gpu_device):
    """The random test above with H > W: a swapped H and W in the addressing or the in-picture test shows."""
    shape, origin, vs, views = scenes.make_scene(32, 7, "plant", width=96, height=160, fx=125.0, fy=130.0,
                                                 cx=48.0, cy=80.0)
    cams = [scenes.camera_dict(K, R, t) for K, R, t, _ in views]
    rng = np.random.default_rng(4)
    centre = np.array(origin) + (np.array(shape) - 1) * vs / 2
    pts = centre + rng.normal(size=(5000, 3)) * np.array(shape) * vs * 0.6  # some fall outside the pictures
    masks = rng.integers(0, 256, (5, len(views), 160, 96), dtype=np.uint8)
    labels, scores = proc3d.label_points(pts, cams, masks)
    want_l, want_s = reference_scores(pts, cams, masks)
    assert np.array_equal(scores, want_s)
    assert np.array_equal(labels, want_l)
    assert scores.max() > 0 and (scores.sum(axis=0) == 0).any() and len(np.unique(labels)) == 5
