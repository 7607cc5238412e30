"""The checkers of the multiclass ``PointCloud`` task (``proc3d.select_classes``, ``proc3d.vol2pcd_class``,
``tasks.proc3d.point_cloud_run``): the reference's lines restated in NumPy, in the reference's own order of operations.

``literal_class_volumes`` is ``PointCloud.run`` :81-115 of plant3dvision/tasks/proc3d.py as written: the float64
``[nx, ny, nz, L]`` array, the background's prior, ``argmax``, per class ``np.delete`` + ``np.max`` and the two
in-place products.  ``literal_run`` goes on to :117-129 with ``oracle.vol2pcd_oracle`` in the place of
``proc3d.vol2pcd`` and plain arrays in the place of the open3d container.  ``closed_form_winner`` is the contract of
``include/spacecarve.h`` (``sc_select_classes``) written down a second time, without ``np.delete``: the CPU tests
compare the two.  Nothing here knows how the device decides.
"""
import warnings

import numpy as np

from oracle import vol2pcd_oracle

NONE = 255

# what the adversarial stacks are drawn from: repeated maxima, zeros of both signs, negatives, infinities, NaN, values
# on the contrast boundary (1 > 10 * 0.1 in float64 or not, 1 > 1.5 * 0.6666..., 1 > 2 * 0.5)
POOL = np.array([0.0, -0.0, 1.0, 1.0, 0.1, 10.0, 0.5, 0.05, -1.0, -10.0, -0.1, 2.0, 20.0, 3.0, np.inf, -np.inf, np.nan, np.nan,
                 1e-30, 0.099999, 0.100001, 0.1 + 2.0 ** -56, 2.0 / 3.0, 0.666, 5.0, 0.0, 0.0], dtype=np.float64)
INT_POOL = np.array([0, 0, 0, 1, 1, 2, 3, 7, 200, 255], dtype=np.uint8)

#: (background_prior, min_contrast, min_score): the defaults, contrast off (== 1 and below), the prior at 0 and
#: fractional, a score nothing passes (== 1 and above)
PARAMETER_SETS = [(1.0, 10.0, 0.2), (1.0, 1.0, 0.2), (2.0, 0.5, 0.0), (0.0, 10.0, 0.2), (0.25, 1.5, 0.999), (1.0, 2.0, 1.0)]


def literal_class_volumes(voxels, background_prior=1.0, min_contrast=10.0, min_score=0.2):
    """``(l, {label: pred_c})`` for every label but ``'background'``: tasks/proc3d.py:81-115 as written."""
    out = {}
    with warnings.catch_warnings(), np.errstate(invalid="ignore", over="ignore"):
        warnings.simplefilter("ignore")
        l = list(voxels.keys())
        res = np.zeros((*voxels[l[0]].shape, len(l)))
        for i in range(len(l)):
            res[:, :, :, i] = voxels[l[i]]
        for i in range(len(l)):
            if l[i] == 'background':
                res[:, :, :, i] *= background_prior
        res_idx = np.argmax(res, axis=3)
        for i in range(len(l)):
            if l[i] != 'background':
                pred_no_c = np.copy(res)
                pred_no_c = np.max(np.delete(res, i, axis=3), axis=3)
                pred_c = res[:, :, :, i]
                pred_c = (res_idx == i)
                if min_contrast > 1.0:
                    pred_c *= (pred_c > (min_contrast * pred_no_c))
                pred_c *= (pred_c > min_score)
                out[l[i]] = pred_c
    return l, out


def winner_of(l, class_volumes, shape):
    """The uint8 winner volume of a set of class volumes (they must not overlap) and the voxel count per class."""
    winner = np.full(shape, NONE, dtype=np.uint8)
    counts = np.zeros(len(l), dtype=np.int64)
    for i, label in enumerate(l):
        if label in class_volumes:
            mine = np.asarray(class_volumes[label], dtype=bool)
            assert (winner[mine] == NONE).all(), "two classes own a voxel"
            winner[mine] = i
            counts[i] = int(mine.sum())
    return winner, counts


def literal_winner(voxels, background_prior=1.0, min_contrast=10.0, min_score=0.2):
    """``(winner, labels, counts)`` from the literal lines: the signature of ``proc3d.select_classes``."""
    l, vols = literal_class_volumes(voxels, background_prior, min_contrast, min_score)
    winner, counts = winner_of(l, vols, np.asarray(voxels[l[0]]).shape)
    return winner, l, counts


def closed_form_winner(voxels, background_prior=1.0, min_contrast=10.0, min_score=0.2):
    """``(winner, labels, counts)`` by the rule of ``sc_select_classes`` in include/spacecarve.h."""
    l = list(voxels.keys())
    with warnings.catch_warnings(), np.errstate(invalid="ignore", over="ignore"):
        warnings.simplefilter("ignore")
        res = np.stack([np.asarray(voxels[k]).astype(np.float64) for k in l], axis=-1)
        bg = l.index("background") if "background" in l else -1
        if bg >= 0:
            res[..., bg] = res[..., bg] * np.float64(background_prior)
        isnan = np.isnan(res)
        first_nan = np.argmax(isnan, axis=-1)
        plain = np.argmax(np.where(isnan, -np.inf, res), axis=-1)  # the first index of the greatest value
        m = np.where(isnan.any(axis=-1), first_nan, plain)
        others = res.copy()
        np.put_along_axis(others, m[..., None], -np.inf, axis=-1)  # (L >= 2: -inf is never the only value left)
        v2 = np.where(np.isnan(others).any(axis=-1), np.nan, np.max(np.where(np.isnan(others), -np.inf, others), axis=-1))
        ok = m != bg
        if min_contrast > 1.0:
            ok = ok & (1.0 > np.float64(min_contrast) * v2)
        ok = ok & bool(1.0 > min_score)
    winner = np.where(ok, m, NONE).astype(np.uint8)
    counts = np.array([int((winner == i).sum()) for i in range(len(l))], dtype=np.int64)
    return winner, l, counts


def adversarial_stack(shape, L, seed, dtype=np.float64, background_at=None):
    """``{label: volume}`` with the labels ``c0 .. c{L-1}`` (``'background'`` at index ``background_at``), drawn from the
    pools above; one voxel in eight repeats its first value in every class (a tie of all L)."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    labels = [("background" if q == background_at else f"c{q}") for q in range(L)]
    out = {}
    all_tie = rng.integers(0, 8, size=shape) == 0
    first = None
    for k in labels:
        if dtype == np.bool_:
            v = rng.integers(0, 2, size=shape).astype(np.bool_)
        elif dtype == np.uint8:
            v = INT_POOL[rng.integers(0, INT_POOL.size, size=shape)]
        else:
            v = POOL[rng.integers(0, POOL.size, size=shape)].astype(dtype)
        if first is None:
            first = v
        out[k] = np.ascontiguousarray(np.where(all_tie, first, v).astype(dtype))
    return out


class Cloud:
    def __init__(self, points, normals, colors=None):
        self.points, self.normals, self.colors = points, normals, colors


def vol2pcd(volume, origin, voxel_size, level_set_value):
    """``oracle.vol2pcd_oracle`` behind the one documented deviation of the device's ``vol2pcd``: a volume
    of one class -- nothing above 0.5, or nothing at or below it -- is an empty cloud."""
    occ = np.asarray(volume) > 0.5
    if not occ.any() or occ.all():
        return Cloud(np.zeros((0, 3)), np.zeros((0, 3)))
    pts, normals = vol2pcd_oracle.vol2pcd(volume, origin, voxel_size, level_set_value)[:2]
    return Cloud(pts, normals)


def literal_run(voxels, origin, voxel_size, level_set_value=1.0, background_prior=1.0, min_contrast=10.0, min_score=0.2,
                colors=None, random_color=None):
    """``(points, normals, colors, point_labels, points_per_class)``: tasks/proc3d.py:99-129 with arrays in the place of
    the open3d clouds (``pcd + out`` appends)."""
    l, vols = literal_class_volumes(voxels, background_prior, min_contrast, min_score)
    points, normals, cols, point_labels, per_class = np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), [], {}
    origin = np.array(origin)
    voxel_size = float(voxel_size)
    for i in range(len(l)):
        if l[i] != 'background':
            out = vol2pcd(vols[l[i]], origin, voxel_size, level_set_value)
            color = np.zeros((len(out.points), 3))
            if l[i] in colors:
                color[:] = np.asarray(colors[l[i]])
            else:
                color[:] = random_color()
            points, normals, cols = np.concatenate([points, out.points]), np.concatenate([normals, out.normals]), np.concatenate([cols, color])
            point_labels = point_labels + [l[i]] * len(out.points)
            per_class[l[i]] = len(out.points)
    return points, normals, cols, point_labels, per_class


ORGANS = ("stem", "leaf", "flower", "fruit")


def organ_scene(shape, seed=7, dtype=np.float32):
    """Five class volumes, ``background`` first: every organ is three balls with a core of 1 and a linear rim, rounded to
    sixteenths and scaled by 8 (so values repeat across classes: ties on purpose); the background is 8 x (1 - the
    greatest organ value of the voxel)."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), axis=-1)
    unit = {}
    for k in ORGANS:
        f = np.zeros(shape)
        for _ in range(3):
            c = rng.uniform(0.15, 0.85, 3) * np.array(shape)
            core, rim = rng.uniform(2.0, 4.5), rng.uniform(2.0, 4.0)
            d = np.sqrt(((g - c) ** 2).sum(axis=-1))
            f = np.maximum(f, np.clip((core + rim - d) / rim, 0.0, 1.0))
        unit[k] = np.round(f * 16.0) / 16.0
    top = np.max(np.stack([unit[k] for k in ORGANS]), axis=0)
    scene = {"background": (8.0 * (1.0 - top)).astype(dtype)}
    for k in ORGANS:
        scene[k] = (8.0 * unit[k]).astype(dtype)
    return scene
