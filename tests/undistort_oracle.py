"""The checker of the lens correction (``sc_undistort_rgb`` / ``proc2d.undistort``), NumPy only, written as DESIGN.md 17
reads.

PARITY UNPINNED: OpenCV is not available here, so this restates ``cv2.undistort(img, A, dist,
None)`` from OpenCV's published algorithm -- ``initUndistortRectifyMap`` with identity rectification and
``newCameraMatrix = A``, map type ``CV_16SC2``, ``INTER_BITS = 5``, then ``remap(INTER_LINEAR, BORDER_CONSTANT 0)`` on
8-bit pixels with 15-bit weights -- with the two documented deviations: the ray of a pixel is evaluated directly (not
by running sums along the row), and a source column or row beyond +-32768 lies outside (no ``(short)`` wrap).

Every operation of the ray is one IEEE binary64 operation, in the order written (NumPy does not contract).
"""
import numpy as np

INT32_MIN = -(1 << 31)
CAMERAS = ("real", "barrel", "pincushion", "k3", "identity")
SHAPES = [(1, 1), (7, 13), (61, 1031), (1031, 61), (270, 360), (1080, 1440)]
LARGER = SHAPES[2:]


def camera(name, H, W):
    """The test cameras for a picture of ``H x W``: (float32 3x3, float32 [5]), every value through float32 as the
    reference's ``get_camera_arrays_from_params`` makes them."""
    f = 0.81 * max(H, W)
    fx, fy, cx, cy, d = {
        "real": (f, f, W / 2, H / 2, (-0.00115644, 0, 0, 0, 0)),
        "barrel": (f, 1.006 * f, W / 2 - 4.7, H / 2 + 4.9, (-0.12, 0.05, 0.002, -0.0015, 0)),
        "pincushion": (f, f, W / 2, H / 2, (0.2, 0.03, 0, 0, 0)),
        "k3": (f, 0.99 * f, W / 2 + 0.3, H / 2 - 0.4, (-0.2, 0.08, -0.001, 0.0007, -0.02)),
        "identity": (f, f, W / 2, H / 2, (0, 0, 0, 0, 0)),
    }[name]
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32), np.array(d, dtype=np.float32)


def picture(H, W, V=None, seed=None):
    """Seeded uniform random bytes, ``[H, W, 3]`` or ``[V, H, W, 3]``."""
    rng = np.random.default_rng(H * 7919 + W if seed is None else seed)
    return rng.integers(0, 256, size=((H, W, 3) if V is None else (V, H, W, 3)), dtype=np.uint8)


def intrinsics(mtx, dist):
    """``(K[4] = fx fy cx cy, dist[5] = k1 k2 p1 p2 k3)`` as float64, widened as cv2 widens its arguments."""
    m = np.asarray(mtx, dtype=np.float64)
    d = np.asarray(dist, dtype=np.float64).reshape(-1)
    d5 = np.zeros(5, dtype=np.float64)
    d5[:min(5, d.size)] = d[:5]
    return np.array([m[0, 0], m[1, 1], m[0, 2], m[1, 2]], dtype=np.float64), d5


def rays(H, W, K, dist):
    """``(u, v)``: where output pixel (row i, column j) looks in the source, float64 ``[H, W]`` each."""
    fx, fy, cx, cy = (np.float64(c) for c in K)
    k1, k2, p1, p2, k3 = (np.float64(c) for c in dist)
    j = np.broadcast_to(np.arange(W, dtype=np.float64)[None, :], (H, W))
    i = np.broadcast_to(np.arange(H, dtype=np.float64)[:, None], (H, W))
    with np.errstate(all="ignore"):
        x = (j - cx) / fx
        y = (i - cy) / fy
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = (2 * x) * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = (x * kr + p1 * _2xy) + p2 * (r2 + 2 * x2)
        yd = (y * kr + p1 * (r2 + 2 * y2)) + p2 * _2xy
        u = fx * xd + cx
        v = fy * yd + cy
    return u, v


def _fixed(u, v):
    with np.errstate(all="ignore"):
        fu, fv = np.rint(32 * u), np.rint(32 * v)  # round half to even
        unmapped = ~np.isfinite(u) | ~np.isfinite(v) | ~(np.abs(fu) < 2.0 ** 30) | ~(np.abs(fv) < 2.0 ** 30)
    iu = np.where(unmapped, float(INT32_MIN), fu).astype(np.int64).astype(np.int32)
    iv = np.where(unmapped, float(INT32_MIN), fv).astype(np.int64).astype(np.int32)
    return iu, iv


def umap(H, W, K, dist):
    """The map: ``(iu, iv)`` int32 ``[H, W]`` each, source position in 1/32 pixel; ``INT32_MIN`` in both for an
    unmapped pixel."""
    return _fixed(*rays(H, W, K, dist))


def remap(img, iu, iv):
    """The pictures ``[..., H, W, 3]`` looked up through the map: fixed-point bilinear, 0 outside the picture."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape[-1] == 3 and img.shape[-3:-1] == iu.shape
    H, W = iu.shape
    iu, iv = iu.astype(np.int64), iv.astype(np.int64)
    sx, sy, a, b = iu >> 5, iv >> 5, (iu & 31)[..., None], (iv & 31)[..., None]

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        p = img[..., np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1), :].astype(np.int64)
        return np.where(inside[..., None], p, 0)

    S = (32 - a) * (32 - b) * tap(sy, sx) + a * (32 - b) * tap(sy, sx + 1) \
        + (32 - a) * b * tap(sy + 1, sx) + a * b * tap(sy + 1, sx + 1)
    return ((S + 512) >> 10).astype(np.uint8)


def undistort(img, mtx, dist):
    """``cv2.undistort(img, mtx, dist, None)`` for uint8 RGB pictures ``[H, W, 3]`` or ``[V, H, W, 3]``."""
    img = np.asarray(img)
    H, W = img.shape[-3:-1]
    K, d = intrinsics(mtx, dist)
    return remap(img, *umap(H, W, K, d))


def account(H, W, iu, iv, K=None, dist=None):
    """What the map asks of a picture: the shares of pixels with all four taps inside, with some inside, with none
    inside or unmapped (the three add up to 1), and -- given the camera -- the least distance of ``32 u``, ``32 v``
    of a mapped pixel to a rounding tie (a value of k + 1/2)."""
    unmapped = (iu == INT32_MIN) & (iv == INT32_MIN)
    sx, sy = iu.astype(np.int64) >> 5, iv.astype(np.int64) >> 5
    nin = np.zeros(iu.shape, dtype=np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            nin += (sy + dy >= 0) & (sy + dy < H) & (sx + dx >= 0) & (sx + dx < W)
    nin[unmapped] = 0
    n = float(iu.size)
    out = {"all": np.count_nonzero(nin == 4) / n, "some": np.count_nonzero((nin > 0) & (nin < 4)) / n,
           "none": np.count_nonzero(nin == 0) / n, "unmapped": np.count_nonzero(unmapped) / n, "tie": None}
    if K is not None:
        tie = np.inf
        for r in rays(H, W, K, dist):
            t = 32 * r[~unmapped]
            if t.size:
                tie = min(tie, float(np.abs((t - np.floor(t)) - 0.5).min()))
        out["tie"] = tie
    return out


def weights15(a, b):
    """OpenCV's 15-bit table entry for the fraction ``(a, b)`` / 32, for the taps (sy, sx), (sy, sx+1), (sy+1, sx),
    (sy+1, sx+1): the float32 weights times 2^15 as int16 with saturation.  The products are exact and add up to 2^15
    except for ``a = b = 0``, whose single weight 32768 saturates to 32767."""
    fa, fb = np.float32(a) / np.float32(32), np.float32(b) / np.float32(32)
    w = np.array([(1 - fa) * (1 - fb), fa * (1 - fb), (1 - fa) * fb, fa * fb], dtype=np.float32) * np.float32(32768)
    return np.clip(np.rint(w), -32768, 32767).astype(np.int64)
