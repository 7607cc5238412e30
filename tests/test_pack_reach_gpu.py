"""SC_OPT_PACK_REACH: a batch of device masks that is packed at its flush packs, of every view, only the 32x32 tiles a
voxel of the engine can reach -- the image of the grid's box (whole bricks), worked out on the host from the pose.
Outside, the arena keeps what an earlier batch left there, and no kernel may look: labels equal the oracle's whatever
was packed before, the counters of the fused carve equal a fresh engine's, and the switch never changes a label.

Shapes: a 40 x 44 x 72 grid (ny no multiple of 16, nz none of 64: bricks stick out at both far faces), 12 views (8 are
packed ahead, 4 by riders), pictures of 320 x 224 (10 x 7 tiles: the eight-byte row loads of brick_verdict) and of
160 x 96 (5 tiles wide: its byte-by-byte path).  A rectangle is the hull of the box's image widened by the slack (2 px
and a little) plus one whole tile on every side and rounded outwards: at least three tiles in each direction wherever
it is not cut off.  For it to stay under 40 % of a picture the rings are far away (the grid's image a few dozen pixels
across), and in the 160 x 96 pictures the principal point is moved until the image hangs over the picture's corner,
where the rectangle is clamped."""
import numpy as np
import pytest

from oracle import oracle_c
from plant3dvision_amd import _native as nat, scenes

SHAPE = (40, 44, 72)
NVIEWS = 12
BRICK_Y, BRICK_Z, TILE = 16, 64, 32
# (width, height, fx = fy, cx, cy): the ring is scenes.make_scene's (radius 2 x the grid's longest edge, at its centre's height)
RIGS = {"320x224": dict(width=320, height=224, fx=72.0, fy=72.0, cx=160.0, cy=112.0),
        "160x96": dict(width=160, height=96, fx=36.0, fy=36.0, cx=8.0, cy=8.0)}
CAP = 0.40  # share of a picture's tiles the reach rectangle of a view may cover (every view)


def reach_rect_np(shape, origin, vs, K, R, t, W, H, planes=None):
    """NumPy restatement of the host's reach rectangle (tiles [tx0, tx1) x [ty0, ty1)), or None for the whole picture:
    the hull of the images of the eight corners of (engine's planes) x (whole bricks), widened by rect_box's slack for
    the whole box plus one tile, clamped to the picture, rounded outwards to tiles."""
    nx, ny, nz = shape
    planes = range(nx) if planes is None else planes
    f32 = np.float32
    last = (planes[-1], (ny + BRICK_Y - 1) // BRICK_Y * BRICK_Y - 1, (nz + BRICK_Z - 1) // BRICK_Z * BRICK_Z - 1)
    first = (planes[0], 0, 0)
    c = [[float(f32(origin[a]) + f32(first[a]) * f32(vs)), float(f32(origin[a]) + f32(last[a]) * f32(vs))] for a in range(3)]
    Rm = np.asarray(R, dtype=np.float64).reshape(3, 3)
    tv = np.asarray(t, dtype=np.float64)
    Kd = [float(k) for k in K]
    err = [(abs(tv[r]) + sum(abs(Rm[r, a]) * max(abs(c[a][0]), abs(c[a][1])) for a in range(3))) * 2.0 ** -19 for r in range(3)]
    us, vs_, qx, qy, pz = [], [], [], [], []
    for q in range(8):
        X = np.array([c[0][q & 1], c[1][(q >> 1) & 1], c[2][(q >> 2) & 1]])
        p = Rm @ X + tv
        if not (p[2] > 8.0 * err[2] and p[2] > 2.0 ** -10):
            return None
        qx.append(p[0] / p[2]); qy.append(p[1] / p[2]); pz.append(p[2])
        us.append(qx[-1] * Kd[0] + Kd[2]); vs_.append(qy[-1] * Kd[1] + Kd[3])
    inv = 2.0 / min(pz)
    qxm, qym = max(abs(x) for x in qx), max(abs(x) for x in qy)
    mu = 2.0 + abs(Kd[0]) * (err[0] + qxm * err[2]) * inv + (abs(Kd[0]) * qxm + abs(Kd[2]) + max(abs(min(us)), abs(max(us)))) * 2.0 ** -20
    mv = 2.0 + abs(Kd[1]) * (err[1] + qym * err[2]) * inv + (abs(Kd[1]) * qym + abs(Kd[3]) + max(abs(min(vs_)), abs(max(vs_)))) * 2.0 ** -20
    if not (mu <= 32.0 and mv <= 32.0):
        return None
    ulo, uhi, vlo, vhi = min(us) - mu - 32.0, max(us) + mu + 32.0, min(vs_) - mv - 32.0, max(vs_) + mv + 32.0
    if uhi < 0 or vhi < 0 or ulo > W - 1 or vlo > H - 1:
        return (0, 0, 0, 0)
    return (int(max(ulo, 0.0) // TILE), int(min(uhi, W - 1.0) // TILE) + 1, int(max(vlo, 0.0) // TILE), int(min(vhi, H - 1.0) // TILE) + 1)


def rect_tiles(rect, W, H):
    tx, ty = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    return tx * ty if rect is None else max(0, rect[1] - rect[0]) * max(0, rect[3] - rect[2])


def ball_points(centre, radius, spacing):
    n = int(np.ceil(radius / spacing))
    ax = np.arange(-n, n + 1) * spacing
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    keep = X ** 2 + Y ** 2 + Z ** 2 <= radius ** 2
    return np.stack([X[keep], Y[keep], Z[keep]], axis=1) + np.asarray(centre, dtype=np.float64)


_SCENES = {}


def rig_scene(rig, kind):
    """(shape, origin, vs, views, oracle labels) -- built once per (rig, kind), never modified."""
    key = (rig, kind)
    if key in _SCENES:
        return _SCENES[key]
    kw = RIGS[rig]
    W, H = kw["width"], kw["height"]
    base = {"thin": "empty", "corner": "empty", "inside": "empty"}.get(kind, kind)
    sh, origin, vs, views = scenes.make_scene(SHAPE, NVIEWS, base, **kw)
    hi = [origin[a] + (sh[a] - 1) * vs for a in range(3)]
    mid = [(origin[a] + hi[a]) / 2 for a in range(3)]
    if kind == "thin":  # a thin column through the middle of the grid with a ball on it
        col = np.stack([np.full(200, mid[0]), np.full(200, mid[1]), np.linspace(origin[2] + 2 * vs, hi[2] - 2 * vs, 200)], axis=1)
        pts = np.concatenate([col, ball_points((mid[0] + 2.0, mid[1] - 1.5, mid[2] + 4.0), 2.5, 0.4)])
        views = [(K, R, t, scenes.splat_mask(pts, K, R, t, W, H, dilate=1)) for K, R, t, _ in views]
    elif kind == "corner":  # a ball in the grid's last corner: the live box touches three of its faces
        pts = ball_points((hi[0] - 1.5, hi[1] - 1.5, hi[2] - 2.0), 3.0, 0.4)
        views = [(K, R, t, scenes.splat_mask(pts, K, R, t, W, H, dilate=1)) for K, R, t, _ in views]
    elif kind == "inside":  # the thin object, and one camera inside the grid: its view is not certified
        _, _, _, thin, _ = rig_scene(rig, "thin")
        views = [tuple(v) for v in thin]
        K, R, t, m = views[5]
        Rm = np.asarray(R, dtype=np.float64).reshape(3, 3)
        t2 = (-Rm @ np.asarray(mid, dtype=np.float64)).astype(np.float32)  # the same look, from the grid's centre
        views[5] = (K, R, t2, m)
        assert not nat.view_certified(sh, origin, vs, K, R, t2)
    want = oracle_c.carve(sh, origin, vs, views, nthreads=8)
    _SCENES[key] = (sh, origin, vs, views, want)
    return _SCENES[key]


def reach_share(rig, kind="thin"):
    sh, origin, vs, views, _ = rig_scene(rig, kind)
    W, H = RIGS[rig]["width"], RIGS[rig]["height"]
    total = rect_tiles(None, W, H)
    return [rect_tiles(reach_rect_np(sh, origin, vs, K, R, t, W, H), W, H) / total for K, R, t, _ in views]


def rider_lower_bound(rig, kind="thin"):
    """Tiles the riders cannot do without: a voxel that survives the carve lies in a brick no view found empty (live, or a
    candidate) and lands, in every view that sees it, on a foreground pixel -- so the tile under it holds foreground
    under a live brick's footprint.  Which four views ride is the engine's choice: the four smallest counts."""
    sh, origin, vs, views, want = rig_scene(rig, kind)
    W, H = RIGS[rig]["width"], RIGS[rig]["height"]
    idx = np.argwhere(want >= 0).astype(np.float64)
    X = np.asarray(origin, dtype=np.float64) + idx * vs
    per_view = []
    for K, R, t, _ in views:
        p = X @ np.asarray(R, dtype=np.float64).reshape(3, 3).T + np.asarray(t, dtype=np.float64)
        u, v = p[:, 0] / p[:, 2] * float(K[0]) + float(K[2]), p[:, 1] / p[:, 2] * float(K[1]) + float(K[3])
        # (well inside a tile and the picture: float32 against float64 cannot move such a voxel to another tile)
        ok = (p[:, 2] > 0) & (u > 0.01) & (u < W - 0.01) & (v > 0.01) & (v < H - 0.01)
        ok &= (np.abs(u / TILE - np.round(u / TILE)) > 1e-3) & (np.abs(v / TILE - np.round(v / TILE)) > 1e-3)
        per_view.append(len({(int(a) // TILE, int(b) // TILE) for a, b in zip(u[ok], v[ok])}))
    return sum(sorted(per_view)[:NVIEWS - 8])


def box_image_np(shape, origin, vs, K, R, t):
    """Brute force, independent of reach_rect's hull and slack: (u, v) of EVERY voxel centre of the grid's box of whole
    bricks (float64 arithmetic on the kernels' float32 coordinates), for the voxels in front of the camera."""
    nx, ny, nz = shape
    f32 = np.float32
    nyb, nzb = (ny + BRICK_Y - 1) // BRICK_Y * BRICK_Y, (nz + BRICK_Z - 1) // BRICK_Z * BRICK_Z
    ax = [(f32(origin[a]) + np.arange(n, dtype=f32) * f32(vs)).astype(np.float64) for a, n in enumerate((nx, nyb, nzb))]
    X = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    p = X @ np.asarray(R, dtype=np.float64).reshape(3, 3).T + np.asarray(t, dtype=np.float64)
    assert (p[:, 2] > 0).all()
    return p[:, 0] / p[:, 2] * float(K[0]) + float(K[2]), p[:, 1] / p[:, 2] * float(K[1]) + float(K[3])


@pytest.mark.parametrize("rig", sorted(RIGS))
def test_reach_rectangles_of_the_test_scenes_on_the_cpu(rig):
    """The NumPy restatement of the host's rectangle leaves under 40 % of the tiles inside in EVERY view of every scene
    the GPU tests use; the riders' lower bound stays under their cap (half of their views' tiles); and, by brute force
    over every voxel of the box of whole bricks, the rectangle holds every pixel a voxel lands on with a whole tile and
    the 2-pixel slack to spare on each side where the picture's edge does not cut it."""
    W, H = RIGS[rig]["width"], RIGS[rig]["height"]
    for kind in ("thin", "corner"):
        share = reach_share(rig, kind)
        assert len(share) == NVIEWS and max(share) < CAP, (rig, kind, share)
        assert min(share) > 0.0
    sh, origin, vs, views, _ = rig_scene(rig, "thin")
    for K, R, t, _ in views:
        tx0, tx1, ty0, ty1 = reach_rect_np(sh, origin, vs, K, R, t, W, H)
        u, v = box_image_np(sh, origin, vs, K, R, t)
        assert (tx0 == 0 or tx0 * TILE <= u.min() - 34.0) and (tx1 * TILE >= W or tx1 * TILE - 1 >= u.max() + 34.0), (rig, tx0, tx1, u.min(), u.max())
        assert (ty0 == 0 or ty0 * TILE <= v.min() - 34.0) and (ty1 * TILE >= H or ty1 * TILE - 1 >= v.max() + 34.0), (rig, ty0, ty1, v.min(), v.max())
    inside = reach_share(rig, "inside")
    assert inside[5] == 1.0, "an uncertified view takes the whole picture"
    lb = rider_lower_bound(rig)
    assert 0 < lb < 0.5 * (NVIEWS - 8) * rect_tiles(None, W, H), (rig, lb)


def run_batches(rig, batches, reach, opts=None, pack_rows=None, every=None):
    """One engine, the batches one after the other (clear() between them); returns the labels, fused_counts_ex and
    pack_counts of the last one.  `reach`: the switch, one value or one per batch; `every`: a list that takes the
    pack_counts of every batch."""
    sh, origin, vs = rig_scene(rig, batches[-1])[:3]
    e = nat.Engine(sh, origin, vs, nat.SC_MODE_CARVE)
    reaches = list(reach) if isinstance(reach, (list, tuple)) else [reach] * len(batches)
    if pack_rows is not None:
        e.set_option(nat.SC_OPT_PACK_ROWS, pack_rows)
    for k, v in (opts or {}).items():
        e.set_option(getattr(nat, k), v)
    ptr = 0
    try:
        for q, kind in enumerate(batches):
            views = rig_scene(rig, kind)[3]
            stack = np.ascontiguousarray(np.stack([m for _, _, _, m in views]))
            if not ptr:
                ptr = e.dev_alloc(stack.nbytes)
            if q:
                e.clear()
            e.set_option(nat.SC_OPT_PACK_REACH, reaches[q])
            e.dev_upload(ptr, stack)
            K = np.stack([v[0] for v in views]); R = np.stack([v[1] for v in views]); t = np.stack([v[2] for v in views])
            e.process_views_device(K, R, t, ptr, *stack.shape, nat.SC_MASK_U8)
            got = e.get_values().copy()
            if every is not None:
                every.append(e.pack_counts())
        return got, e.fused_counts_ex(), e.pack_counts()
    finally:
        if ptr:
            e.synchronize()
            e.dev_free(ptr)
        e.close()


CASES = [("thin", {}), ("corner", {}), ("solid", {}), ("empty", {}), ("inside", {}),
         ("thin", {"SC_OPT_UNIT_CULL": 2}), ("thin", {"SC_OPT_LIST_CAP": 16}), ("corner", {"SC_OPT_UNIT_CULL": 2, "SC_OPT_LIST_CAP": 16})]


@pytest.mark.gpu
@pytest.mark.parametrize("pack_rows", [None, 3, 1])  # the default form for the width; bands whatever the width; one-row panels
@pytest.mark.parametrize("rig", sorted(RIGS))
def test_labels_equal_the_oracle_with_the_switch_on_and_off(gpu_device, rig, pack_rows):
    for kind, opts in CASES:
        want = rig_scene(rig, kind)[4]
        for reach in (1, 0):
            got, counts, packs = run_batches(rig, [kind], reach, opts, pack_rows)
            assert np.array_equal(got, want), (rig, kind, opts, pack_rows, reach, int((got != want).sum()))
            if opts.get("SC_OPT_LIST_CAP"):
                assert kind == "corner" or counts["list_overflow"] == 1, "the case is meant to reach the overflow fallback"


@pytest.mark.gpu
@pytest.mark.parametrize("rig", sorted(RIGS))
@pytest.mark.parametrize("poison", ["solid", "empty"])
def test_stale_tiles_of_an_earlier_batch_are_never_looked_at(gpu_device, rig, poison):
    """The arena is reused from batch to batch: outside a view's rectangle lie the previous batch's tiles, occupancy
    bytes and cell words.  The poison batch is packed with the switch OFF -- whole pictures, all foreground or all
    background, strictly more tiles than the thin batch packs -- so every tile the thin batch leaves alone holds
    poison when it runs on the same engine with the switch on (and, for the record, off).  Labels equal the oracle's
    and every counter of the fused carve equals a fresh engine's: no verdict saw a stale tile."""
    want = rig_scene(rig, "thin")[4]
    for reach in (1, 0):
        for pack_rows in (None, 3):
            fresh, fresh_counts, _ = run_batches(rig, ["thin"], reach, None, pack_rows)
            packs = []
            got, counts, _ = run_batches(rig, [poison, "thin"], [0, reach], None, pack_rows, every=packs)
            per_batch = [c[0] + c[2] for c in packs]
            assert per_batch[0] == NVIEWS * rect_tiles(None, RIGS[rig]["width"], RIGS[rig]["height"])
            assert (per_batch[1] < per_batch[0]) if reach else (per_batch[1] == per_batch[0]), (rig, poison, reach, packs)
            assert np.array_equal(fresh, want) and np.array_equal(got, want), (rig, poison, reach, pack_rows)
            assert counts == fresh_counts, (rig, poison, reach, pack_rows, counts, fresh_counts)


@pytest.mark.gpu
@pytest.mark.parametrize("rig", sorted(RIGS))
def test_pack_counts(gpu_device, rig):
    """With the switch on every view packs exactly its rectangle -- ahead or beside the dense stage, in bands or in
    panels, whatever the masks hold: the riders fewer than half of their views' tiles, and no fewer than hold
    foreground under a live brick; with it off, every tile."""
    sh, origin, vs, views, _ = rig_scene(rig, "thin")
    W, H = RIGS[rig]["width"], RIGS[rig]["height"]
    per_view = rect_tiles(None, W, H)
    rects = sorted(rect_tiles(reach_rect_np(sh, origin, vs, K, R, t, W, H), W, H) for K, R, t, _ in views)
    for pack_rows in (None, 3):
        _, _, on = run_batches(rig, ["thin"], 1, None, pack_rows)
        _, _, off = run_batches(rig, ["thin"], 0, None, pack_rows)
        print(rig, pack_rows, "pack counts on", on, "off", off, "lower bound", rider_lower_bound(rig))
        assert off == (8 * per_view, 8 * per_view, 4 * per_view, 4 * per_view)
        assert on[1] == 8 * per_view and on[3] == 4 * per_view
        assert sum(rects[:8]) <= on[0] <= sum(rects[-8:])  # (which eight go ahead is the engine's order)
        assert rider_lower_bound(rig) <= on[2] < 0.5 * on[3], (rig, pack_rows, on)
        assert sum(rects[:4]) <= on[2] <= sum(rects[-4:])
        for kind in ("empty", "solid"):
            _, _, other = run_batches(rig, [kind], 1, None, pack_rows)
            assert other[0] == on[0] and other[2] == on[2], (rig, kind, other, on)
