"""GPU: the mask producer (``sc_masks_from_rgb`` / ``proc2d.masks_from_images``) against the checker
(tests/proc2d_oracle.py), bit for bit: ``np.array_equal``, no tolerance."""
import os

import numpy as np
import pytest

from oracle import oracle_c
from plant3dvision_amd import _native as nat
from plant3dvision_amd import masks2d, proc2d, scenes
from tests import proc2d_oracle as oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_plant_rgb")
# (H, W): widths that are not multiples of 4, 16 or 64; 61 wide is less than one 64-bit word per row
SIZES = [(1, 1), (7, 13), (1031, 61), (61, 1031), (1080, 1440)]


def entry(images, type, coefs, threshold, dilation, device):
    """``sc_masks_from_rgb`` itself on host arrays: (masks, ranges [V][2])."""
    images = np.ascontiguousarray(images)
    V, H, W, _ = images.shape
    b = nat.backend()
    c = np.asarray(coefs, dtype=np.float64)
    steps = proc2d.dilation_steps(dilation) if dilation else np.zeros(0, np.uint8)
    out = np.empty((V, H, W), dtype=np.uint8)
    ranges = np.full((V, 2), -1, dtype=np.int32)
    rc = b.call("sc_masks_from_rgb", nat.addr(images), 0, V, H, W, proc2d.FILTERS[type], nat.addr(c), float(threshold),
                nat.addr(steps) if steps.size else 0, int(steps.size), device, 0, nat.addr(out), 0, nat.addr(ranges))
    assert rc == nat.SC_OK, b.string(b.call("sc_masks_last_error"))
    return out, ranges


@pytest.fixture(scope="module")
def colours():
    img = oracle.all_colours()
    return img, oracle.normalised(img)


@pytest.mark.gpu
@pytest.mark.parametrize("type_,coefs,threshold", [
    ("excess_green", (0, 1, 0), 0.0), ("excess_green", (0, 1, 0), 0.1), ("excess_green", (0, 1, 0), 0.3),
    ("linear", (0, 1, 0), 0.15), ("linear", (0, 1, 0), 0.3), ("linear", (0.1, 1.0, 0.1), 0.3)])
def test_every_colour(gpu_device, colours, type_, coefs, threshold):
    """Exhaustive over the per-pixel function for the range 0..255: each of the 2^24 colours once."""
    img, norm = colours
    want = oracle.masks(img, type_, coefs, threshold, 0, norm=norm)
    got, ranges = entry(img[None], type_, coefs, threshold, 0, gpu_device)
    assert ranges.tolist() == [[0, 255]]
    diff = int(np.count_nonzero(got[0] != want))
    print(f"every colour {type_} {coefs} > {threshold}: set {int((want != 0).sum())}, different {diff}")
    assert np.array_equal(got[0], want)
    assert 0 < (want != 0).sum() < want.size


def _ranged_pictures(H, W, seed):
    rng = np.random.default_rng(seed)
    pics, want = [], []
    for lo, hi in [(3, 250), (0, 1), (254, 255), (100, 101)]:
        p = rng.integers(lo, hi + 1, size=(H, W, 3), dtype=np.uint8)
        p[0, 0, 0], p[-1, -1, 2] = lo, hi  # both ends are there (a 1 x 1 picture has three bytes)
        pics.append(p)
        want.append([lo, hi])
    for c in (0, 17, 200):  # the imin == imax branch
        pics.append(np.full((H, W, 3), c, dtype=np.uint8))
        want.append([c, c])
    return np.stack(pics), want


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SIZES)
def test_ranges_are_per_picture(gpu_device, H, W):
    """Seven pictures of different byte ranges in ONE batch (a batch-wide min / max fails), three of them constant."""
    images, want_ranges = _ranged_pictures(H, W, seed=H * 7919 + W)
    for type_, coefs, threshold, dil in [("linear", (0.1, 1.0, 0.1), 0.3, 0), ("excess_green", (0, 1, 0), 0.0, 0),
                                         ("linear", (0, 1, 0), 0.15, 3), ("excess_green", (0, 1, 0), 0.0, 5)]:
        got, ranges = entry(images, type_, coefs, threshold, dil, gpu_device)
        assert ranges.tolist() == want_ranges, (type_, "range")  # first: a wrong range is not a wrong filter
        want = oracle.masks_batch(images, type=type_, parameters=coefs, threshold=threshold, dilation_n=dil)
        for q in range(len(images)):
            assert np.array_equal(got[q], want[q]), (type_, dil, "picture", q, want_ranges[q])
    # a single picture of the batch alone gives what it gave in the batch
    alone, r1 = entry(images[2:3], "linear", (0.1, 1.0, 0.1), 0.3, 0, gpu_device)
    assert r1.tolist() == [want_ranges[2]]
    assert np.array_equal(alone[0], oracle.masks(images[2], "linear", (0.1, 1.0, 0.1), 0.3, 0))


def _patterns(H, W, seed):
    """Binary pictures: sparse dots, the four corners and a pixel on each edge, a full row, nothing."""
    rng = np.random.default_rng(seed)
    dots = rng.random((H, W)) < 0.002
    dots[rng.integers(0, H), rng.integers(0, W)] = True
    corners = np.zeros((H, W), dtype=bool)
    for y, x in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1)]:
        corners[y, x] = True
    row = np.zeros((H, W), dtype=bool)
    row[H // 2, :] = True
    one = np.zeros((H, W), dtype=bool)
    one[H // 2, W // 2] = True
    return np.stack([dots, corners, row, one, np.zeros((H, W), dtype=bool)])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SIZES)
def test_dilation_through_the_public_entry(gpu_device, H, W):
    """R = B = 0 and G in {0, 255} under linear [0, 1, 0] > 0.5 has mask = (G == 255): any pattern can be fed."""
    pats = _patterns(H, W, seed=H * 31 + W)
    images = np.zeros(pats.shape + (3,), dtype=np.uint8)
    images[..., 1] = np.where(pats, 255, 0)
    for n in (0, 1, 2, 3, 5, 8, 32):
        got = proc2d.masks_from_images(images, "linear", (0, 1, 0), 0.5, n, device=gpu_device)
        assert got.dtype == np.uint8 and got.shape == pats.shape
        for q, p in enumerate(pats):
            # (an empty picture is constant: min(x, 1) = 0 everywhere, nothing passes)
            want = np.array(255 * (oracle.dilation(p, n) if n else p), dtype=np.uint8)
            assert np.array_equal(got[q], want), (n, "pattern", q)
        # the same pictures through the whole checker (range, filter, threshold, dilation)
        assert np.array_equal(got, oracle.masks_batch(images, type="linear", parameters=(0, 1, 0), threshold=0.5, dilation_n=n))


def _real_pictures():
    from PIL import Image
    names = ["00000_rgb.jpg", "00020_rgb.jpg", "00040_rgb.jpg"]
    return np.stack([np.asarray(Image.open(os.path.join(GOLDEN, n)).convert("RGB"), dtype=np.uint8) for n in names])


@pytest.mark.gpu
@pytest.mark.parametrize("type_,coefs,threshold,dil", [("linear", [0, 1, 0], 0.15, 3), ("excess_green", [0, 1, 0], 0.0, 5)])
def test_real_pictures_both_routes(gpu_device, type_, coefs, threshold, dil):
    """Three pictures of the reference's real_plant scan, the two shipped parameter sets, as one batch; the host-array
    route and the device-tensor route give the same bytes."""
    import torch
    images = _real_pictures()
    assert images.shape[0] == 3 and images.shape[3] == 3 and sorted(images.shape[1:3]) == [1080, 1440]
    want = oracle.masks_batch(images, type=type_, parameters=coefs, threshold=threshold, dilation_n=dil)
    share = [(w != 0).mean() for w in want]
    assert all(0.01 < s < 0.99 for s in share), share  # neither empty nor full
    host = proc2d.masks_from_images(images, type_, coefs, threshold, dil, device=gpu_device)
    assert np.array_equal(host, want)
    dev = proc2d.masks_from_images(torch.from_numpy(images).cuda(gpu_device), type_, coefs, threshold, dil)
    assert dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == want.shape
    assert np.array_equal(dev.cpu().numpy(), want)
    one = proc2d.masks_from_images(images[1], type_, coefs, threshold, dil, device=gpu_device)
    assert one.shape == want[1].shape and np.array_equal(one, want[1])


def _painted(views, seed):
    """The scene's masks as RGB pictures: a green object on a grey, noisy background."""
    rng = np.random.default_rng(seed)
    pics = []
    for _, _, _, m in views:
        H, W = m.shape
        grey = rng.integers(70, 170, size=(H, W, 1)) + rng.integers(-12, 13, size=(H, W, 3))
        green = np.stack([rng.integers(10, 90, size=(H, W)), rng.integers(140, 256, size=(H, W)),
                          rng.integers(10, 90, size=(H, W))], axis=-1)
        pics.append(np.where((m != 0)[..., None], green, grey).astype(np.uint8))
    return np.stack(pics)


@pytest.mark.gpu
def test_hand_over_to_the_carve(gpu_device):
    """Pictures in HBM -> masks in HBM -> carve, no host copy in between; calls right behind one another on one
    stream, and one on another stream, each give their own result (the work buffers are reused in order)."""
    import torch
    shape, origin, vs, views = scenes.make_scene(64, 12, "plant")
    cams = [scenes.camera_dict(K, R, t) for K, R, t, _ in views]
    a, b, c = _painted(views, 1), _painted(views[::-1], 2), _painted(views, 3)[:, ::-1].copy()
    kw = dict(type="excess_green", parameters=[0, 1, 0], threshold=0.1, dilation=1)
    ta, tb, tc = (torch.from_numpy(x).cuda(gpu_device) for x in (a, b, c))
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))  # the uploads
    ma = proc2d.masks_from_images(ta, **kw)
    mb = proc2d.masks_from_images(tb, **kw)  # right behind the first: same stream, same work buffers
    with torch.cuda.stream(side):
        mc = proc2d.masks_from_images(tc, "linear", [0, 1, 0], 0.45, 2)  # another stream of the same device
    vols = masks2d.voxels_from_masks({"plant": ma}, cams, shape, origin, vs, type="carving")
    side.synchronize()
    wa = oracle.masks_batch(a, type="excess_green", parameters=[0, 1, 0], threshold=0.1, dilation_n=1)
    wb = oracle.masks_batch(b, type="excess_green", parameters=[0, 1, 0], threshold=0.1, dilation_n=1)
    wc = oracle.masks_batch(c, type="linear", parameters=[0, 1, 0], threshold=0.45, dilation_n=2)
    assert 0.005 < (wa != 0).mean() < 0.9
    assert np.array_equal(ma.cpu().numpy(), wa)
    assert np.array_equal(mb.cpu().numpy(), wb)
    assert np.array_equal(mc.cpu().numpy(), wc)
    want = oracle_c.carve(shape, origin, vs, [(K, R, t, wa[q]) for q, (K, R, t, _) in enumerate(views)])
    assert vols["plant"].dtype == np.int32 and np.array_equal(vols["plant"], want)
    assert len(np.unique(want)) > 1


@pytest.mark.gpu
def test_work_buffers_grow_are_released_and_come_back(gpu_device):
    """The life of the device's work buffers: a small call, a larger one on another stream that has to replace them
    while the small call's work may still be running, the small call in the larger buffers, a refused call, the
    release, and the small call in buffers allocated anew -- each result is the checker's."""
    import torch
    rng = np.random.default_rng(70)
    small = rng.integers(0, 256, size=(1, 33, 70, 3), dtype=np.uint8)
    large = rng.integers(0, 256, size=(3, 130, 200, 3), dtype=np.uint8)
    kw = dict(type="linear", parameters=[0, 1, 0], threshold=0.9, dilation=2)
    ws, wl = (oracle.masks_batch(x, type="linear", parameters=[0, 1, 0], threshold=0.9, dilation_n=2) for x in (small, large))
    assert 0.05 < (ws != 0).mean() < 0.95 and 0.05 < (wl != 0).mean() < 0.95
    nat.backend().call("sc_masks_release")  # whatever earlier tests left: the first call allocates
    ts, tl = torch.from_numpy(small).cuda(gpu_device), torch.from_numpy(large).cuda(gpu_device)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))  # the uploads
    m1 = proc2d.masks_from_images(ts, **kw)
    with torch.cuda.stream(side):
        m2 = proc2d.masks_from_images(tl, **kw)  # grows: waits for the first call before it frees its buffers
    m3 = proc2d.masks_from_images(ts, **kw)
    with pytest.raises(ValueError, match="finite"):
        proc2d.masks_from_images(ts, **dict(kw, threshold=float("nan")))
    m4 = proc2d.masks_from_images(ts, **kw)
    side.synchronize()
    torch.cuda.current_stream(gpu_device).synchronize()
    assert np.array_equal(m1.cpu().numpy(), ws)
    assert np.array_equal(m2.cpu().numpy(), wl)
    assert np.array_equal(m3.cpu().numpy(), ws)
    assert np.array_equal(m4.cpu().numpy(), ws)
    nat.backend().call("sc_masks_release")
    assert np.array_equal(proc2d.masks_from_images(ts, **kw).cpu().numpy(), ws)
    assert np.array_equal(proc2d.masks_from_images(small, device=gpu_device, **kw), ws)  # the host route
