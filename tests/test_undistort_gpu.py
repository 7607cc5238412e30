"""GPU: the lens correction (``sc_undistort_rgb`` / ``proc2d.undistort``) against the checker
(tests/undistort_oracle.py), bit for bit: ``np.array_equal``, no tolerance."""
import os

import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import proc2d
from tests import proc2d_oracle
from tests import undistort_oracle as oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_plant_rgb")


def entry(images, mtx, dist, device):
    """``sc_undistort_rgb`` itself on host arrays: (pictures, iu, iv)."""
    images = np.ascontiguousarray(images)
    V, H, W, _ = images.shape
    K, d = oracle.intrinsics(mtx, dist)
    b = nat.backend()
    out = np.full(images.shape, 0x5a, dtype=np.uint8)
    umap = np.full((H, W, 2), 0x5a5a5a5a, dtype=np.int32)
    rc = b.call("sc_undistort_rgb", nat.addr(images), 0, V, H, W, nat.addr(K), nat.addr(d), device, 0, nat.addr(out), 0,
                nat.addr(umap))
    assert rc == nat.SC_OK, b.string(b.call("sc_undistort_last_error"))
    return out, umap[..., 0], umap[..., 1]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", oracle.SHAPES)
@pytest.mark.parametrize("name", oracle.CAMERAS)
def test_every_camera_on_every_shape(gpu_device, name, H, W):
    images = oracle.picture(H, W, V=3)
    mtx, dist = oracle.camera(name, H, W)
    K, d = oracle.intrinsics(mtx, dist)
    iu, iv = oracle.umap(H, W, K, d)
    got, giu, giv = entry(images, mtx, dist, gpu_device)
    print(name, (H, W), "map entries that differ:", int(np.count_nonzero((giu != iu) | (giv != iv))))
    assert np.array_equal(giu, iu) and np.array_equal(giv, iv)  # first: a wrong map is not a wrong remap
    want = oracle.remap(images, iu, iv)
    print(name, (H, W), "bytes that differ:", int(np.count_nonzero(got != want)))
    assert np.array_equal(got, want)


def _real_pictures():
    from PIL import Image
    names = ["00000_rgb.jpg", "00020_rgb.jpg", "00040_rgb.jpg"]
    return np.stack([np.asarray(Image.open(os.path.join(GOLDEN, n)).convert("RGB"), dtype=np.uint8) for n in names])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["real", "barrel"])
def test_real_pictures_both_routes(gpu_device, name):
    """Three pictures of the reference's real_plant scan as one batch; the host-array route and the device-tensor route
    give the same bytes."""
    import torch
    images = _real_pictures()
    H, W = images.shape[1:3]
    assert images.shape[0] == 3 and images.shape[3] == 3 and sorted((H, W)) == [1080, 1440]
    mtx, dist = oracle.camera(name, H, W)
    want = oracle.undistort(images, mtx, dist)
    assert (want != images).any(axis=-1).mean() > 0.02  # not a copy (`real` moves a photograph's pixels by little)
    host = proc2d.undistort(images, mtx, dist, device=gpu_device)
    assert host.dtype == np.uint8 and np.array_equal(host, want)
    dev = proc2d.undistort(torch.from_numpy(images).cuda(gpu_device), mtx, dist)
    assert dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == want.shape
    assert np.array_equal(dev.cpu().numpy(), want)
    one = proc2d.undistort(images[1], mtx, dist[:4], device=gpu_device)
    assert one.shape == want[1].shape and np.array_equal(one, want[1])


@pytest.mark.gpu
def test_unmapped_pixels(gpu_device):
    """k1 = 1e300 at 7 x 13: every pixel but the one on the optical centre overflows -- zeros, INT32_MIN, no fault."""
    H, W = 7, 13
    images = oracle.picture(H, W, V=2, seed=3)
    mtx = np.array([[10, 0, 6], [0, 10, 3], [0, 0, 1]], dtype=np.float64)
    dist = np.array([1e300, 0, 0, 0], dtype=np.float64)
    iu, iv = oracle.umap(H, W, *oracle.intrinsics(mtx, dist))
    lost = (iu == oracle.INT32_MIN) & (iv == oracle.INT32_MIN)
    assert lost.sum() == H * W - 1 and not lost[3, 6]
    got, giu, giv = entry(images, mtx, dist, gpu_device)
    assert np.array_equal(giu, iu) and np.array_equal(giv, iv)
    assert (got[:, lost] == 0).all() and np.array_equal(got[:, 3, 6], images[:, 3, 6])
    assert np.array_equal(proc2d.undistort(images, mtx, dist, device=gpu_device), oracle.undistort(images, mtx, dist))


@pytest.mark.gpu
def test_a_picture_alone_and_in_a_batch(gpu_device):
    """V = 1 against the same picture inside a batch of 5 (the last picture of the batch: the one whose last bytes end
    the buffer)."""
    H, W = 61, 1031
    images = oracle.picture(H, W, V=5, seed=9)
    mtx, dist = oracle.camera("pincushion", H, W)
    batch = proc2d.undistort(images, mtx, dist, device=gpu_device)
    assert np.array_equal(batch, oracle.undistort(images, mtx, dist))
    for q in (0, 2, 4):
        assert np.array_equal(proc2d.undistort(images[q], mtx, dist, device=gpu_device), batch[q]), q
        assert np.array_equal(proc2d.undistort(images[q:q + 1], mtx, dist, device=gpu_device)[0], batch[q]), q


@pytest.mark.gpu
def test_hand_over_to_the_masks(gpu_device):
    """Pictures in HBM -> corrected pictures in HBM -> masks, on one stream with no host copy in between."""
    import torch
    H, W = 270, 360
    images = oracle.picture(H, W, V=4, seed=21)
    mtx, dist = oracle.camera("barrel", H, W)
    kw = dict(type="excess_green", parameters=[0, 1, 0], threshold=0.3, dilation=1)
    t = torch.from_numpy(images).cuda(gpu_device)
    masks = proc2d.masks_from_images(proc2d.undistort(t, mtx, dist), **kw)
    flat = oracle.undistort(images, mtx, dist)
    want = proc2d_oracle.masks_batch(flat, type="excess_green", parameters=[0, 1, 0], threshold=0.3, dilation_n=1)
    assert 0.2 < (want != 0).mean() < 0.8
    assert np.array_equal(masks.cpu().numpy(), want)
    assert not np.array_equal(want, proc2d_oracle.masks_batch(images, type="excess_green", parameters=[0, 1, 0], threshold=0.3,
                                                              dilation_n=1))  # the correction shows in the masks


@pytest.mark.gpu
def test_two_streams_and_the_work_buffer_grows_is_released_and_comes_back(gpu_device):
    """A small call, a larger one on another stream that has to replace the map while the small call's work may still
    be running, the small call in the larger buffer, a refused call, the release, and the small call in a buffer
    allocated anew -- each result is the checker's."""
    import torch
    small, large = oracle.picture(33, 70, V=2, seed=70), oracle.picture(130, 203, V=9, seed=71)
    cs, cl = oracle.camera("k3", 33, 70), oracle.camera("pincushion", 130, 203)
    ws, wl = oracle.undistort(small, *cs), oracle.undistort(large, *cl)
    nat.backend().call("sc_undistort_release")  # whatever earlier tests left: the first call allocates
    ts, tl = torch.from_numpy(small).cuda(gpu_device), torch.from_numpy(large).cuda(gpu_device)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))  # the uploads
    m1 = proc2d.undistort(ts, *cs)
    with torch.cuda.stream(side):
        m2 = proc2d.undistort(tl, *cl)  # grows: waits for the first call before it frees its buffer
    m3 = proc2d.undistort(ts, *cs)
    with pytest.raises(ValueError, match="finite"):
        proc2d.undistort(ts, cs[0], [float("nan"), 0, 0, 0])
    m4 = proc2d.undistort(ts, *cs)
    side.synchronize()
    torch.cuda.current_stream(gpu_device).synchronize()
    assert np.array_equal(m1.cpu().numpy(), ws)
    assert np.array_equal(m2.cpu().numpy(), wl)
    assert np.array_equal(m3.cpu().numpy(), ws)
    assert np.array_equal(m4.cpu().numpy(), ws)
    nat.backend().call("sc_undistort_release")
    assert np.array_equal(proc2d.undistort(ts, *cs).cpu().numpy(), ws)
    assert np.array_equal(proc2d.undistort(small, *cs, device=gpu_device), ws)  # the host route
