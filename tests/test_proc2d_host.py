"""CPU: the mask producer's checker (tests/proc2d_oracle.py), the argument checks of ``sc_masks_from_rgb`` (no device
call) and the ``Masks`` task logic ``tasks.proc2d.masks_run`` with an injected ``masks_fn``."""
import numpy as np
import pytest

from plant3dvision_amd import _native as nat
from plant3dvision_amd import masks2d
from plant3dvision_amd import proc2d
from plant3dvision_amd.tasks import proc2d as task
from tests import proc2d_oracle as oracle


def test_checker_sums_the_channels_left_to_right():
    """``img.sum(axis=2)`` is ``(r' + g') + b'`` on every colour: a NumPy that adds in another order shows here."""
    norm = oracle.normalised(oracle.all_colours())
    assert norm.min() == 0.0 and norm.max() == 1.0
    s = norm.sum(axis=2)
    assert np.array_equal(s, (norm[:, :, 0] + norm[:, :, 1]) + norm[:, :, 2])
    assert np.count_nonzero(s != norm[:, :, 0] + (norm[:, :, 1] + norm[:, :, 2])) > 0  # the order matters


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_checker_dilation_of_one_pixel_is_the_composed_footprint(n):
    """Pins the direction of p - o: the T-shaped elements (n = 8) are not symmetric."""
    series = masks2d.disk_series(n)
    counts = {name: reps for name, reps in series}
    a, b, c = counts.get("t0", 0), counts.get("diamond", 0), counts.get("square", 0)
    assert all(counts.get(k, 0) == a for k in ("t90", "t180", "t270"))
    want = masks2d._compose((a, b, c))
    r = want.shape[0] // 2
    img = np.zeros((2 * r + 9, 2 * r + 11), dtype=bool)
    cy, cx = r + 4, r + 5
    img[cy, cx] = True
    got = oracle.dilation(img, n)
    assert np.array_equal(got[cy - r:cy + r + 1, cx - r:cx + r + 1], want)
    assert got.sum() == want.sum()
    if n == 8:
        assert a > 0  # the series of 8 does hold T-shaped elements


def test_checker_structure_sets_p_plus_o():
    """One pixel at p dilated by one footprint sets exactly the pixels p + o (out[q] = OR_o in[q - o])."""
    from scipy import ndimage
    for name, offsets in masks2d._FOOTPRINTS.items():
        img = np.zeros((5, 5), dtype=bool)
        img[2, 2] = True
        want = np.zeros_like(img)
        for dy, dx in offsets:
            want[2 + dy, 2 + dx] = True
        assert np.array_equal(ndimage.binary_dilation(img, structure=oracle.structure(name)), want), name


def test_dilation_steps_expand_the_series():
    assert proc2d.dilation_steps(1).tolist() == [nat.SC_FOOT["diamond"]]
    for n in (2, 3, 5, 8, 32):
        steps = proc2d.dilation_steps(n)
        assert steps.dtype == np.uint8 and steps.size == sum(reps for _, reps in masks2d.disk_series(n)) <= 32
    assert list(nat.SC_FOOT) == list(masks2d._FOOTPRINTS)


def _call(rgb=None, on_dev=0, V=1, H=2, W=2, filt=0, coefs=(0.0, 1.0, 0.0), thr=0.3, steps=(), nsteps=None, out=True,
          device=0):
    b = nat.backend()
    img = np.zeros((2, 2, 3), dtype=np.uint8) if rgb is None else rgb
    c = None if coefs is None else np.asarray(coefs, dtype=np.float64)
    st = np.asarray(steps, dtype=np.uint8)
    o = np.full(16, 7, dtype=np.uint8)
    rc = b.call("sc_masks_from_rgb", nat.addr(img) if img is not False else 0, on_dev, V, H, W, filt,
                nat.addr(c) if c is not None else 0, thr, nat.addr(st) if st.size else 0,
                st.size if nsteps is None else nsteps, device, 0, nat.addr(o) if out else 0, 0, 0)
    assert (o == 7).all()  # nothing was written
    return rc, b.string(b.call("sc_masks_last_error"))


def test_argument_errors_do_not_need_a_device():
    cases = [
        (dict(rgb=False), "null"), (dict(out=False), "null"), (dict(coefs=None), "null"),
        (dict(V=0), "at least 1"), (dict(H=0), "at least 1"), (dict(W=-3), "at least 1"),
        (dict(H=32768, W=32768), "2^31"), (dict(H=1, W=715827883), "2^31"),
        (dict(filt=2), "filter"), (dict(filt=-1), "filter"),
        (dict(coefs=(0.0, np.nan, 0.0)), "finite"), (dict(coefs=(np.inf, 0.0, 0.0)), "finite"),
        (dict(thr=np.nan), "threshold"), (dict(thr=-np.inf), "threshold"),
        (dict(nsteps=-1), "nsteps"), (dict(steps=[4] * 33), "nsteps"), (dict(nsteps=2), "steps"),
        (dict(steps=[0, 6]), "step ids"), (dict(steps=[255]), "step ids"),
        (dict(device=-1), "device"), (dict(device=64), "device"),
    ]
    for kw, word in cases:
        rc, msg = _call(**kw)
        assert rc == nat.SC_ERR_INVALID and word in msg, (kw, rc, msg)


def test_python_entry_refuses_what_the_kernels_do_not_take():
    with pytest.raises(Exception, match="Unknown masking type 'hsv'!"):
        proc2d.masks_from_images(np.zeros((2, 2, 3), np.uint8), type="hsv")
    for bad in (np.zeros((2, 2, 3), np.float64), np.zeros((2, 2, 4), np.uint8), np.zeros((2, 2), np.uint8),
                np.zeros((1, 1, 2, 2, 3), np.uint8), np.zeros((0, 2, 3), np.uint8)):
        with pytest.raises(ValueError):
            proc2d.masks_from_images(bad)
    with pytest.raises(ValueError):
        proc2d.masks_from_images(np.zeros((2, 2, 3), np.uint8), parameters=(1, 2))
    with pytest.raises(ValueError, match="finite"):
        proc2d.masks_from_images(np.zeros((2, 2, 3), np.uint8), threshold=float("nan"))
    with pytest.raises(ValueError):
        proc2d.masks_from_images(np.zeros((2, 2, 3), np.uint8), dilation=33)


class _File:
    def __init__(self, id, array):
        self.id, self.array = id, array


def _checker_fn(calls):
    def fn(batch, type, parameters, threshold, dilation):
        calls.append(batch.shape)
        return oracle.masks_batch(batch, type=type, parameters=parameters, threshold=threshold, dilation_n=dilation)
    return fn


def test_masks_run_keeps_ids_and_order_and_batches_by_size():
    rng = np.random.default_rng(5)
    sizes = [(6, 9), (4, 5), (6, 9), (6, 9), (4, 5)]
    files = [_File(f"{q:05d}_rgb", rng.integers(0, 256, size=s + (3,), dtype=np.uint8)) for q, s in enumerate(sizes)]
    calls = []
    out = task.masks_run(files, "linear", [0.1, 1.0, 0.1], 0.3, 2, masks_fn=_checker_fn(calls))
    assert sorted(calls) == [(2, 4, 5, 3), (3, 6, 9, 3)]
    assert [o[0] for o in out] == [f.id for f in files]
    for f, (_, mask, md) in zip(files, out):
        want = oracle.masks(f.array, "linear", [0.1, 1.0, 0.1], 0.3, 2)
        assert mask.dtype == np.uint8 and np.array_equal(mask, want)
        assert md == {"Masks": {"upstream_task": "Undistorted", "filter": "linear", "threshold": 0.3, "dilation": 2,
                                "linear_coeff": [0.1, 1.0, 0.1]}}
    assert out[0][2]["Masks"] is not out[1][2]["Masks"]


def test_masks_run_metadata_follows_the_reference():
    files = [_File("a", np.arange(48, dtype=np.uint8).reshape(4, 4, 3))]
    fn = _checker_fn([])
    (_, _, md), = task.masks_run(files, "excess_green", [0, 1, 0], 0.0, 5, masks_fn=fn)
    assert md == {"Masks": {"upstream_task": "Undistorted", "filter": "excess_green", "threshold": 0.0, "dilation": 5}}
    (_, _, md), = task.masks_run(files, "excess_green", [0, 1, 0], 0.0, 0, query={}, masks_fn=fn)
    assert "query" not in md["Masks"]
    (_, _, md), = task.masks_run(files, "linear", (0, 1, 0), 0.15, 3, query={"channel": "rgb"},
                                 upstream_task="ImagesFilesetExists", masks_fn=fn)
    assert md == {"Masks": {"upstream_task": "ImagesFilesetExists", "filter": "linear", "threshold": 0.15, "dilation": 3,
                            "linear_coeff": [0, 1, 0], "query": {"channel": "rgb"}}}
    with pytest.raises(Exception, match="Unknown masking type 'green'!"):
        task.masks_run(files, "green", [0, 1, 0], 0.3, 0, masks_fn=fn)
    assert task.MASKS_DEFAULTS == dict(type="linear", parameters=[0, 1, 0], threshold=0.3, dilation=0)
