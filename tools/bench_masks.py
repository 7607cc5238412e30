#!/usr/bin/env python3
"""Timing of the geometric pipeline's mask producer: 72 seeded 1080 x 1440 RGB pictures -> masks, for the
two shipped parameter sets -- linear [0, 1, 0] > 0.15, dilation 3 (geom_pipe_real.toml) and excess_green > 0.0,
dilation 5 (training_seg.toml):
  (a) device pictures -> device masks (``proc2d.masks_from_images`` on a CUDA tensor), HIP events around the
      repetitions after warm-up, with the byte bound (2 x 3 H W read + H W written per picture, at 8 TB/s) and its share;
  (b) host pictures -> host masks (the same function on a NumPy array), host clock;
  (c) the reference chain in NumPy / SciPy (tests/proc2d_oracle.py) over the same pictures on one thread, which is how
      the reference runs it; the masks of (a) are compared with it bit for bit in the same run.
One JSON line.  No GPU, no figures: there is no fallback."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETS = {"linear_010_t0.15_d3": dict(type="linear", parameters=[0, 1, 0], threshold=0.15, dilation=3),
        "excess_green_t0.0_d5": dict(type="excess_green", parameters=[0, 1, 0], threshold=0.0, dilation=5)}
HBM_PEAK = 8.0e12  # bytes per second (spec)


def pictures(n, H, W, seed=7):
    """A plant-like green object (a stem and a few leaves that turn with the view) on a dark grey, noisy background."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((n, H, W, 3), dtype=np.uint8)
    for q in range(n):
        a = 2 * np.pi * q / n
        obj = (np.abs(xx - W / 2) < 6 + 3 * np.cos(a)) & (yy > 0.35 * H)
        for k in range(7):
            cy, cx = H * (0.3 + 0.08 * k), W / 2 + 0.22 * W * np.cos(a + 0.9 * k)
            ry, rx = 0.04 * H, 0.02 * W + 0.09 * W * abs(np.sin(a + 0.9 * k))
            obj |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
        # a dark backdrop, slightly magenta, with per-channel noise: under one per cent of it passes excess_green > 0
        grey = rng.integers(5, 30, size=(H, W, 1)) + rng.integers(0, 5, size=(H, W, 3)) + np.array([4, 0, 3])
        green = np.stack([rng.integers(20, 90, size=(H, W)), rng.integers(130, 256, size=(H, W)),
                          rng.integers(10, 80, size=(H, W))], axis=-1)
        out[q] = np.where(obj[..., None], green, grey).astype(np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=72)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1440)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true", help="skip (c) and the comparison (profiling runs)")
    a = ap.parse_args()
    import torch
    from plant3dvision_amd import proc2d
    from tests import proc2d_oracle
    V, H, W = a.views, a.height, a.width
    imgs = pictures(V, H, W)
    dev_imgs = torch.from_numpy(imgs).cuda(a.device)
    bound_s = V * (2 * 3 * H * W + H * W) / HBM_PEAK
    out = {"views": V, "height": H, "width": W, "reps": a.reps, "byte_bound_ms": bound_s * 1e3, "sets": {}}
    for name, kw in SETS.items():
        for _ in range(a.warmup):
            masks = proc2d.masks_from_images(dev_imgs, **kw)
        torch.cuda.synchronize(a.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            masks = proc2d.masks_from_images(dev_imgs, **kw)
        e1.record()
        e1.synchronize()
        dev_ms = e0.elapsed_time(e1) / a.reps
        host_ms = host_masks = None
        for _ in range(1 + a.host_reps if a.host_reps else 0):  # the first one warms up
            t0 = time.perf_counter()
            host_masks = proc2d.masks_from_images(imgs, device=a.device, **kw)
            dt = (time.perf_counter() - t0) * 1e3
            host_ms = dt if host_ms is None else min(host_ms, dt)
        if a.no_cpu:
            out["sets"][name] = {"device_to_device_ms": dev_ms, "share_of_byte_bound": bound_s * 1e3 / dev_ms,
                                 "host_to_host_ms": host_ms}
            continue
        t0 = time.perf_counter()
        want = proc2d_oracle.masks_batch(imgs, type=kw["type"], parameters=kw["parameters"], threshold=kw["threshold"],
                                         dilation_n=kw["dilation"])
        cpu_ms = (time.perf_counter() - t0) * 1e3
        got = masks.cpu().numpy()
        out["sets"][name] = {
            "device_to_device_ms": dev_ms, "share_of_byte_bound": bound_s * 1e3 / dev_ms,
            "host_to_host_ms": host_ms, "numpy_scipy_one_thread_ms": cpu_ms,
            "speedup_device": cpu_ms / dev_ms, "speedup_host_route": cpu_ms / host_ms if host_ms else None,
            "set_share": float((want != 0).mean()),
            "bit_identical_device": bool(np.array_equal(got, want)),
            "bit_identical_host_route": host_masks is None or bool(np.array_equal(host_masks, want))}
    print(json.dumps(out))
    if not all(s.get("bit_identical_device", True) and s.get("bit_identical_host_route", True) for s in out["sets"].values()):
        sys.exit("masks differ from the checker")


if __name__ == "__main__":
    main()
