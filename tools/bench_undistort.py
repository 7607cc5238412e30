#!/usr/bin/env python3
"""Timing of the lens correction: 72 seeded 1080 x 1440 RGB pictures of uniform random bytes through the
`barrel` camera of tests/undistort_oracle.py:
  (a) device pictures -> device pictures (``proc2d.undistort`` on a CUDA tensor), HIP events around the repetitions
      after warm-up, with the byte bound (3 H W read + 3 H W written per picture, at 8 TB/s) and its share;
  (b) host pictures -> host pictures (the same function on a NumPy array), host clock;
  (c) the checker (tests/undistort_oracle.py, NumPy) over the same pictures on one host thread, picture by picture as
      the reference's task runs; the pictures of (a) and (b) are compared with it bit for bit in the same run;
  (d) a plain device copy of the same tensor (``out.copy_(images)``), HIP events, same session.
The bar: (a) <= 2 x (d).  One JSON line, also written to --out.  No GPU, no figures: there is no fallback."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes per second (spec)


def _events_ms(torch, device, reps, fn):
    torch.cuda.synchronize(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=72)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1440)
    ap.add_argument("--camera", default="barrel")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true", help="skip (c) and the comparison (profiling runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_bench.json"))
    a = ap.parse_args()
    import torch
    from plant3dvision_amd import proc2d
    from tests import undistort_oracle as oracle
    V, H, W = a.views, a.height, a.width
    imgs = oracle.picture(H, W, V=V, seed=7)
    mtx, dist = oracle.camera(a.camera, H, W)
    dev_imgs = torch.from_numpy(imgs).cuda(a.device)
    copy_out = torch.empty_like(dev_imgs)
    res = {}

    def correct():
        res["dev"] = proc2d.undistort(dev_imgs, mtx, dist)

    for _ in range(a.warmup):
        correct()
        copy_out.copy_(dev_imgs)
    # (a) and (d) alternate, three rounds each: the least of each is reported, all rounds are kept
    rounds = [(_events_ms(torch, a.device, a.reps, correct), _events_ms(torch, a.device, a.reps, lambda: copy_out.copy_(dev_imgs)))
              for _ in range(3)]
    dev_ms, copy_ms = min(r[0] for r in rounds), min(r[1] for r in rounds)
    host_ms = host_out = None
    for _ in range(1 + a.host_reps if a.host_reps else 0):  # the first one warms up
        t0 = time.perf_counter()
        host_out = proc2d.undistort(imgs, mtx, dist, device=a.device)
        dt = (time.perf_counter() - t0) * 1e3
        host_ms = dt if host_ms is None else min(host_ms, dt)
    bound_ms = V * 6 * H * W / HBM_PEAK * 1e3
    out = {"views": V, "height": H, "width": W, "camera": a.camera, "reps": a.reps, "byte_bound_ms": bound_ms,
           "device_to_device_ms": dev_ms, "device_copy_ms": copy_ms, "rounds_ms": rounds,
           "share_of_byte_bound": bound_ms / dev_ms, "ratio_to_copy": dev_ms / copy_ms, "bar_met": bool(dev_ms <= 2 * copy_ms),
           "host_to_host_ms": host_ms}
    if not a.no_cpu:
        got = res["dev"].cpu().numpy()
        same_dev = same_host = True
        K, d = oracle.intrinsics(mtx, dist)
        cpu_s = 0.0
        for q in range(V):  # picture by picture, the map computed every time, as cv2.undistort does per call
            t0 = time.perf_counter()
            want = oracle.undistort(imgs[q], mtx, dist)
            cpu_s += time.perf_counter() - t0
            same_dev = same_dev and bool(np.array_equal(got[q], want))
            same_host = same_host and (host_out is None or bool(np.array_equal(host_out[q], want)))
        iu, iv = oracle.umap(H, W, K, d)
        out.update({"checker_one_thread_ms": cpu_s * 1e3, "speedup_device": cpu_s * 1e3 / dev_ms,
                    "speedup_host_route": cpu_s * 1e3 / host_ms if host_ms else None,
                    "account": oracle.account(H, W, iu, iv, K, d),
                    "bit_identical_device": same_dev, "bit_identical_host_route": same_host})
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not (out.get("bit_identical_device", True) and out.get("bit_identical_host_route", True)):
        sys.exit("pictures differ from the checker")


if __name__ == "__main__":
    main()
