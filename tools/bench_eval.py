#!/usr/bin/env python3
"""Timing of the evaluation counts: ``metrics.voxel_confusion`` at 512^3 and 256^3 x 6 classes (float32
predictions, uint8 ground truth, the first class the background) and ``metrics.compare_mask_stacks`` on 72 masks of
1080 x 1440 at ``dilation_amount`` 0 and 3:
  (a) device tensors -> counts, HIP events around the repetitions after warm-up (every call ends in the read-back of
      its counts, so the events span whole calls);
  (b) host arrays -> counts, host clock, the slabs' copies included;
  (c) the NumPy / SciPy checker (tests/evaluation_oracle.py, the reference's lines restated) on the same box -- for
      the volumes at 128^3 and 256^3 ONLY: at 512^3 x 6 its float64 temporaries pass 12 GB, which does not fit
      comfortably beside everything else; ``checker_512_extrapolated_s`` is 8 x the 256^3 time, not a measurement.
The counts of (a) and (b) are compared with the checker's wherever the checker ran.  Also: the bytes the volume kernel
must read (every prediction and every non-background ground-truth value once) over the time of (a), as bytes/s and as
a share of the 6.3 TB/s a streaming read achieves on this device -- a whole-call rate: launch, counter read-back and
synchronisation are inside it.  One JSON line, also written to ``--out``.  No GPU, no figures: there is no fallback."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ACHIEVABLE_HBM = 6.3e12  # bytes/s, a float4 streaming read


def volumes(n, classes, seed):
    """Averaging-like predictions (most voxels near 0, a few clear winners) and 0 / 1 ground truths."""
    rng = np.random.default_rng(seed)
    labels = ["background"] + [f"organ{q}" for q in range(1, classes)]
    truth = rng.integers(0, classes, size=(n, n, n), dtype=np.uint8)
    voxels, gts = {}, {}
    for q, k in enumerate(labels):
        noise = rng.random((n, n, n), dtype=np.float32) * np.float32(0.05)
        voxels[k] = np.where(truth == q, np.float32(0.9), np.float32(0.0)) + noise
        gts[k] = (truth == q).astype(np.uint8)
        flip = rng.random((n, n, n), dtype=np.float32) < 0.05
        gts[k][flip] ^= 1
    return voxels, gts


def mask_stacks(n, H, W, seed):
    rng = np.random.default_rng(seed)
    gt = np.zeros((n, H, W), np.uint8)
    pred = np.zeros((n, H, W), np.uint8)
    for v in range(n):  # a few blobs per picture, the prediction shifted by a few pixels
        for _ in range(6):
            y, x, r = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(20, 120))
            gt[v, max(0, y - r):y + r, max(0, x - r):x + r] = 255
            pred[v, max(0, y - r + 3):y + r + 3, max(0, x - r - 2):x + r - 2] = 255
    return gt, pred


def timed_device(fn, warmup, reps, device):
    import torch
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps, out


def timed_host(fn, reps):
    best = out = None
    for _ in range(1 + reps):  # the first one warms up
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--checker-sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--masks", type=int, nargs=3, default=[72, 1080, 1440], metavar=("N", "H", "W"))
    ap.add_argument("--dilations", type=int, nargs="+", default=[0, 3])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true", help="skip (c) and the comparisons (profiling runs)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "eval_bench.json"))
    a = ap.parse_args()
    import torch
    from plant3dvision_amd import metrics
    from tests import evaluation_oracle as oracle
    dev = f"cuda:{a.device}"
    out = {"classes": a.classes, "reps": a.reps, "pred_dtype": "float32", "gt_dtype": "uint8", "volumes": {}, "masks": {},
           "checker_note": "the NumPy checker runs at the --checker-sizes only: 512^3 x 6 classes needs more than 12 GB of float64 temporaries"}
    equal = True
    for n in sorted(set(a.sizes) | (set() if a.no_cpu else set(a.checker_sizes))):
        voxels, gts = volumes(n, a.classes, seed=n)
        res = {}
        if n in a.sizes:
            tv = {k: torch.from_numpy(v).to(dev) for k, v in voxels.items()}
            tg = {k: torch.from_numpy(v).to(dev) for k, v in gts.items()}
            res["device_to_counts_ms"], got = timed_device(lambda: metrics.voxel_confusion(tv, tg), a.warmup, a.reps, a.device)
            res["device_with_projections_ms"], _ = timed_device(lambda: metrics.voxel_confusion(tv, tg, projections=True), 1,
                                                                max(1, a.reps // 4), a.device)
            del tv, tg
            res["host_to_counts_ms"], host = timed_host(lambda: metrics.voxel_confusion(voxels, gts, device=a.device), a.host_reps)
            res["host_equals_device"] = host == got
            equal = equal and res["host_equals_device"]
            need = n ** 3 * (a.classes * 4 + (a.classes - 1) * 1)  # every value once; the background's ground truth never
            res["bytes_to_read"] = need
            res["bytes_per_s_whole_call"] = need / (res["device_to_counts_ms"] * 1e-3)
            res["share_of_achievable_hbm"] = res["bytes_per_s_whole_call"] / ACHIEVABLE_HBM
        if not a.no_cpu and n in a.checker_sizes:
            t0 = time.perf_counter()
            want = oracle.voxel_histograms(voxels, gts)
            res["checker_s"] = time.perf_counter() - t0
            if n in a.sizes:
                res["equal_to_checker_device"], res["equal_to_checker_host_route"] = got == want, host == want
                equal = equal and res["equal_to_checker_device"] and res["equal_to_checker_host_route"]
                res["checker_over_device"] = res["checker_s"] * 1e3 / res["device_to_counts_ms"]
        out["volumes"][f"{n}^3"] = res
        del voxels, gts
    big = max(a.checker_sizes) if not a.no_cpu else None
    if big and f"{big}^3" in out["volumes"] and "512^3" in out["volumes"]:
        out["volumes"]["512^3"]["checker_512_extrapolated_s"] = out["volumes"][f"{big}^3"]["checker_s"] * (512 / big) ** 3

    n, H, W = a.masks
    gt, pred = mask_stacks(n, H, W, seed=7)
    tgt, tpred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    for k in a.dilations:
        res = {"pictures": n, "H": H, "W": W}
        res["device_to_counts_ms"], got = timed_device(lambda: metrics.compare_mask_stacks(tgt, tpred, k), a.warmup, a.reps, a.device)
        res["host_to_counts_ms"], host = timed_host(lambda: metrics.compare_mask_stacks(gt, pred, k, device=a.device), a.host_reps)
        res["host_equals_device"] = bool(np.array_equal(host, got))
        equal = equal and res["host_equals_device"]
        if not a.no_cpu:
            t0 = time.perf_counter()
            want = oracle.mask_stack_counts(gt, pred, k)
            res["checker_s"] = time.perf_counter() - t0
            res["equal_to_checker_device"] = bool(np.array_equal(got, want))
            res["equal_to_checker_host_route"] = bool(np.array_equal(host, want))
            equal = equal and res["equal_to_checker_device"] and res["equal_to_checker_host_route"]
            res["checker_over_device"] = res["checker_s"] * 1e3 / res["device_to_counts_ms"]
        out["masks"][f"dilation_{k}"] = res
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not equal:
        sys.exit("counts differ")


if __name__ == "__main__":
    main()
