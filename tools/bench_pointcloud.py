#!/usr/bin/env python3
"""Timing of the multiclass ``PointCloud`` task at 512^3 and 256^3 x 6 classes of float32 (the first class
the background: as many prediction bytes as tools/bench_eval.py reads; every organ three balls with a linear rim and a
little noise, so that a class's cloud is a surface and not every voxel of a noise volume):
  (a) device tensors -> winner volume (``proc3d.select_classes``), HIP events around the repetitions after warm-up
      (every call ends in the read-back of its counts, so the events span whole calls); the kernel alone comes from a
      ``rocprofv3 --kernel-trace --stats`` run of this tool (``--only-device``), whose CSV ``--kernel-stats`` merges in;
  (b) host arrays -> winner volume, host clock, the slabs' copies both ways included;
  (c) the whole ``tasks.proc3d.point_cloud_run``, device tensors to the labelled cloud on the host, host clock;
  (d) the literal NumPy lines (tests/pointcloud_oracle.py) on the same box -- at 128^3 and 256^3 ONLY: at 512^3 x 6
      their float64 temporaries pass 12 GB.  Winners and point counts of (a), (b), (c) are compared with (d) wherever
      it ran (the clouds of (d) come from oracle/vol2pcd_oracle.py).
Throughput bar (the issue of this feature): the bytes the kernel must read (every class value once) over the time of (a)
at 512^3, against ``bytes_per_s_whole_call`` of tools/bench_eval.py measured on the same box in the same session
(``--eval-json``, by default profiles/eval_bench.json as that run left it): at least 0.9 of it.  Both figures go into the
JSON; falling short is reported, the exit status stays 0 for it.  One JSON line, also written to ``--out``.  No GPU, no
figures: there is no fallback."""
import argparse, csv, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ACHIEVABLE_HBM = 6.3e12  # bytes/s, a float4 streaming read
PARAMS = dict(background_prior=1.0, min_contrast=10.0, min_score=0.2)


def scene(n, classes, seed):
    """``{label: float32 [n, n, n]}``: per organ three balls (core 1, linear rim) plus noise below 0.02; the background
    is 1 - the greatest ball profile of the voxel.  Built from 1-D squared distances: no [n, n, n, 3] grid."""
    rng = np.random.default_rng(seed)
    ax = np.arange(n, dtype=np.float32)
    labels = ["background"] + [f"organ{q}" for q in range(1, classes)]
    out, top = {}, np.zeros((n, n, n), np.float32)
    for k in labels[1:]:
        f = np.zeros((n, n, n), np.float32)
        for _ in range(3):
            c = rng.uniform(0.15, 0.85, 3) * n
            core, rim = rng.uniform(0.05, 0.10) * n, rng.uniform(0.02, 0.04) * n
            d = np.sqrt(((ax - np.float32(c[0])) ** 2)[:, None, None] + ((ax - np.float32(c[1])) ** 2)[None, :, None]
                        + ((ax - np.float32(c[2])) ** 2)[None, None, :])
            np.maximum(f, np.clip((np.float32(core + rim) - d) / np.float32(rim), 0.0, 1.0), out=f)
        np.maximum(top, f, out=top)
        out[k] = f + rng.random((n, n, n), dtype=np.float32) * np.float32(0.02)
    return {"background": np.float32(1.0) - top, **out}


def kernel_ms(path):
    """Mean duration of select_classes_kernel per call in a rocprofv3 --stats CSV, by the size of the launch unknown:
    the mean over all its calls (run the traced process at ONE size)."""
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "select_classes_kernel" in row["Name"]:
                return float(row["AverageNs"]) * 1e-6, int(row["Calls"])
    return None, 0


def main():
    from bench_eval import timed_device, timed_host
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--checker-sizes", type=int, nargs="+", default=[128, 256], help="(d); the device legs run at these sizes too")
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--level-set-value", type=float, default=1.0)
    ap.add_argument("--only-device", action="store_true", help="(a) only, no comparison: the run rocprofv3 traces")
    ap.add_argument("--no-cpu", action="store_true", help="skip (d) and the comparisons")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --kernel-trace --stats CSV of an --only-device run at --kernel-stats-size")
    ap.add_argument("--kernel-stats-size", type=int, default=512)
    ap.add_argument("--eval-json", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointcloud_bench.json"))
    a = ap.parse_args()
    import torch
    from plant3dvision_amd import proc3d
    from plant3dvision_amd.tasks import proc3d as task
    dev = f"cuda:{a.device}"
    origin, vs = np.zeros(3), 1.0
    out = {"classes": a.classes, "reps": a.reps, "dtype": "float32", "parameters": PARAMS, "level_set_value": a.level_set_value,
           "volumes": {},
           "checker_note": "the literal NumPy lines run at the --checker-sizes only: 512^3 x 6 classes needs more than 12 GB of float64 temporaries"}
    equal = True
    checker = set() if (a.no_cpu or a.only_device) else set(a.checker_sizes)
    sizes = set(a.sizes) | checker
    for n in sorted(sizes):
        voxels = scene(n, a.classes, seed=n)
        res = {}
        got = host = cloud = None
        tv = {k: torch.from_numpy(v).to(dev) for k, v in voxels.items()}
        res["device_to_winner_ms"], got = timed_device(lambda: proc3d.select_classes(tv, **PARAMS), a.warmup, a.reps, a.device)
        need = n ** 3 * a.classes * 4  # every class value once
        res["bytes_to_read"] = need
        res["bytes_written"] = n ** 3
        res["bytes_per_s_whole_call"] = need / (res["device_to_winner_ms"] * 1e-3)
        res["share_of_achievable_hbm"] = res["bytes_per_s_whole_call"] / ACHIEVABLE_HBM
        res["voxels_per_class"] = got[2].tolist()
        if a.kernel_stats and n == a.kernel_stats_size:
            res["kernel_ms"], res["kernel_calls_traced"] = kernel_ms(a.kernel_stats)
        if not a.only_device:
            for _ in range(2):  # (c): the first call pays vol2pcd's work buffers, the second is the figure
                t0 = time.perf_counter()
                cloud, meta = task.point_cloud_run(tv, origin, vs, a.level_set_value, **PARAMS)
                res["device_to_cloud_ms"] = (time.perf_counter() - t0) * 1e3
            res["points"] = len(cloud.points)
            res["points_per_class"] = {k: meta["labels"].count(k) for k in voxels if k != "background"}
        got = (got[0].cpu().numpy(), got[1], got[2])
        del tv
        if not a.only_device:
            res["host_to_winner_ms"], host = timed_host(lambda: proc3d.select_classes(voxels, device=a.device, **PARAMS), a.host_reps)
            res["host_equals_device"] = bool(np.array_equal(host[0], got[0]) and np.array_equal(host[2], got[2]))
            equal = equal and res["host_equals_device"]
        if n in checker:
            from tests import pointcloud_oracle as oracle
            t0 = time.perf_counter()
            want = oracle.literal_winner(voxels, PARAMS["background_prior"], PARAMS["min_contrast"], PARAMS["min_score"])
            res["checker_winner_s"] = time.perf_counter() - t0
            res["winner_equal_to_checker_device"] = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]))
            res["winner_equal_to_checker_host_route"] = bool(np.array_equal(host[0], want[0]) and np.array_equal(host[2], want[2]))
            res["checker_over_device"] = res["checker_winner_s"] * 1e3 / res["device_to_winner_ms"]
            t0 = time.perf_counter()
            per_class = oracle.literal_run(voxels, origin, vs, a.level_set_value, colors=task.POINT_CLOUD_COLORS,
                                           random_color=lambda: np.zeros(3), **PARAMS)[4]
            res["checker_run_s"] = time.perf_counter() - t0
            res["points_per_class_checker"] = per_class
            res["points_equal_to_checker"] = per_class == res["points_per_class"]
            equal = equal and res["winner_equal_to_checker_device"] and res["winner_equal_to_checker_host_route"] \
                and res["points_equal_to_checker"]
        out["volumes"][f"{n}^3"] = res
        del voxels
    big = out["volumes"].get("512^3", {})
    if "bytes_per_s_whole_call" in big and os.path.exists(a.eval_json):
        with open(a.eval_json) as f:
            ev = json.loads(f.readline())
        ref = ev.get("volumes", {}).get("512^3", {}).get("bytes_per_s_whole_call")
        if ref:
            out["throughput_bar"] = {"select_bytes_per_s_whole_call": big["bytes_per_s_whole_call"], "eval_bytes_per_s_whole_call": ref,
                                     "ratio": big["bytes_per_s_whole_call"] / ref, "bar": 0.9, "met": big["bytes_per_s_whole_call"] >= 0.9 * ref,
                                     "eval_json": os.path.relpath(a.eval_json, ROOT)}
    line = json.dumps(out)
    print(line)
    if not a.only_device:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not equal:
        sys.exit("winners or point counts differ")


if __name__ == "__main__":
    main()
