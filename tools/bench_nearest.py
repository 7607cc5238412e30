#!/usr/bin/env python3
"""Timing of the nearest-point search: ``proc3d.nearest_points`` / ``nearest_sums`` on the ``vol2pcd``
cloud of the carved plant -- 512^3 (the README's 226 689 points) and 256^3 -- searched against two targets:
  aligned    : itself displaced by (0.37, -0.21, 0.40) voxels plus seeded uniform jitter of +-0.25 voxel: two
               reconstructions of one plant;
  misaligned : itself displaced by 20 voxels: the ring search runs out and the far pass runs.
Per leg:
  (a) device tensors -> the registration sums (``nearest_sums``, max_distance 2 voxels), HIP events around the
      repetitions after warm-up;
  (b) device tensors -> ``index`` and ``d2`` on the device, the same way;
  (c) host arrays -> host results, host clock, staging and copies included;
  (d) ``scipy.spatial.cKDTree(target).query(queries, workers=16)``, build included, on the same box in the same run.
``index`` and ``d2`` of (b) and (c) are compared with the checker (tests/nearest_oracle.py), ``array_equal`` for both;
a difference ends the run with a non-zero status.  The one bar: on the aligned 512^3 leg (b) is below (d).
One JSON line, also written to ``--out``.  No GPU, no figures: there is no fallback."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def cloud(n, views, device):
    from plant3dvision_amd import proc3d, scenes
    from plant3dvision_amd.cl import Backprojection
    shape, origin, vs, scene_views = scenes.make_scene(n, views, "plant")
    bp = Backprojection(shape, origin, vs, device=device)
    for K, R, t, m in scene_views:
        bp.process_view(K, R, t, m)
    pc = proc3d.vol2pcd(bp, np.array(origin), vs, 1.0, device=device, as_open3d=False)
    bp.close()
    return np.ascontiguousarray(np.asarray(pc.points, dtype=np.float64)), float(vs)


def device_ms(fn, reps, warmup, device):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, default=72)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--far-reps", type=int, default=3, help="repetitions of the misaligned leg (its far pass is O(Q P))")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true", help="skip (d) and the comparison (profiling runs)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "nearest_bench.json"))
    a = ap.parse_args()
    import torch
    from plant3dvision_amd import proc3d
    from tests import nearest_oracle
    out = {"views": a.views, "reps": a.reps, "far_reps": a.far_reps, "clouds": {}}
    equal = True
    for n in a.sizes:
        pts, vs = cloud(n, a.views, a.device)
        rng = np.random.default_rng(n)
        targets = {"aligned": pts + vs * (np.array([0.37, -0.21, 0.40]) + rng.uniform(-0.25, 0.25, size=pts.shape)),
                   "misaligned": pts + vs * np.array([20.0, 0.0, 0.0])}
        res = {"points": int(len(pts)), "voxel_size": vs}
        dq = torch.from_numpy(pts).cuda(a.device)
        for leg, tgt in targets.items():
            tgt = np.ascontiguousarray(tgt)
            dt = torch.from_numpy(tgt).cuda(a.device)
            reps, warm = (a.reps, a.warmup) if leg == "aligned" else (a.far_reps, 1)
            sums_ms, sums = device_ms(lambda: proc3d.nearest_sums(dq, dt, 2.0 * vs), reps, warm, a.device)
            index_ms, (index, d2) = device_ms(lambda: proc3d.nearest_points(dq, dt), reps, warm, a.device)
            host_ms = host = None
            for _ in range(1 + (a.host_reps if leg == "aligned" else 1)):  # the first one warms up
                t0 = time.perf_counter()
                host = proc3d.nearest_points(pts, tgt, device=a.device)
                ms = (time.perf_counter() - t0) * 1e3
                host_ms = ms if host_ms is None else min(host_ms, ms)
            r = {"device_sums_ms": sums_ms, "device_to_device_ms": index_ms, "host_to_host_ms": host_ms,
                 "fitness_at_2_voxels": sums[0] / len(pts), "inlier_rmse_voxels": float(np.sqrt(sums[1] / sums[0])) / vs if sums[0] else 0.0}
            if not a.no_cpu:
                from scipy.spatial import cKDTree
                tree_ms = None
                for _ in range(2):
                    t0 = time.perf_counter()
                    cKDTree(tgt).query(pts, workers=16)
                    ms = (time.perf_counter() - t0) * 1e3
                    tree_ms = ms if tree_ms is None else min(tree_ms, ms)
                r["ckdtree_16_workers_ms"] = tree_ms
                r["ckdtree_over_device"] = tree_ms / index_ms
                t0 = time.perf_counter()
                want = nearest_oracle.nearest(pts, tgt)
                r["checker_s"] = time.perf_counter() - t0
                r["equal_to_checker_device"] = bool(np.array_equal(index.cpu().numpy(), want[0]) and np.array_equal(d2.cpu().numpy(), want[1]))
                r["equal_to_checker_host_route"] = bool(np.array_equal(host[0], want[0]) and np.array_equal(host[1], want[1]))
                equal = equal and r["equal_to_checker_device"] and r["equal_to_checker_host_route"]
            res[leg] = r
            print(f"{n}^3 {leg}: {json.dumps(r)}", file=sys.stderr, flush=True)
        out["clouds"][f"{n}^3"] = res
    big = out["clouds"].get("512^3", {}).get("aligned", {})
    if "ckdtree_16_workers_ms" in big:
        out["bar_aligned_512_device_below_ckdtree"] = bool(big["device_to_device_ms"] < big["ckdtree_16_workers_ms"])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not equal:
        sys.exit("index or d2 differ from the checker")
    if out.get("bar_aligned_512_device_below_ckdtree") is False:
        sys.exit("the device route is not below cKDTree on the aligned 512^3 leg")


if __name__ == "__main__":
    main()
