#!/usr/bin/env python3
"""Timing of the OrganSegmentation clustering: ``proc3d.cluster_dbscan`` on the ``vol2pcd`` cloud of the
carved plant -- 512^3 (the README's 226 689 points) and 256^3 (a shell about a quarter the size, to show how the cost
grows) -- with ``eps = 2 * voxel_size`` and ``min_points = 5``, the task's defaults on a 1-voxel lattice:
  (a) device points -> device labels (a CUDA tensor), HIP events around the repetitions after warm-up;
  (b) host points -> host labels (a NumPy array), host clock, staging and both copies included;
  (c) ``sklearn.cluster.DBSCAN(n_jobs=16)`` on the same box: the only CPU yardstick there is.  Its test is ``<=``, the
      lattice is full of pairs at exactly ``eps``, so its labels differ: it is timed, not compared.
The labels of (a) and (b) are compared with the vectorised order-free checker (tests/dbscan_oracle.py), which the host
tests tie to the literal loop.  One JSON line, also written to ``--out``.  No GPU, no figures: there is no fallback."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, default=72)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--min-points", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true", help="skip (c) and the comparison (profiling runs)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "dbscan_bench.json"))
    a = ap.parse_args()
    import torch
    from plant3dvision_amd import proc3d
    from tests import dbscan_oracle
    out = {"views": a.views, "reps": a.reps, "min_points": a.min_points, "clouds": {}}
    for n in a.sizes:
        pts, vs = cloud(n, a.views, a.device)
        eps = 2.0 * vs
        dev_pts = torch.from_numpy(pts).cuda(a.device)
        for _ in range(a.warmup):
            labels = proc3d.cluster_dbscan(dev_pts, eps, a.min_points)
        torch.cuda.synchronize(a.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            labels = proc3d.cluster_dbscan(dev_pts, eps, a.min_points)
        e1.record()
        e1.synchronize()
        dev_ms = e0.elapsed_time(e1) / a.reps
        host_ms = host_labels = None
        for _ in range(1 + a.host_reps):  # the first one warms up
            t0 = time.perf_counter()
            host_labels = proc3d.cluster_dbscan(pts, eps, a.min_points, device=a.device)
            dt = (time.perf_counter() - t0) * 1e3
            host_ms = dt if host_ms is None else min(host_ms, dt)
        got = labels.cpu().numpy()
        res = {"points": int(len(pts)), "eps": eps, "device_to_device_ms": dev_ms, "host_to_host_ms": host_ms,
               "clusters": int(got.max()) + 1, "noise": int((got == -1).sum())}
        if not a.no_cpu:
            t0 = time.perf_counter()
            want = dbscan_oracle.labels_order_free(pts, eps, a.min_points)
            res["checker_s"] = time.perf_counter() - t0
            res["equal_to_checker_device"] = bool(np.array_equal(got, want))
            res["equal_to_checker_host_route"] = bool(np.array_equal(host_labels, want))
            from sklearn.cluster import DBSCAN
            t0 = time.perf_counter()
            sk = DBSCAN(eps=eps, min_samples=a.min_points, n_jobs=16).fit(pts)
            res["sklearn_16_jobs_ms"] = (time.perf_counter() - t0) * 1e3
            res["sklearn_clusters"] = int(sk.labels_.max()) + 1  # its test is <=: not the same clustering at ties
            res["sklearn_over_host_route"] = res["sklearn_16_jobs_ms"] / host_ms
        out["clouds"][f"{n}^3"] = res
    keys = list(out["clouds"])
    if len(keys) >= 2:
        lo, hi = out["clouds"][keys[0]], out["clouds"][keys[-1]]
        out["scaling"] = {"points_ratio": hi["points"] / lo["points"],
                          "device_time_ratio": hi["device_to_device_ms"] / lo["device_to_device_ms"],
                          "host_route_time_ratio": hi["host_to_host_ms"] / lo["host_to_host_ms"]}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not all(c.get("equal_to_checker_device", True) and c.get("equal_to_checker_host_route", True)
               for c in out["clouds"].values()):
        sys.exit("labels differ from the checker")


if __name__ == "__main__":
    main()
