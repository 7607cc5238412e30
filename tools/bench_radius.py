#!/usr/bin/env python3
"""Timing of the radius search: ``proc3d.radius_points`` / ``radius_counts`` on the ``vol2pcd`` cloud of the
carved 512^3 plant (the README's 226 689 points), searched against itself (``self``: the shape of ``radius_graph`` and of
``OrganSegmentation``'s DBSCAN) and against DESIGN 16's aligned copy (``aligned``: itself displaced by (0.37, -0.21, 0.40)
voxels plus seeded uniform jitter of +-0.25 voxel), for ``radius`` = 1, 2, 4, 8 and 16 voxel sizes.
Per leg and radius:
  (a) device tensors -> device tensors, HIP events around the repetitions after warm-up: ``radius_counts`` alone and
      ``radius_points`` whole (both of its calls); ``E``, the mean and the longest row and ``long_out`` beside them;
  (b) host arrays -> host results, host clock, staging and copies included;
  (c) ``scipy.spatial.cKDTree(targets).query_ball_point(queries, r, workers=16)``, build included, on the same box in the
      same run;
  (d) ``offsets``, ``index`` and ``d2`` of (a) and (b) ``array_equal`` with the checker (tests/radius_oracle.py); a
      difference ends the run with a non-zero status;
  (e) reported, not barred: the share of ``radius_points`` the count-only call accounts for (the second call plans the
      grid and counts again), pairs per second, ``12 E`` bytes over the fill's time (``radius_points`` less two count-only
      calls) against 8 TB/s, and ``knn_points`` at the ``k`` nearest to the mean row length.
The one bar: at ``radius`` = 2 voxel sizes, ``self``, the whole device-to-device ``radius_points`` is below (c).  One JSON
line, also written to ``--out``.  No GPU, no figures: there is no fallback."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_nearest import cloud, device_ms  # noqa: E402

HBM_BYTES_PER_S = 8e12  # the README's figure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=72)
    ap.add_argument("--radii", type=float, nargs="+", default=[1, 2, 4, 8, 16], help="in voxel sizes")
    ap.add_argument("--legs", nargs="+", default=["self", "aligned"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true", help="skip (c) and (d) (profiling runs)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "radius_bench.json"))
    a = ap.parse_args()
    import torch
    from plant3dvision_amd import _native as nat, proc3d
    from tests import radius_oracle
    pts, vs = cloud(a.size, a.views, a.device)
    rng = np.random.default_rng(a.size)
    targets = {"self": pts, "aligned": np.ascontiguousarray(pts + vs * (np.array([0.37, -0.21, 0.40]) + rng.uniform(-0.25, 0.25, size=pts.shape)))}
    out = {"size": a.size, "views": a.views, "points": int(len(pts)), "voxel_size": vs, "reps": a.reps, "lds_row": nat.SC_RADIUS_LDS_ROW, "legs": {}}
    dq = torch.from_numpy(pts).cuda(a.device)
    equal = True
    for leg in a.legs:
        tgt = targets[leg]
        dt = torch.from_numpy(tgt).cuda(a.device)
        res = {}
        for mult in a.radii:
            radius = float(mult) * vs
            r = {"radius": radius}
            r["counts_device_to_device_ms"], _ = device_ms(lambda: proc3d.radius_counts(dq, dt, radius), a.reps, a.warmup, a.device)
            r["device_to_device_ms"], got = device_ms(lambda: proc3d.radius_points(dq, dt, radius, return_long=True), a.reps, a.warmup, a.device)
            offsets, index, d2 = (x.cpu().numpy() for x in got[:3])
            lengths = np.diff(offsets)
            E = int(offsets[-1])
            r.update(E=E, mean_row=float(lengths.mean()), longest_row=int(lengths.max()), long=int(got[3]))
            r["count_share"] = r["counts_device_to_device_ms"] / r["device_to_device_ms"]
            r["pairs_per_s"] = E / (r["device_to_device_ms"] * 1e-3)
            fill_ms = r["device_to_device_ms"] - 2.0 * r["counts_device_to_device_ms"]
            r["fill_ms_derived"] = fill_ms
            r["fill_share_of_hbm"] = 12.0 * E / (fill_ms * 1e-3) / HBM_BYTES_PER_S if fill_ms > 0 else None
            k = int(min(max(round(r["mean_row"]), 1), nat.SC_KNN_MAX))
            r["knn_k"], r["knn_device_to_device_ms"] = k, device_ms(lambda: proc3d.knn_points(dq, dt, k), a.reps, a.warmup, a.device)[0]
            del got
            host_ms = host = None
            for _ in range(1 + a.host_reps):  # the first one warms up
                t0 = time.perf_counter()
                host = proc3d.radius_points(pts, tgt, radius, device=a.device)
                ms = (time.perf_counter() - t0) * 1e3
                host_ms = ms if host_ms is None else min(host_ms, ms)
            r["host_to_host_ms"] = host_ms
            if not a.no_cpu:
                from scipy.spatial import cKDTree
                tree_ms = None
                for _ in range(2):
                    t0 = time.perf_counter()
                    cKDTree(tgt).query_ball_point(pts, radius, workers=16)
                    ms = (time.perf_counter() - t0) * 1e3
                    tree_ms = ms if tree_ms is None else min(tree_ms, ms)
                r["ckdtree_16_workers_ms"] = tree_ms
                r["ckdtree_over_device"] = tree_ms / r["device_to_device_ms"]
                t0 = time.perf_counter()
                want = radius_oracle.radius(pts, tgt, radius, workers=16)
                r["checker_s"] = time.perf_counter() - t0
                r["equal_to_checker_device"] = bool(all(np.array_equal(g, w) for g, w in zip((offsets, index, d2), want)))
                r["equal_to_checker_host_route"] = bool(all(np.array_equal(g, w) for g, w in zip(host, want)))
                equal = equal and r["equal_to_checker_device"] and r["equal_to_checker_host_route"]
                del want
            del host, offsets, index, d2
            res[f"radius={mult:g}"] = r
            print(f"{leg} radius={mult:g}: {json.dumps(r)}", file=sys.stderr, flush=True)
        out["legs"][leg] = res
    bar = out["legs"].get("self", {}).get("radius=2", {})
    if "ckdtree_16_workers_ms" in bar:
        out["bar_self_radius2_device_below_ckdtree"] = bool(bar["device_to_device_ms"] < bar["ckdtree_16_workers_ms"])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not equal:
        sys.exit("offsets, index or d2 differ from the checker")
    if out.get("bar_self_radius2_device_below_ckdtree") is False:
        sys.exit("the device route is not below cKDTree at radius = 2 voxel sizes, self-search")


if __name__ == "__main__":
    main()
