#!/usr/bin/env python3
"""Timing of the k-nearest search: ``proc3d.knn_points`` on the ``vol2pcd`` cloud of the carved 512^3 plant
(the README's 226 689 points), searched against itself (``self``: the shape of ``knn_graph``) and against DESIGN 16's
aligned copy (``aligned``: itself displaced by (0.37, -0.21, 0.40) voxels plus seeded uniform jitter of +-0.25 voxel),
for ``k`` in 1, 8, 16, 32, 300.
Per leg and ``k``:
  (a) device tensors -> ``index`` and ``d2`` on the device, HIP events around the repetitions after warm-up, for every
      ``aim`` (targets per cell the grid is planned for, ``sc_knn_set_aim``) of ``--aims`` and for the built-in one;
      ``far_out`` (queries the pass over all targets took) beside each;
  (b) host arrays -> host results, host clock, staging and copies included (built-in ``aim``);
  (c) ``scipy.spatial.cKDTree(target).query(queries, k=k, workers=16)``, build included, on the same box in the same run;
  (d) ``index`` and ``d2`` of (a) and (b) ``array_equal`` with the checker (tests/knn_oracle.py); a difference ends the
      run with a non-zero status.
The ``k = 1`` legs also time ``proc3d.nearest_points`` the same way.  The one bar: at ``k = 16``, ``self``, (a) with the
built-in ``aim`` is below (c).  One JSON line, also written to ``--out``.  No GPU, no figures: there is no fallback."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_nearest import cloud, device_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=72)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 8, 16, 32, 300])
    ap.add_argument("--aims", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32, 64],
                    help="targets per cell to try; of these a k tries those from k / 32 to max(4, 2 k), and the built-in one")
    ap.add_argument("--legs", nargs="+", default=["self", "aligned"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true", help="skip (c) and (d) (profiling runs)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "knn_bench.json"))
    a = ap.parse_args()
    import torch
    from plant3dvision_amd import _native as nat, proc3d
    from tests import knn_oracle
    b = nat.backend()
    pts, vs = cloud(a.size, a.views, a.device)
    rng = np.random.default_rng(a.size)
    targets = {"self": pts, "aligned": np.ascontiguousarray(pts + vs * (np.array([0.37, -0.21, 0.40]) + rng.uniform(-0.25, 0.25, size=pts.shape)))}
    out = {"size": a.size, "views": a.views, "points": int(len(pts)), "voxel_size": vs, "reps": a.reps, "legs": {}}
    dq = torch.from_numpy(pts).cuda(a.device)
    equal = True
    for leg in a.legs:
        tgt = targets[leg]
        dt = torch.from_numpy(tgt).cuda(a.device)
        res = {}
        for k in a.ks:
            r = {"aims": {}}
            for aim in [0] + [x for x in a.aims if k / 32 <= x <= max(4, 2 * k)]:  # 0: the built-in function of k
                b.call("sc_knn_set_aim", aim)
                ms, got = device_ms(lambda: proc3d.knn_points(dq, dt, k, return_far=True), a.reps, a.warmup, a.device)
                r["aims"]["built-in" if aim == 0 else str(aim)] = {"device_to_device_ms": ms, "far": got[2]}
                if aim == 0:
                    index, d2 = got[0].cpu().numpy(), got[1].cpu().numpy()
            b.call("sc_knn_set_aim", 0)
            r["device_to_device_ms"], r["far"] = r["aims"]["built-in"]["device_to_device_ms"], r["aims"]["built-in"]["far"]
            r["best_aim"] = min((v["device_to_device_ms"], name) for name, v in r["aims"].items() if name != "built-in")[1]
            host_ms = host = None
            for _ in range(1 + a.host_reps):  # the first one warms up
                t0 = time.perf_counter()
                host = proc3d.knn_points(pts, tgt, k, device=a.device)
                ms = (time.perf_counter() - t0) * 1e3
                host_ms = ms if host_ms is None else min(host_ms, ms)
            r["host_to_host_ms"] = host_ms
            if k == 1:
                r["nearest_points_device_to_device_ms"] = device_ms(lambda: proc3d.nearest_points(dq, dt), a.reps, a.warmup, a.device)[0]
            if not a.no_cpu:
                from scipy.spatial import cKDTree
                tree_ms = None
                for _ in range(2):
                    t0 = time.perf_counter()
                    cKDTree(tgt).query(pts, k=k, workers=16)
                    ms = (time.perf_counter() - t0) * 1e3
                    tree_ms = ms if tree_ms is None else min(tree_ms, ms)
                r["ckdtree_16_workers_ms"] = tree_ms
                r["ckdtree_over_device"] = tree_ms / r["device_to_device_ms"]
                t0 = time.perf_counter()
                want = knn_oracle.knn(pts, tgt, k)
                r["checker_s"] = time.perf_counter() - t0
                r["equal_to_checker_device"] = bool(np.array_equal(index, want[0]) and np.array_equal(d2, want[1]))
                r["equal_to_checker_host_route"] = bool(np.array_equal(host[0], want[0]) and np.array_equal(host[1], want[1]))
                equal = equal and r["equal_to_checker_device"] and r["equal_to_checker_host_route"]
            res[f"k={k}"] = r
            print(f"{leg} k={k}: {json.dumps(r)}", file=sys.stderr, flush=True)
        out["legs"][leg] = res
    bar = out["legs"].get("self", {}).get("k=16", {})
    if "ckdtree_16_workers_ms" in bar:
        out["bar_self_k16_device_below_ckdtree"] = bool(bar["device_to_device_ms"] < bar["ckdtree_16_workers_ms"])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not equal:
        sys.exit("index or d2 differ from the checker")
    if out.get("bar_self_k16_device_below_ckdtree") is False:
        sys.exit("the device route is not below cKDTree at k = 16, self-search")


if __name__ == "__main__":
    main()
