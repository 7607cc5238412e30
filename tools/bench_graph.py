#!/usr/bin/env python3
"""Timing of the graph unit: ``proc3d.graph_distances`` / ``graph_components`` / ``distance_to_root_clusters``
on the ``vol2pcd`` cloud of the carved 512^3 plant (the README's 226 689 points), over the rows ``knn_points(p, p, k)``
gives at ``k`` = 8, 16, 32 and ``radius_points(p, p, 2 voxels)``.  The root is the lowest point (the least z).
Per kind of rows:
  (a) device tensors -> device tensors, the rows already on the device, HIP events around the repetitions after warm-up:
      ``graph_distances`` (with its rounds, the directed arcs of the adjacency and the time per round),
      ``graph_components`` and the whole ``distance_to_root_clusters`` (bins of ``--bin`` voxels; its tail is host NumPy);
  (b) host arrays -> host results, host clock, staging and copies included: the same three calls;
  (c) ``scipy.sparse.csgraph.dijkstra(csr, indices=root)`` on a ready symmetric ``csr_matrix`` (building it is not
      timed), on the same box in the same run; at ``k`` = 8 also ``nx.dijkstra_predecessor_and_distance`` once, on a ready
      ``networkx.Graph``;
  (d) the distances of (a) and (b) ``array_equal`` with scipy's; a difference ends the run with a non-zero status.
At most 16 host workers are used (scipy's Dijkstra and networkx use one).
The one bar: at ``k`` = 16 the device-to-device ``graph_distances`` is below (c).  One JSON line, also written to
``--out``.  No GPU, no figures: there is no fallback."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_nearest import cloud, device_ms  # noqa: E402


def symmetric_csr(rows, n):
    """The graph of rule G1 as a scipy ``csr_matrix``: every arc in both directions, one entry per pair (a ``csr_matrix``
    would ADD repeated entries), weight ``sqrt(d2)``; explicit zeros stay edges of weight zero."""
    from scipy import sparse
    if len(rows) == 2:
        index, d2 = rows
        src = np.repeat(np.arange(n, dtype=np.int64), index.shape[1])
        index, d2 = index.reshape(-1), d2.reshape(-1)
    else:
        offsets, index, d2 = rows
        src = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    keep = (index >= 0) & (index != src)
    i, j, w = src[keep], index[keep].astype(np.int64), np.sqrt(d2[keep])
    i, j, w = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([w, w])
    _, first = np.unique(i * n + j, return_index=True)
    return sparse.csr_matrix((w[first], (i[first], j[first])), shape=(n, n)), int(len(first))


def host_ms(fn, reps):
    best = out = None
    for _ in range(1 + reps):  # the first one warms up
        t0 = time.perf_counter()
        out = fn()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=72)
    ap.add_argument("--ks", type=int, nargs="*", default=[8, 16, 32])
    ap.add_argument("--radii", type=float, nargs="*", default=[2], help="in voxel sizes")
    ap.add_argument("--bin", type=float, default=8.0, help="bin size of distance_to_root_clusters, in voxel sizes")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true", help="skip (c) and (d) (profiling runs)")
    ap.add_argument("--no-networkx", action="store_true", help="skip the networkx baseline at k = 8")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "graph_bench.json"))
    a = ap.parse_args()
    import torch
    from plant3dvision_amd import _native as nat, proc3d
    pts, vs = cloud(a.size, a.views, a.device)
    n = len(pts)
    root = int(np.argmin(pts[:, 2]))
    dp = torch.from_numpy(pts).cuda(a.device)
    out = {"size": a.size, "views": a.views, "points": n, "voxel_size": vs, "root": root, "reps": a.reps, "bin_voxels": a.bin,
           "rounds_per_wait": nat.SC_GRAPH_ROUNDS_PER_WAIT, "rows": {}}
    equal = True
    kinds = [(f"knn k={k}", lambda k=k: proc3d.knn_points(dp, dp, k)) for k in a.ks]
    kinds += [(f"radius={m:g}", lambda m=m: proc3d.radius_points(dp, dp, float(m) * vs)) for m in a.radii]
    for name, make in kinds:
        drows = make()
        hrows = tuple(x.cpu().numpy() for x in drows)
        r = {"E": int(hrows[-1].size)}
        r["distances_device_to_device_ms"], got = device_ms(lambda: proc3d.graph_distances(drows, root, return_rounds=True), a.reps, a.warmup, a.device)
        d_dev, r["rounds"] = got[0].cpu().numpy(), got[1]
        r["ms_per_round"] = r["distances_device_to_device_ms"] / max(r["rounds"], 1)
        r["reached"] = int(np.isfinite(d_dev).sum())
        r["components_device_to_device_ms"], got = device_ms(lambda: proc3d.graph_components(drows), a.reps, a.warmup, a.device)
        r["components"] = got[1]
        r["clusters_device_to_device_ms"], got = device_ms(lambda: proc3d.distance_to_root_clusters(dp, drows, root, a.bin * vs), a.reps, a.warmup, a.device)
        r["clusters"], r["cluster_edges"] = int(len(got[1])), int(len(got[2]))
        r["distances_host_to_host_ms"], d_host = host_ms(lambda: proc3d.graph_distances(hrows, root, device=a.device), a.host_reps)
        r["components_host_to_host_ms"], _ = host_ms(lambda: proc3d.graph_components(hrows, device=a.device), a.host_reps)
        r["clusters_host_to_host_ms"], _ = host_ms(lambda: proc3d.distance_to_root_clusters(pts, hrows, root, a.bin * vs, device=a.device), a.host_reps)
        r["device_and_host_routes_equal"] = bool(np.array_equal(d_dev, d_host))
        equal = equal and r["device_and_host_routes_equal"]
        if not a.no_cpu:
            from scipy.sparse import csgraph
            csr, r["directed_arcs"] = symmetric_csr(hrows, n)
            r["scipy_dijkstra_ms"], want = host_ms(lambda: csgraph.dijkstra(csr, directed=True, indices=root), 1)
            r["scipy_over_device"] = r["scipy_dijkstra_ms"] / r["distances_device_to_device_ms"]
            r["equal_to_scipy_device"] = bool(np.array_equal(d_dev, want))
            r["equal_to_scipy_host_route"] = bool(np.array_equal(d_host, want))
            equal = equal and r["equal_to_scipy_device"] and r["equal_to_scipy_host_route"]
            if name == "knn k=8" and not a.no_networkx:
                import networkx as nx
                coo = csr.tocoo()
                g = nx.Graph()
                g.add_nodes_from(range(n))
                g.add_weighted_edges_from(zip(coo.row.tolist(), coo.col.tolist(), coo.data.tolist()))
                t0 = time.perf_counter()
                _, dist = nx.dijkstra_predecessor_and_distance(g, root)
                r["networkx_dijkstra_ms"] = (time.perf_counter() - t0) * 1e3
                full = np.full(n, np.inf)
                full[np.fromiter(dist.keys(), dtype=np.int64, count=len(dist))] = np.fromiter(dist.values(), dtype=np.float64, count=len(dist))
                r["equal_to_networkx_device"] = bool(np.array_equal(d_dev, full))
                equal = equal and r["equal_to_networkx_device"]
                del g, coo
        out["rows"][name] = r
        print(f"{name}: {json.dumps(r)}", file=sys.stderr, flush=True)
        del drows, hrows
    bar = out["rows"].get("knn k=16", {})
    if "scipy_dijkstra_ms" in bar:
        out["bar_k16_device_below_scipy"] = bool(bar["distances_device_to_device_ms"] < bar["scipy_dijkstra_ms"])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not equal:
        sys.exit("the distances differ (device route, host route, scipy, networkx)")
    if out.get("bar_k16_device_below_scipy") is False:
        sys.exit("the device route is not below scipy's Dijkstra at k = 16")


if __name__ == "__main__":
    main()
