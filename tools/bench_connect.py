#!/usr/bin/env python3
"""Timing of ``sc_graph_connect`` on the cloud of ``tools/bench_nearest.py``: the ``vol2pcd`` cloud of the
carved 512^3 plant (226 689 points), the root the lowest point.  Cases, each with its component count recorded:
  * the components of the rows ``knn_points(p, p, k)`` gives at ``k`` = 2, 4, 8, 16;
  * the components of ``radius_points(p, p, r)`` at ``r`` = 1 and 2 voxels;
  * a synthetic fragmented one: every point of a 16 384-point subsample its own label.
Per case ``connect_edges`` is timed device to device (HIP events) and host to host, and the route before
``sc_graph_connect`` host to host: the loop over the public ``nearest_points`` kept verbatim below (``old_route``), in the
same process, old and new alternating.  Old and new outputs are asserted equal, bit for bit, wherever both ran.  The old
route makes one search per component: above ``--old-max`` components it is not run (the row says so), above
``--old-few`` it runs once.  At ``k`` = 16 the whole skeleton (``weighted=True``) with the cloud resident is timed against
the parent's host route, built here from the public array-form functions.  The spread of every figure is the range of
its repeated identical runs; a bar is met when the difference exceeds the larger spread of the two sides.  One JSON
line, also written to ``--out``.  No GPU, no figures: there is no fallback."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_nearest import cloud  # noqa: E402


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def old_route(points, labels, root, device=0):
    """``proc3d.connect_edges`` before ``sc_graph_connect``, verbatim: one ``nearest_points`` search and a host relabel per
    component."""
    from plant3dvision_amd.proc3d import nearest_points
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    edges, weights = [], []
    inside = lab == lab[root] if len(points) else np.zeros(0, dtype=bool)
    while not inside.all():
        out_ids, in_ids = np.flatnonzero(~inside), np.flatnonzero(inside)
        index, d2 = nearest_points(points[out_ids], points[in_ids], device=device)
        a = int(np.argmin(d2))  # the first least d2: the smallest i; nearest_points gave it its smallest j (rule N2)
        i, j = int(out_ids[a]), int(in_ids[index[a]])
        edges.append((i, j))
        weights.append(np.sqrt(d2[a]))
        inside |= lab == lab[i]
    return np.array(edges, dtype=np.int32).reshape(-1, 2), np.array(weights, dtype=np.float64)


def old_skeleton(pts, root, binsize, k, device=0):
    """``skeleton_from_distance_to_root_clusters(..., weighted=True)`` as the parent drove it: every step host to host."""
    import networkx as nx
    from plant3dvision_amd import proc3d
    rows = proc3d.knn_points(pts, pts, int(k), device=device)
    extra = None
    labels, count = proc3d.graph_components(rows, device=device)
    if count > 1:
        extra = old_route(pts, labels, root, device=device)
    got = proc3d.distance_to_root_clusters(pts, rows, root, binsize, extra=extra, device=device, weights=True)
    cluster, centers, cluster_edges, edge_w = got[0], got[1], got[2], got[4]
    g = nx.Graph()
    for c in range(len(centers)):
        g.add_node(c, center=centers[c])
    g.add_weighted_edges_from((int(a), int(b), float(w)) for (a, b), w in zip(cluster_edges.tolist(), edge_w.tolist()))
    return nx.minimum_spanning_tree(g), {int(v): int(c) for v, c in enumerate(cluster.tolist()) if c >= 0}


def wall_ms(fn, device):
    import torch
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(device)
    return (time.perf_counter() - t0) * 1e3, out


def event_ms(fn, device):
    import torch
    torch.cuda.synchronize(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def figures(times):
    """Median and spread (the range) of repeated identical runs."""
    t = sorted(times)
    return {"ms": t[len(t) // 2], "spread_ms": t[-1] - t[0], "runs": len(t)}


def alternate(timers, reps, warmup):
    """``timers``: name -> (clock, fn, runs or None).  One run of each in turn, ``reps`` times after ``warmup`` turns."""
    times, last = {name: [] for name in timers}, {}
    for turn in range(warmup + reps):
        for name, (clock, fn, runs) in timers.items():
            if runs is not None and runs < reps and not warmup <= turn < warmup + runs:
                continue  # (a route run fewer times has no warm-up turn of its own)
            ms, last[name] = clock(fn)
            if turn >= warmup:
                times[name].append(ms)
    return {name: figures(t) for name, t in times.items() if t}, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=72)
    ap.add_argument("--ks", type=int, nargs="*", default=[2, 4, 8, 16])
    ap.add_argument("--radii", type=float, nargs="*", default=[1, 2], help="in voxel sizes")
    ap.add_argument("--synthetic", type=int, default=16384, help="points of the subsample whose points are all singletons (0: none)")
    ap.add_argument("--bin", type=float, default=8.0, help="bin size of the skeleton, in voxel sizes")
    ap.add_argument("--skeleton-k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--old-few", type=int, default=256, help="above this many components the old route runs once")
    ap.add_argument("--old-max", type=int, default=20000, help="above this many components the old route is not run")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "connect_bench.json"))
    a = ap.parse_args()
    import torch
    from plant3dvision_amd import proc3d
    if not torch.cuda.is_available():
        sys.exit("bench_connect needs a GPU: there is no fallback")
    pts, vs = cloud(a.size, a.views, a.device)
    n = len(pts)
    root = int(np.argmin(pts[:, 2]))
    dp = torch.from_numpy(pts).cuda(a.device)
    out = {"size": a.size, "views": a.views, "points": n, "voxel_size": vs, "root": root, "reps": a.reps, "cases": {}}
    equal = True

    cases = [(f"knn k={k}", pts, dp, root, lambda k=k: proc3d.graph_components(proc3d.knn_points(dp, dp, k))) for k in a.ks]
    cases += [(f"radius={m:g}", pts, dp, root, lambda m=m: proc3d.graph_components(proc3d.radius_points(dp, dp, float(m) * vs)))
              for m in a.radii]
    if a.synthetic:
        pick = np.sort(np.random.default_rng(0).choice(n, size=min(a.synthetic, n), replace=False))
        sub = np.ascontiguousarray(pts[pick])
        dsub = torch.from_numpy(sub).cuda(a.device)
        cases.append((f"singletons {len(sub)}", sub, dsub, int(np.argmin(sub[:, 2])),
                      lambda: (torch.arange(len(sub), dtype=torch.int32, device=dsub.device), len(sub))))

    def clock_wall(fn):
        return wall_ms(fn, a.device)

    def clock_event(fn):
        return event_ms(fn, a.device)

    for name, hp, tp, rt, make in cases:
        dl, count = make()
        hl = _host(dl)
        r = {"points": len(hp), "components": int(count)}
        old_runs = 0 if count > a.old_max else 1 if count > a.old_few else a.reps
        timers = {"new_device_to_device": (clock_event, lambda: proc3d.connect_edges(tp, dl, rt, n_labels=count), None),
                  "new_host_to_host": (clock_wall, lambda: proc3d.connect_edges(hp, hl, rt, device=a.device), None)}
        if old_runs:
            timers["old_host_to_host"] = (clock_wall, lambda: old_route(hp, hl, rt, device=a.device), old_runs)
        r["figures"], last = alternate(timers, a.reps, a.warmup)
        dd, hh = last["new_device_to_device"], last["new_host_to_host"]
        r["edges"] = int(len(hh[0]))
        r["device_equals_host"] = bool(np.array_equal(_host(dd[0]), hh[0]) and np.array_equal(_host(dd[1]), hh[1]))
        equal = equal and r["device_equals_host"] and r["edges"] == count - 1
        if old_runs:
            old = last["old_host_to_host"]
            r["new_equals_old_route"] = bool(np.array_equal(old[0], hh[0]) and np.array_equal(old[1], hh[1]) and old[0].dtype == hh[0].dtype)
            equal = equal and r["new_equals_old_route"]
        else:
            r["old_host_to_host"] = f"not run: {count} components, one nearest_points search each"
        out["cases"][name] = r
        print(f"{name}: {json.dumps(r)}", file=sys.stderr, flush=True)

    def margin(r):
        f = r["figures"]
        return max(f["new_host_to_host"]["spread_ms"], f["old_host_to_host"]["spread_ms"])

    real = [(r["components"], name) for name, r in out["cases"].items() if not name.startswith("singletons") and "old_host_to_host" in r["figures"]]
    if real:
        name = max(real)[1]
        r = out["cases"][name]
        f = r["figures"]
        out["bar_most_fragmented"] = {"case": name, "met": bool(f["old_host_to_host"]["ms"] - f["new_host_to_host"]["ms"] > margin(r))}
    r = out["cases"].get("knn k=8")
    if r and "old_host_to_host" in r["figures"]:
        f = r["figures"]
        out["bar_k8_not_slower"] = {"met": bool(f["new_host_to_host"]["ms"] - f["old_host_to_host"]["ms"] <= margin(r))}

    if a.skeleton_k:
        binsize = a.bin * vs
        pcd = proc3d.PointCloud(pts, None)
        timers = {"resident": (clock_wall, lambda: proc3d.skeleton_from_distance_to_root_clusters(pcd, root, binsize, a.skeleton_k,
                                                                                                   device=a.device, weighted=True), None),
                  "parent_host_route": (clock_wall, lambda: old_skeleton(pts, root, binsize, a.skeleton_k, device=a.device), None)}
        f, last = alternate(timers, a.reps, a.warmup)
        (tree_a, values_a), (tree_b, values_b) = last["resident"], last["parent_host_route"]
        same = values_a == values_b and sorted(map(sorted, tree_a.edges)) == sorted(map(sorted, tree_b.edges)) and \
            all(tree_a.edges[e] == tree_b.edges[e] for e in tree_a.edges) and \
            all(np.array_equal(tree_a.nodes[c]["center"], tree_b.nodes[c]["center"]) for c in tree_a.nodes)
        equal = equal and same
        spread = max(f["resident"]["spread_ms"], f["parent_host_route"]["spread_ms"])
        out["skeleton"] = {"k": a.skeleton_k, "bin_voxels": a.bin, "clusters": tree_a.number_of_nodes(), "figures": f, "equal": bool(same),
                           "bar_resident_below_parent": {"met": bool(f["parent_host_route"]["ms"] - f["resident"]["ms"] > spread)}}
        print(f"skeleton: {json.dumps(out['skeleton'])}", file=sys.stderr, flush=True)

    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not equal:
        sys.exit("the new route differs from the old one, or device to device from host to host")
    missed = [k for k in ("bar_most_fragmented", "bar_k8_not_slower") if out.get(k, {}).get("met") is False]
    if out.get("skeleton", {}).get("bar_resident_below_parent", {}).get("met") is False:
        missed.append("skeleton bar_resident_below_parent")
    if missed:
        sys.exit("bars missed: " + ", ".join(missed))


if __name__ == "__main__":
    main()
