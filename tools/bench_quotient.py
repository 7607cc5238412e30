#!/usr/bin/env python3
"""Timing of ``sc_graph_quotient`` on the cloud and rows of ``tools/bench_graph.py``: the ``vol2pcd`` cloud of
the carved 512^3 plant (226 689 points), the rows ``knn_points(p, p, k)`` gives at ``k`` = 8, 16, 32 and
``radius_points(p, p, 2 voxels)``, bins of ``--bin`` voxels, the root the lowest point.  Everything is device tensors to
device tensors, HIP events around the repetitions after warm-up.  Per kind of rows:
  (a) ``graph_quotient`` over the labels ``distance_to_root_clusters`` makes (components of the bins), with the points and
      the bins as key, without and with edge weights;
  (b) the same with every node in ONE label: the serial worst case of the centres' walk (one lane per axis over all the
      nodes);
  (c) the whole ``distance_to_root_clusters`` against the route before ``sc_graph_quotient`` in the same process:
      ``graph_distances``, the bins, ``graph_components`` and the host tail of that time, kept verbatim below
      (``host_tail``; it is handed the host points ready, so the download of device points that route made is not
      charged to it); their outputs are asserted equal, bit for bit;
  (d) at ``k`` = 8 the edge set of ``nx.minimum_spanning_tree`` over our weighted cluster edges against that of
      ``nx.minimum_spanning_tree(nx.quotient_graph(g, clusters))`` over the ``networkx.Graph`` of the same rows.
      ``quotient_graph``'s default edge relation tries every pair of nodes of every pair of clusters; it is given the
      equivalent relation "some edge of g joins the two blocks" from one pass over ``g.edges`` instead; the edge data
      (the summed ``weight``) is networkx's own default.
The bar: at ``k`` = 16 the new ``distance_to_root_clusters`` is below the old route by more than 5 %.  One JSON line, also
written to ``--out``.  No GPU, no figures: there is no fallback."""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_nearest import cloud, device_ms  # noqa: E402


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def bins_of(d, bin_size, n):
    import torch
    finite = torch.isfinite(d)
    n_bins = max(1, int(torch.ceil(d[finite].max() / bin_size).item())) if n else 1
    bins = torch.clamp(torch.floor(torch.where(finite, d, torch.zeros_like(d)) / bin_size), max=n_bins - 1).to(torch.int32)
    return torch.where(finite, bins, torch.full_like(bins, -1)).contiguous()


def host_tail(xyz, rows, labels, count, bins, tdevice):
    """What ``distance_to_root_clusters`` did behind ``graph_components`` before ``sc_graph_quotient``: the rows leave the
    device, NumPy renumbers, ``np.bincount`` makes the centres, ``np.unique`` over all arcs the cluster edges."""
    import torch
    lab, hbins = _host(labels).astype(np.int64), _host(bins)
    used = lab >= 0
    _, first = np.unique(lab[used], return_index=True)
    smallest = np.flatnonzero(used)[first]
    order = np.lexsort((smallest, hbins[smallest]))
    renumber = np.empty(count, dtype=np.int64)
    renumber[order] = np.arange(count)
    cluster = np.where(used, renumber[np.where(used, lab, 0)] if count else -1, -1).astype(np.int32)
    counts = np.bincount(cluster[used], minlength=count).astype(np.float64)
    centers = np.stack([np.bincount(cluster[used], weights=xyz[used, c], minlength=count) / counts for c in range(3)], axis=1).reshape(-1, 3)
    n = len(lab)
    if len(rows) == 2:
        index = _host(rows[0])
        src = np.repeat(np.arange(n, dtype=np.int64), index.shape[1])
    else:
        index = _host(rows[1])
        src = np.repeat(np.arange(n, dtype=np.int64), np.diff(_host(rows[0])))
    index = index.reshape(-1).astype(np.int64)
    keep = index >= 0
    src, dst = src[keep], index[keep]
    ca, cb = cluster[src].astype(np.int64), cluster[dst].astype(np.int64)
    cross = (ca >= 0) & (cb >= 0) & (ca != cb)
    lo, hi = np.minimum(ca[cross], cb[cross]), np.maximum(ca[cross], cb[cross])
    pairs = np.unique(lo * max(count, 1) + hi)
    cluster_edges = np.stack([pairs // max(count, 1), pairs % max(count, 1)], axis=1).astype(np.int32).reshape(-1, 2)
    return torch.from_numpy(cluster).to(tdevice), centers, cluster_edges


def networkx_tree(hrows, cluster, n_clusters):
    """Sorted edges of ``nx.minimum_spanning_tree(nx.quotient_graph(g, clusters))`` over the graph of the rows."""
    import networkx as nx
    index, d2 = hrows
    n = len(index)
    src = np.repeat(np.arange(n, dtype=np.int64), index.shape[1])
    flat, w = index.reshape(-1).astype(np.int64), np.sqrt(d2.reshape(-1))
    keep = (flat >= 0) & (flat != src)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_weighted_edges_from(zip(src[keep].tolist(), flat[keep].tolist(), w[keep].tolist()))
    order = np.argsort(cluster, kind="stable")
    cuts = np.searchsorted(cluster[order], np.arange(n_clusters + 1))
    blocks = [frozenset(order[cuts[c]:cuts[c + 1]].tolist()) for c in range(n_clusters)]
    block_of = {b: c for c, b in enumerate(blocks)}
    joined = set()
    for u, v in g.edges():
        a, b = int(cluster[u]), int(cluster[v])
        if a >= 0 and b >= 0 and a != b:
            joined.add((min(a, b), max(a, b)))
    inside = g.subgraph(np.flatnonzero(cluster >= 0).tolist())
    q = nx.quotient_graph(inside, blocks, relabel=True,
                          edge_relation=lambda b, c: (min(block_of[b], block_of[c]), max(block_of[b], block_of[c])) in joined)
    return sorted((min(a, b), max(a, b)) for a, b in nx.minimum_spanning_tree(q).edges()), q.number_of_edges()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=72)
    ap.add_argument("--ks", type=int, nargs="*", default=[8, 16, 32])
    ap.add_argument("--radii", type=float, nargs="*", default=[2], help="in voxel sizes")
    ap.add_argument("--bin", type=float, default=8.0, help="bin size, in voxel sizes")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-networkx", action="store_true", help="skip (d)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "quotient_bench.json"))
    a = ap.parse_args()
    import torch
    from plant3dvision_amd import proc3d
    pts, vs = cloud(a.size, a.views, a.device)
    n = len(pts)
    root = int(np.argmin(pts[:, 2]))
    dp = torch.from_numpy(pts).cuda(a.device)
    bin_size = a.bin * vs
    out = {"size": a.size, "views": a.views, "points": n, "voxel_size": vs, "root": root, "reps": a.reps, "bin_voxels": a.bin,
           "first_edges": proc3d.QUOTIENT_FIRST_EDGES, "rows": {}}
    equal = True
    kinds = [(f"knn k={k}", lambda k=k: proc3d.knn_points(dp, dp, k)) for k in a.ks]
    kinds += [(f"radius={m:g}", lambda m=m: proc3d.radius_points(dp, dp, float(m) * vs)) for m in a.radii]
    one = torch.zeros(n, dtype=torch.int32, device=dp.device)
    for name, make in kinds:
        drows = make()
        r = {"E": int(drows[-1].numel())}
        d = proc3d.graph_distances(drows, root)
        bins = bins_of(d, bin_size, n)
        labels, count = proc3d.graph_components(drows, key=bins)
        for w in (False, True):
            tag = "_weighted" if w else ""
            r["quotient" + tag + "_ms"], got = device_ms(lambda: proc3d.graph_quotient(drows, labels, count, points=dp, key=bins, weights=w),
                                                         a.reps, a.warmup, a.device)
            r["one_label" + tag + "_ms"], lone = device_ms(lambda: proc3d.graph_quotient(drows, one, 1, points=dp, weights=w),
                                                           a.reps, a.warmup, a.device)
            assert int(lone[1][0]) == n and len(lone[3]) == 0
        r["clusters"], r["cluster_edges"] = int(len(got[1])), int(len(got[3]))
        same = np.array_equal(_host(lone[2])[0], [np.bincount(np.zeros(n, dtype=np.int64), weights=pts[:, c])[0] / float(n) for c in range(3)])
        r["one_label_centre_equals_bincount"] = bool(same)

        def old_route():
            dd = proc3d.graph_distances(drows, root)
            bb = bins_of(dd, bin_size, n)
            ll, cc = proc3d.graph_components(drows, key=bb)
            return host_tail(pts, drows, ll, cc, bb, dp.device) + (dd,)

        r["clusters_new_ms"], new = device_ms(lambda: proc3d.distance_to_root_clusters(dp, drows, root, bin_size), a.reps, a.warmup, a.device)
        r["clusters_old_route_ms"], old = device_ms(old_route, a.reps, a.warmup, a.device)
        r["clusters_new_weighted_ms"], neww = device_ms(lambda: proc3d.distance_to_root_clusters(dp, drows, root, bin_size, weights=True),
                                                        a.reps, a.warmup, a.device)
        r["new_over_old"] = r["clusters_new_ms"] / r["clusters_old_route_ms"]
        r["new_equals_old_route"] = bool(all(np.array_equal(_host(x), _host(y)) and _host(x).dtype == _host(y).dtype for x, y in zip(new, old)))
        equal = equal and r["new_equals_old_route"] and same
        if name == "knn k=8" and not a.no_networkx:
            import networkx as nx
            cluster, edges, edge_w = _host(neww[0]), neww[2], neww[4]
            want, r["networkx_quotient_edges"] = networkx_tree(tuple(_host(x) for x in drows), cluster, r["clusters"])
            g = nx.Graph()
            g.add_nodes_from(range(r["clusters"]))
            g.add_weighted_edges_from((a_, b_, w_) for (a_, b_), w_ in zip(edges.tolist(), edge_w.tolist()))
            ours = sorted((min(x, y), max(x, y)) for x, y in nx.minimum_spanning_tree(g).edges())
            r["independent_cycles"] = int(len(edges) - r["clusters"] + nx.number_connected_components(g))
            r["weighted_tree_equals_networkx"] = bool(ours == want)
            equal = equal and r["weighted_tree_equals_networkx"]
        out["rows"][name] = r
        print(f"{name}: {json.dumps(r)}", file=sys.stderr, flush=True)
        del drows
    bar = out["rows"].get("knn k=16")
    if bar:
        out["bar_k16_new_below_old_by_5_percent"] = bool(bar["new_over_old"] < 0.95)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not equal:
        sys.exit("the new route differs from the old one, from np.bincount or from networkx's tree")
    if out.get("bar_k16_new_below_old_by_5_percent") is False:
        sys.exit("distance_to_root_clusters is not 5 % below the old route at k = 16")


if __name__ == "__main__":
    main()
