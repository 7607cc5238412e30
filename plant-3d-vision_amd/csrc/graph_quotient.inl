// graph_quotient.inl -- the quotient of a graph under a labelling, the third entry of graph.hip: clusters
// numbered by (least key, smallest member), member counts, centres, cluster edges and their summed weights.  The rules
// Q1..Q6 are the contract in include/spacecarve.h.  Included at the end of graph.hip: it uses that file's Arcs, arc_of,
// judge, Staged, the judging kernel, grid_for and the slots.
//
// Every float64 sum here is a serial walk by ONE lane over a segment that an earlier launch laid out in the rule's
// order (stable radix sorts and scans; nothing is appended by atomics), so each sum has exactly one order.  No
// floating-point atomic.  The only data blocks share inside a launch are the label statistics (integer fetch-min and
// fetch-add, relaxed, agent scope) and the judge's flag; everything else is written in one launch and read in a later
// one.  Every loop is bounded by a count fixed before it starts.

namespace {

constexpr int kWalkAhead = 8;                   // loads a centre's walker keeps in flight
constexpr unsigned long long kNoLabel = ~0ull;  // the sort key of a label without members: behind every real key

struct QHeader {
    int C;  // clusters
    int X;  // arcs whose ends lie in different clusters
    int K;  // cluster edges
};

// f(storage, bytes) is one hipcub call: asked for its size with the call's own count, held against what was reserved,
// then run
template <class F>
hipError_t cub_run(void *storage, size_t reserved, F f) {
    size_t need = 0;
    const hipError_t e = f(nullptr, need);
    if (e != hipSuccess) return e;
    return need > reserved ? hipErrorOutOfMemory : f(storage, need);
}

int bits_of(unsigned long long x) {  // radix bits that hold 0 .. x
    int b = 1;
    while (x >>= 1) ++b;
    return b;
}

__global__ __launch_bounds__(kB) void quotient_clear_kernel(int L, int *__restrict__ kmin, int *__restrict__ smallest, int *__restrict__ cnt) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t l = (int64_t)blockIdx.x * kB + threadIdx.x; l < L; l += stride) {
        kmin[l] = 0x7FFFFFFF;
        smallest[l] = 0x7FFFFFFF;
        cnt[l] = 0;
    }
}

// Blocks on different XCDs meet in the three arrays: relaxed agent-scope integer atomics only; read after the launch.
__global__ __launch_bounds__(kB) void quotient_stats_kernel(int N, const int32_t *__restrict__ labels, const int32_t *__restrict__ key, int *kmin,
                                                            int *smallest, int *cnt) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t v = (int64_t)blockIdx.x * kB + threadIdx.x; v < N; v += stride) {
        const int l = labels[v];
        if (l < 0) continue;
        if (key) (void)__hip_atomic_fetch_min(&kmin[l], key[v], DB_RLX);
        (void)__hip_atomic_fetch_min(&smallest[l], (int)v, DB_RLX);
        (void)__hip_atomic_fetch_add(&cnt[l], 1, DB_RLX);
    }
}

// (kmin, smallest) as one unsigned key: the signed kmin with its sign bit turned, so that the order is the signed one
__global__ __launch_bounds__(kB) void quotient_keys_kernel(int L, int has_key, const int *__restrict__ kmin, const int *__restrict__ smallest,
                                                           const int *__restrict__ cnt, unsigned long long *__restrict__ lkey, int *__restrict__ lid) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t l = (int64_t)blockIdx.x * kB + threadIdx.x; l < L; l += stride) {
        const unsigned int hi = has_key ? (unsigned int)kmin[l] ^ 0x80000000u : 0u;
        lkey[l] = cnt[l] ? ((unsigned long long)hi << 32) | (unsigned int)smallest[l] : kNoLabel;
        lid[l] = (int)l;
    }
}

// Place r of the sorted labels is cluster r while the label has members (those come first).  members[] gets L + 1
// entries (0 past the clusters) for the scan that makes the segments; counts_out only its first C.
__global__ __launch_bounds__(kB) void quotient_rank_kernel(int L, const unsigned long long *__restrict__ lkey, const int *__restrict__ lid,
                                                           const int *__restrict__ cnt, int *__restrict__ renumber, int *__restrict__ members,
                                                           int32_t *__restrict__ counts_out, QHeader *__restrict__ h) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t r = (int64_t)blockIdx.x * kB + threadIdx.x; r < L; r += stride) {
        const int l = lid[r];
        const bool used = lkey[r] != kNoLabel;
        renumber[l] = used ? (int)r : -1;
        members[r] = used ? cnt[l] : 0;
        if (used) {
            counts_out[r] = cnt[l];
            if (r == L - 1 || lkey[r + 1] == kNoLabel) h->C = (int)r + 1;
        }
        if (r == 0) members[L] = 0;
    }
}

__global__ __launch_bounds__(kB) void quotient_cluster_kernel(int N, int L, const int32_t *__restrict__ labels, const int *__restrict__ renumber,
                                                              int32_t *__restrict__ cluster, unsigned int *__restrict__ skey, int *__restrict__ sval) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t v = (int64_t)blockIdx.x * kB + threadIdx.x; v < N; v += stride) {
        const int l = labels[v];
        const int c = l < 0 ? -1 : renumber[l];
        cluster[v] = c;
        if (skey) {
            skey[v] = c < 0 ? (unsigned int)L : (unsigned int)c;  // outside nodes behind every cluster
            sval[v] = (int)v;
        }
    }
}

// The coordinates in cluster order, one axis after the other: a walker reads contiguous memory.
__global__ __launch_bounds__(kB) void quotient_gather_kernel(int N, const int *__restrict__ node, const double *__restrict__ points,
                                                             double *__restrict__ xs) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t p = (int64_t)blockIdx.x * kB + threadIdx.x; p < N; p += stride) {
        const int64_t v = node[p];
        xs[p] = points[3 * v];
        xs[(int64_t)N + p] = points[3 * v + 1];
        xs[2 * (int64_t)N + p] = points[3 * v + 2];
    }
}

// One lane per (cluster, axis): s = +0.0, then the members' coordinates in rising node index, left to right -- the
// order of np.bincount(cluster, weights).  kWalkAhead loads are in flight at a time (the walk is bound by their latency);
// the adds stay in order (the unit is built with -ffp-contract=off and without fast-math: the compiler may not
// reassociate them).
__global__ __launch_bounds__(kB) void quotient_centres_kernel(int L, int N, const int *__restrict__ members, const int *__restrict__ start,
                                                              const double *__restrict__ xs, double *__restrict__ centers) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x; t < 3 * (int64_t)L; t += stride) {
        const int c = (int)(t / 3), a = (int)(t % 3);
        const int n = members[c];
        if (n == 0) continue;  // past the clusters: the row stays untouched
        const double *x = xs + (int64_t)a * N + start[c];
        double s = 0.0;
        int q = 0;
        for (; q + kWalkAhead <= n; q += kWalkAhead) {
            double v[kWalkAhead];
#pragma unroll
            for (int u = 0; u < kWalkAhead; ++u) v[u] = x[q + u];
#pragma unroll
            for (int u = 0; u < kWalkAhead; ++u) s += v[u];
        }
        for (; q < n; ++q) s += x[q];
        centers[3 * (int64_t)c + a] = s / (double)n;
    }
}

__device__ __forceinline__ bool cross_arc(const Arcs &g, const int32_t *__restrict__ cluster, int64_t t, int &i, int &j, double &w, int &ci,
                                          int &cj) {
    if (!arc_of(g, t, i, j, w)) return false;
    ci = cluster[i];
    cj = cluster[j];
    return ci >= 0 && cj >= 0 && ci != cj;
}

// g.w is NULL here: no square root is taken for a flag
__global__ __launch_bounds__(kB) void quotient_cross_kernel(Arcs g, const int32_t *__restrict__ cluster, int *__restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x; t < g.E + g.M; t += stride) {
        int i, j, ci, cj;
        double w;
        flag[t] = cross_arc(g, cluster, t, i, j, w, ci, cj) ? 1 : 0;
    }
}

// The crossing arcs in the order given (pos = exclusive sum of flag).  With weights: key = the node pair lo * N + hi,
// value = the arc's weight; without: key = the cluster pair a * C + b at once.
__global__ __launch_bounds__(kB) void quotient_compact_kernel(Arcs g, const int32_t *__restrict__ cluster, const int *__restrict__ flag,
                                                              const int *__restrict__ pos, int weighted, unsigned long long *__restrict__ okey,
                                                              double *__restrict__ oval, QHeader *__restrict__ h) {
    const int64_t stride = (int64_t)gridDim.x * kB, A = g.E + g.M;
    const unsigned long long C = (unsigned long long)h->C;  // written by an earlier launch
    for (int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x; t < A; t += stride) {
        if (t == A - 1) h->X = pos[t] + flag[t];
        if (!flag[t]) continue;
        int i, j, ci, cj;
        double w = 0.0;
        (void)cross_arc(g, cluster, t, i, j, w, ci, cj);
        const int p = pos[t];
        if (weighted) {
            okey[p] = (unsigned long long)(i < j ? i : j) * (unsigned long long)g.N + (unsigned long long)(i < j ? j : i);
            oval[p] = w;
        } else {
            okey[p] = (unsigned long long)(ci < cj ? ci : cj) * C + (unsigned long long)(ci < cj ? cj : ci);
        }
    }
}

// Behind the sort by node pair: the first entry of every pair takes the least weight of the pair's arcs and the key of
// its cluster pair; the others take the key C * C, which sorts behind every cluster pair.
__global__ __launch_bounds__(kB) void quotient_pairs_kernel(int X, int N, int C, const unsigned long long *__restrict__ ikey,
                                                            const double *__restrict__ ival, const int32_t *__restrict__ cluster,
                                                            unsigned long long *__restrict__ okey, double *__restrict__ oval) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t p = (int64_t)blockIdx.x * kB + threadIdx.x; p < X; p += stride) {
        const unsigned long long k = ikey[p];
        if (p > 0 && ikey[p - 1] == k) {
            okey[p] = (unsigned long long)C * (unsigned long long)C;
            oval[p] = 0.0;
            continue;
        }
        double m = ival[p];
        for (int64_t q = p + 1; q < X && ikey[q] == k; ++q) m = ival[q] < m ? ival[q] : m;
        const int ci = cluster[k / (unsigned long long)N], cj = cluster[k % (unsigned long long)N];
        okey[p] = (unsigned long long)(ci < cj ? ci : cj) * (unsigned long long)C + (unsigned long long)(ci < cj ? cj : ci);
        oval[p] = m;
    }
}

__global__ __launch_bounds__(kB) void quotient_heads_kernel(int X, unsigned long long none, const unsigned long long *__restrict__ key,
                                                            int *__restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t p = (int64_t)blockIdx.x * kB + threadIdx.x; p < X; p += stride) {
        const unsigned long long k = key[p];
        flag[p] = k != none && (p == 0 || key[p - 1] != k) ? 1 : 0;
    }
}

// One lane per cluster edge (the head of its segment; pos = exclusive sum of the head flags).  K is the same for every
// lane: flag and pos are complete.  The rows are written iff they all fit (rule Q5).  The sum: +0.0, then the node
// pairs' weights in rising (i, j), which is the order the two stable sorts left them in.
__global__ __launch_bounds__(kB) void quotient_emit_kernel(int X, int C, int64_t capacity, const unsigned long long *__restrict__ key,
                                                           const double *__restrict__ val, const int *__restrict__ flag, const int *__restrict__ pos,
                                                           int32_t *__restrict__ edges, double *__restrict__ edge_w, QHeader *__restrict__ h) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    const int K = pos[X - 1] + flag[X - 1];
    if (blockIdx.x == 0 && threadIdx.x == 0) h->K = K;
    if (K > capacity) return;
    for (int64_t p = (int64_t)blockIdx.x * kB + threadIdx.x; p < X; p += stride) {
        if (!flag[p]) continue;
        const int64_t e = pos[p];
        const unsigned long long k = key[p];
        edges[2 * e] = (int32_t)(k / (unsigned long long)C);
        edges[2 * e + 1] = (int32_t)(k % (unsigned long long)C);
        if (!edge_w) continue;
        double s = 0.0;
        for (int64_t q = p; q < X && key[q] == k; ++q) s += val[q];
        edge_w[e] = s;
    }
}

}  // namespace

extern "C" int sc_graph_quotient(int64_t N, const int64_t *offsets, int row_len, const int32_t *index, const double *weights, int64_t E,
                                 int weights_squared, const int32_t *extra, const double *extra_w, int64_t M, const int32_t *labels, int64_t L,
                                 const int32_t *key, const double *points, int on_device, int device, int32_t *cluster_out, int32_t *counts_out,
                                 double *centers_out, int32_t *edges_out, double *edge_w_out, int64_t capacity, int32_t *nclusters_out,
                                 int64_t *nedges_out, void *hip_stream) {
    if (!nclusters_out || !nedges_out) return g_err.fail(SC_ERR_INVALID, "null argument (nclusters_out, nedges_out)");
    const bool weighted = edge_w_out != nullptr;
    if (judge(N, offsets, row_len, index, weights, weighted, E, extra, extra_w, M, on_device, device) != SC_OK) return SC_ERR_INVALID;
    if (L < 0 || L > N) return g_err.fail(SC_ERR_INVALID, "L must be 0 .. N");
    if (capacity < 0 || (capacity > 0 && !edges_out)) return g_err.fail(SC_ERR_INVALID, "capacity must not be negative, nor positive without edges_out");
    if (weighted && !edges_out) return g_err.fail(SC_ERR_INVALID, "edge_w_out without edges_out");
    if (N == 0) {
        *nclusters_out = 0;
        *nedges_out = 0;
        return SC_OK;
    }
    if (!labels || !cluster_out || (L > 0 && !counts_out)) return g_err.fail(SC_ERR_INVALID, "null argument (labels, cluster_out, counts_out)");
    if (points && L > 0 && !centers_out) return g_err.fail(SC_ERR_INVALID, "null argument (centers_out with points)");
    if (!on_device)
        for (int64_t v = 0; v < N; ++v)
            if (labels[v] >= L) return g_err.fail(SC_ERR_INVALID, kBadLabelText);

    const int n = (int)N, nl = (int)L;
    const int64_t A = E + M;
    const int64_t cap_here = std::min(capacity, A);  // K <= A: the places of host rows the device may fill
    const bool centres = points != nullptr && L > 0;
    int rc = SC_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    UnitCall call(g_err, g_slots, device, stream, rc);
    size_t tmp_cap = 0;
    unsigned int bad = 0;
    QHeader head = {0, 0, 0};

    Layout lay;
    const size_t o_hdr = lay.take(256);  // the flag, the QHeader at +64
    const size_t o_kmin = lay.take((size_t)L * 4), o_small = lay.take((size_t)L * 4), o_cnt = lay.take((size_t)L * 4);
    const size_t o_lkey0 = lay.take((size_t)L * 8), o_lkey1 = lay.take((size_t)L * 8), o_lid0 = lay.take((size_t)L * 4),
                 o_lid1 = lay.take((size_t)L * 4);
    const size_t o_renum = lay.take((size_t)L * 4), o_members = lay.take((size_t)(L + 1) * 4), o_start = lay.take((size_t)(L + 1) * 4);
    const size_t o_skey0 = lay.take(centres ? (size_t)N * 4 : 0), o_skey1 = lay.take(centres ? (size_t)N * 4 : 0),
                 o_sval0 = lay.take(centres ? (size_t)N * 4 : 0), o_sval1 = lay.take(centres ? (size_t)N * 4 : 0),
                 o_xs = lay.take(centres ? (size_t)N * 24 : 0);
    const size_t o_flag = lay.take((size_t)A * 4), o_pos = lay.take((size_t)A * 4);
    const size_t o_key0 = lay.take((size_t)A * 8), o_key1 = lay.take((size_t)A * 8);
    const size_t o_val0 = lay.take(weighted ? (size_t)A * 8 : 0), o_val1 = lay.take(weighted ? (size_t)A * 8 : 0);
    // copies of host arrays, and the outputs before they go home
    const size_t o_lab = lay.take(on_device ? 0 : (size_t)N * 4), o_nkey = lay.take(on_device || !key ? 0 : (size_t)N * 4),
                 o_pts = lay.take(on_device || !centres ? 0 : (size_t)N * 24), o_clu = lay.take(on_device ? 0 : (size_t)N * 4),
                 o_cnto = lay.take(on_device ? 0 : (size_t)L * 4), o_ctr = lay.take(on_device || !centres ? 0 : (size_t)L * 24),
                 o_edges = lay.take(on_device ? 0 : (size_t)cap_here * 8), o_edgew = lay.take(on_device || !weighted ? 0 : (size_t)cap_here * 8);
    Staged at;
    at.plan(lay, on_device, N, offsets != nullptr, E, weighted, M);
    size_t o_tmp = 0;

    typedef unsigned long long u64;
    if ((rc = call.enter()) != SC_OK) goto done;
    {  // scan and sort storage: the largest any of the calls below can ask for
        size_t t = 0;
        const int scan_n = (int)std::max<int64_t>(A, L + 1);
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t, (const int *)nullptr, (int *)nullptr, scan_n, stream));
        tmp_cap = std::max(tmp_cap, t);
        if (L) UNIT_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, t, (const u64 *)nullptr, (u64 *)nullptr, (const int *)nullptr, (int *)nullptr, nl, 0, 64, stream));
        tmp_cap = std::max(tmp_cap, t);
        if (centres) UNIT_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, t, (const unsigned int *)nullptr, (unsigned int *)nullptr, (const int *)nullptr, (int *)nullptr, n, 0, 32, stream));
        tmp_cap = std::max(tmp_cap, t);
        if (A && weighted) UNIT_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, t, (const u64 *)nullptr, (u64 *)nullptr, (const double *)nullptr, (double *)nullptr, (int)A, 0, 64, stream));
        tmp_cap = std::max(tmp_cap, t);
        if (A && !weighted) UNIT_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, t, (const u64 *)nullptr, (u64 *)nullptr, (int)A, 0, 64, stream));
        tmp_cap = std::max(tmp_cap, t);
    }
    o_tmp = lay.take(tmp_cap);
    if ((rc = call.grow(lay.total)) != SC_OK) goto done;
    {
        char *const w = call.sl.base;
        unsigned int *flagword = reinterpret_cast<unsigned int *>(w + o_hdr);
        QHeader *h = reinterpret_cast<QHeader *>(w + o_hdr + 64);
        int *kmin = reinterpret_cast<int *>(w + o_kmin), *smallest = reinterpret_cast<int *>(w + o_small), *cnt = reinterpret_cast<int *>(w + o_cnt);
        u64 *lkey[2] = {reinterpret_cast<u64 *>(w + o_lkey0), reinterpret_cast<u64 *>(w + o_lkey1)};
        int *lid[2] = {reinterpret_cast<int *>(w + o_lid0), reinterpret_cast<int *>(w + o_lid1)};
        int *renumber = reinterpret_cast<int *>(w + o_renum), *members = reinterpret_cast<int *>(w + o_members),
            *start = reinterpret_cast<int *>(w + o_start);
        unsigned int *skey[2] = {reinterpret_cast<unsigned int *>(w + o_skey0), reinterpret_cast<unsigned int *>(w + o_skey1)};
        int *sval[2] = {reinterpret_cast<int *>(w + o_sval0), reinterpret_cast<int *>(w + o_sval1)};
        double *xs = reinterpret_cast<double *>(w + o_xs);
        int *flag = reinterpret_cast<int *>(w + o_flag), *pos = reinterpret_cast<int *>(w + o_pos);
        u64 *ekey[2] = {reinterpret_cast<u64 *>(w + o_key0), reinterpret_cast<u64 *>(w + o_key1)};
        double *eval[2] = {reinterpret_cast<double *>(w + o_val0), reinterpret_cast<double *>(w + o_val1)};
        const int32_t *lab_d = on_device ? labels : reinterpret_cast<const int32_t *>(w + o_lab);
        const int32_t *key_d = !key ? nullptr : on_device ? key : reinterpret_cast<const int32_t *>(w + o_nkey);
        const double *pts_d = !centres ? nullptr : on_device ? points : reinterpret_cast<const double *>(w + o_pts);
        int32_t *clu_d = on_device ? cluster_out : reinterpret_cast<int32_t *>(w + o_clu);
        int32_t *cnto_d = on_device ? counts_out : reinterpret_cast<int32_t *>(w + o_cnto);
        double *ctr_d = on_device ? centers_out : reinterpret_cast<double *>(w + o_ctr);
        int32_t *edges_d = on_device ? edges_out : reinterpret_cast<int32_t *>(w + o_edges);
        double *edgew_d = !weighted ? nullptr : on_device ? edge_w_out : reinterpret_cast<double *>(w + o_edgew);
        void *const tmp_d = w + o_tmp;
        Arcs g;
        g.offsets = offsets ? (on_device ? offsets : reinterpret_cast<const int64_t *>(w + at.offsets)) : nullptr;
        g.index = on_device ? index : reinterpret_cast<const int32_t *>(w + at.index);
        g.w = !weighted ? nullptr : on_device ? weights : reinterpret_cast<const double *>(w + at.weights);
        g.extra = on_device ? extra : reinterpret_cast<const int32_t *>(w + at.extra);
        g.extra_w = !weighted ? nullptr : on_device ? extra_w : reinterpret_cast<const double *>(w + at.extra_w);
        g.E = E;
        g.M = M;
        g.N = n;
        g.row_len = offsets ? 0 : row_len;
        g.squared = weights_squared ? 1 : 0;
        Arcs bare = g;  // the arcs without their weights
        bare.w = bare.extra_w = nullptr;

        UNIT_TRY(call.sl.wait(stream));
        UNIT_TRY(hipMemsetAsync(w + o_hdr, 0, 256, stream));
        if (!on_device) {
            if (offsets) UNIT_TRY(hipMemcpyAsync(w + at.offsets, offsets, (size_t)(N + 1) * 8, hipMemcpyHostToDevice, stream));
            if (E) UNIT_TRY(hipMemcpyAsync(w + at.index, index, (size_t)E * 4, hipMemcpyHostToDevice, stream));
            if (E && weighted) UNIT_TRY(hipMemcpyAsync(w + at.weights, weights, (size_t)E * 8, hipMemcpyHostToDevice, stream));
            if (M) UNIT_TRY(hipMemcpyAsync(w + at.extra, extra, (size_t)M * 8, hipMemcpyHostToDevice, stream));
            if (M && weighted) UNIT_TRY(hipMemcpyAsync(w + at.extra_w, extra_w, (size_t)M * 8, hipMemcpyHostToDevice, stream));
            UNIT_TRY(hipMemcpyAsync(w + o_lab, labels, (size_t)N * 4, hipMemcpyHostToDevice, stream));
            if (key) UNIT_TRY(hipMemcpyAsync(w + o_nkey, key, (size_t)N * 4, hipMemcpyHostToDevice, stream));
            if (centres) UNIT_TRY(hipMemcpyAsync(w + o_pts, points, (size_t)N * 24, hipMemcpyHostToDevice, stream));
        } else {  // device arrays: the first kernel is the judge (wait 1)
            hipLaunchKernelGGL(graph_flags_kernel, dim3(grid_for(std::max(std::max(E, M), N + 1))), dim3(kB), 0, stream, g, lab_d, nl, flagword);
            UNIT_TRY(hipGetLastError());
            UNIT_TRY(hipMemcpyAsync(&bad, flagword, 4, hipMemcpyDeviceToHost, stream));
            UNIT_TRY(call.sl.record(stream));
            UNIT_TRY(hipStreamSynchronize(stream));
            if (bad != 0u) {
                rc = g_err.fail(SC_ERR_INVALID, flag_text(bad));
                goto done;
            }
        }

        // Q1: statistics of the labels, their order, the clusters
        if (L) {
            hipLaunchKernelGGL(quotient_clear_kernel, dim3(grid_for(L)), dim3(kB), 0, stream, nl, kmin, smallest, cnt);
            hipLaunchKernelGGL(quotient_stats_kernel, dim3(grid_for(N)), dim3(kB), 0, stream, n, lab_d, key_d, kmin, smallest, cnt);
            hipLaunchKernelGGL(quotient_keys_kernel, dim3(grid_for(L)), dim3(kB), 0, stream, nl, key_d ? 1 : 0, kmin, smallest, cnt, lkey[0], lid[0]);
            UNIT_TRY(cub_run(tmp_d, tmp_cap, [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, lkey[0], lkey[1], lid[0], lid[1], nl, 0, 64, stream); }));
            hipLaunchKernelGGL(quotient_rank_kernel, dim3(grid_for(L)), dim3(kB), 0, stream, nl, lkey[1], lid[1], cnt, renumber, members, cnto_d, h);
        }
        hipLaunchKernelGGL(quotient_cluster_kernel, dim3(grid_for(N)), dim3(kB), 0, stream, n, nl, lab_d, renumber, clu_d,
                           centres ? skey[0] : nullptr, sval[0]);
        UNIT_TRY(hipGetLastError());

        // Q2: nodes in cluster order (stable: rising node index inside a cluster), their coordinates, one walk per (cluster, axis)
        if (centres) {
            const int node_bits = bits_of((u64)L);
            UNIT_TRY(cub_run(tmp_d, tmp_cap, [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, skey[0], skey[1], sval[0], sval[1], n, 0, node_bits, stream); }));
            UNIT_TRY(cub_run(tmp_d, tmp_cap, [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, members, start, nl + 1, stream); }));
            hipLaunchKernelGGL(quotient_gather_kernel, dim3(grid_for(N)), dim3(kB), 0, stream, n, sval[1], pts_d, xs);
            hipLaunchKernelGGL(quotient_centres_kernel, dim3(grid_for(3 * L)), dim3(kB), 0, stream, nl, n, members, start, xs, ctr_d);
            UNIT_TRY(hipGetLastError());
        }

        // Q3: the crossing arcs, in the order given
        if (A && L) {
            hipLaunchKernelGGL(quotient_cross_kernel, dim3(grid_for(A)), dim3(kB), 0, stream, bare, clu_d, flag);
            UNIT_TRY(cub_run(tmp_d, tmp_cap, [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, flag, pos, (int)A, stream); }));
            hipLaunchKernelGGL(quotient_compact_kernel, dim3(grid_for(A)), dim3(kB), 0, stream, g, clu_d, flag, pos, weighted ? 1 : 0, ekey[0], eval[0], h);
            UNIT_TRY(hipGetLastError());
        }
        if (!on_device) UNIT_TRY(hipMemcpyAsync(cluster_out, clu_d, (size_t)N * 4, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(hipMemcpyAsync(&head, h, sizeof head, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        UNIT_TRY(hipStreamSynchronize(stream));  // wait 2: C and the number of crossing arcs size the sorts
        if (head.C < 0 || head.C > L || head.X < 0 || head.X > A) {
            rc = g_err.fail(SC_ERR_DEVICE, "cluster or arc count out of range");
            goto done;
        }

        if (head.X > 0) {
            const int X = head.X;
            const u64 none = (u64)head.C * (u64)head.C;
            const int pair_bits = bits_of((u64)N * (u64)N), edge_bits = bits_of(none);
            if (weighted) {
                UNIT_TRY(cub_run(tmp_d, tmp_cap, [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, ekey[0], ekey[1], eval[0], eval[1], X, 0, pair_bits, stream); }));
                hipLaunchKernelGGL(quotient_pairs_kernel, dim3(grid_for(X)), dim3(kB), 0, stream, X, n, head.C, ekey[1], eval[1], clu_d, ekey[0], eval[0]);
                UNIT_TRY(cub_run(tmp_d, tmp_cap, [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, ekey[0], ekey[1], eval[0], eval[1], X, 0, edge_bits, stream); }));
            } else {
                UNIT_TRY(cub_run(tmp_d, tmp_cap, [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortKeys(t, b, ekey[0], ekey[1], X, 0, edge_bits, stream); }));
            }
            hipLaunchKernelGGL(quotient_heads_kernel, dim3(grid_for(X)), dim3(kB), 0, stream, X, none, ekey[1], flag);
            UNIT_TRY(cub_run(tmp_d, tmp_cap, [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, flag, pos, X, stream); }));
            hipLaunchKernelGGL(quotient_emit_kernel, dim3(grid_for(X)), dim3(kB), 0, stream, X, head.C, capacity, ekey[1], eval[1], flag, pos, edges_d,
                               edgew_d, h);
            UNIT_TRY(hipGetLastError());
        }
        if (!on_device) {
            if (head.C) UNIT_TRY(hipMemcpyAsync(counts_out, cnto_d, (size_t)head.C * 4, hipMemcpyDeviceToHost, stream));
            if (head.C && centres) UNIT_TRY(hipMemcpyAsync(centers_out, ctr_d, (size_t)head.C * 24, hipMemcpyDeviceToHost, stream));
        }
        UNIT_TRY(hipMemcpyAsync(&head, h, sizeof head, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        UNIT_TRY(hipStreamSynchronize(stream));  // wait 3: K
        if (head.K < 0 || head.K > head.X) {
            rc = g_err.fail(SC_ERR_DEVICE, "edge count out of range");
            goto done;
        }
        if (!on_device && head.K > 0 && head.K <= capacity) {  // host rows: they go home behind a last wait
            UNIT_TRY(hipMemcpyAsync(edges_out, edges_d, (size_t)head.K * 8, hipMemcpyDeviceToHost, stream));
            if (weighted) UNIT_TRY(hipMemcpyAsync(edge_w_out, edgew_d, (size_t)head.K * 8, hipMemcpyDeviceToHost, stream));
            UNIT_TRY(call.sl.record(stream));
            UNIT_TRY(hipStreamSynchronize(stream));
        }
        *nclusters_out = head.C;
        *nedges_out = head.K;
    }

done:
    give_back_if_large(call);
    return rc;
}
