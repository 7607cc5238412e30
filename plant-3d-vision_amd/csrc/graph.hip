// graph.hip -- distances to a root, connected components and the quotient under a labelling (DESIGN.md 21,
// graph_quotient.inl) over the rows of sc_knn / sc_radius; the edges that connect the components (DESIGN.md 22,
// graph_connect.inl).
//
// The two graph steps of the reference's XU skeleton (plant3dvision/proc3d.py:212-426): what
// nx.dijkstra_predecessor_and_distance(g, root) returns as distances, and nx.connected_components, of whole graphs or
// of the nodes of one key (the bins of distance_to_root_clusters).  The rules G1..G4 are the contract in
// include/spacecarve.h.  The distances are PINNED: a label-correcting fixpoint in float64 gives Dijkstra's numbers bit
// for bit (float64 addition of non-negative numbers is monotone and never decreases), which tests/test_graph_host.py
// shows against networkx and scipy.
//
// Distances: degree (integer atomics on both ends of every arc), scan, scatter -> the symmetric adjacency; then one
// launch per round of a frontier label-correcting loop.  d[] holds the bit patterns of non-negative doubles, whose
// order as uint64 is the order of the numbers; lowering is an integer fetch-min.  Inside a round blocks on different
// XCDs share d[], stamp[] and the next frontier's length: every access to them is a relaxed agent-scope atomic, none
// a plain load (sc_unionfind.h has the same rule for parent[]).  The frontiers themselves are written in one launch
// and read in the next.  No floating-point atomic, no wavefront waits on another, no kernel spins; every loop of
// these launches is bounded by a count fixed before it starts.
// Components: sc_unionfind.h over the arcs as given (no adjacency is built), flatten, mark roots, scan, number.  The
// union-find's loops end as they do in dbscan.hip: a parent only ever falls, and a failed swap means another lane's
// succeeded.
// Stand-alone unit on the scaffold of sc_unit.h.

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>

#include "sc_points.h"
#include "sc_unionfind.h"
#include "sc_unit.h"

namespace {

constexpr int kB = 256;
constexpr int kDefaultBlocks = 2048;                    // the cap of every grid: 8 blocks on each of 256 CUs
constexpr int kLanes = 8;                               // lanes that share one frontier node's row
constexpr int kRoundsPerWait = SC_GRAPH_ROUNDS_PER_WAIT;  // rounds enqueued between two looks at the header
constexpr size_t kKeepMax = (size_t)1 << 30;            // work buffers above this are given back when the call ends
constexpr unsigned long long kInfBits = 0x7FF0000000000000ull;

thread_local UnitError g_err;
std::atomic<int> g_blocks{0};  // sc_graph_set_blocks

enum : unsigned { kBadIndex = 1, kBadOffsets = 2, kBadWeight = 4, kBadExtra = 8, kBadExtraWeight = 16, kBadLabel = 32 };

// The arcs as the caller gave them, in device memory: E places of rows, then M extra pairs.
struct Arcs {
    const int64_t *offsets;  // CSR [N + 1], or NULL: rows of row_len places
    const int32_t *index;    // [E]
    const double *w;         // [E] or NULL (components)
    const int32_t *extra;    // [M][2] or NULL
    const double *extra_w;   // [M] or NULL
    int64_t E, M;
    int N, row_len, squared;
};

struct Header {
    unsigned int cnt[3];  // round r reads cnt[r % 3], appends to cnt[(r + 1) % 3], clears cnt[(r + 2) % 3]
    unsigned int rounds;  // rounds that found a frontier
};

int grid_for(int64_t work) {
    const int cap = g_blocks.load() > 0 ? g_blocks.load() : kDefaultBlocks;
    return (int)std::max<int64_t>(1, std::min<int64_t>((work + kB - 1) / kB, cap));
}

__device__ __forceinline__ bool weight_ok(double x) { return x >= 0.0 && x != __longlong_as_double((long long)kInfBits); }

// The row of place e of a CSR: the last i with offsets[i] <= e (rows before it may be empty).  offsets rise from 0
// to E > e (judged before), so 0 <= i < N.  At most 32 steps.
__device__ __forceinline__ int row_of(const int64_t *__restrict__ offsets, int N, int64_t e) {
    int lo = 0, hi = N;  // offsets[lo] <= e < offsets[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// Arc t of E + M: its two ends and weight; false for an unused place and a self-arc (rule G1: they change nothing).
__device__ __forceinline__ bool arc_of(const Arcs &g, int64_t t, int &i, int &j, double &w) {
    if (t < g.E) {
        j = g.index[t];
        if (j < 0) return false;
        i = g.row_len ? (int)(t / g.row_len) : row_of(g.offsets, g.N, t);
        if (g.w) w = g.squared ? sqrt(g.w[t]) : g.w[t];
    } else {
        const int64_t m = t - g.E;
        i = g.extra[2 * m];
        j = g.extra[2 * m + 1];
        if (g.extra_w) w = g.extra_w[m];
    }
    return i != j;
}

// ---- the judge of device inputs (rule G4) ------------------------------------------------------------------------
// Reads every array within its stated length only, whatever it holds; the entry waits for the flag before any other
// launch touches the arrays.  labels: NULL, or the N labels of sc_graph_quotient, each below L (rule Q6).
__global__ __launch_bounds__(kB) void graph_flags_kernel(Arcs g, const int32_t *__restrict__ labels, int L, unsigned int *flag) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    int64_t work = g.E > g.M ? g.E : g.M;
    if ((g.offsets || labels) && work < (int64_t)g.N + 1) work = (int64_t)g.N + 1;
    unsigned bad = 0;
    for (int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x; t < work; t += stride) {
        if (labels && t < g.N && labels[t] >= L) bad |= kBadLabel;
        if (t < g.E) {
            const int j = g.index[t];
            if (j >= g.N || j < (g.row_len ? -1 : 0)) bad |= kBadIndex;
            if (g.w && j >= 0 && !weight_ok(g.w[t])) bad |= kBadWeight;
        }
        if (g.offsets && t <= g.N) {
            const int64_t o = g.offsets[t];
            if ((t == 0 && o != 0) || (t == g.N && o != g.E) || (t < g.N && g.offsets[t + 1] < o)) bad |= kBadOffsets;
        }
        if (t < g.M) {
            const int a = g.extra[2 * t], b = g.extra[2 * t + 1];
            if (a < 0 || a >= g.N || b < 0 || b >= g.N) bad |= kBadExtra;
            if (g.extra_w && !weight_ok(g.extra_w[t])) bad |= kBadExtraWeight;
        }
    }
    if (bad) atomicOr(flag, bad);
}

// ---- the symmetric adjacency -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kB) void graph_degree_kernel(Arcs g, unsigned long long *__restrict__ deg) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x; t < g.E + g.M; t += stride) {
        int i, j;
        double w;
        if (!arc_of(g, t, i, j, w)) continue;
        atomicAdd(&deg[i], 1ull);
        atomicAdd(&deg[j], 1ull);
    }
}

// cursor = a copy of start; afterwards cursor[v] == start[v + 1].  The order inside a row is whatever the atomics
// give; no result depends on it.
__global__ __launch_bounds__(kB) void graph_scatter_kernel(Arcs g, unsigned long long *__restrict__ cursor, int32_t *__restrict__ nbr,
                                                           double *__restrict__ wgt) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x; t < g.E + g.M; t += stride) {
        int i, j;
        double w = 0.0;
        if (!arc_of(g, t, i, j, w)) continue;
        const unsigned long long a = atomicAdd(&cursor[i], 1ull), b = atomicAdd(&cursor[j], 1ull);
        nbr[a] = j;
        wgt[a] = w;
        nbr[b] = i;
        wgt[b] = w;
    }
}

// ---- the rounds --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kB) void graph_init_kernel(int N, int root, unsigned long long *__restrict__ d, unsigned int *__restrict__ stamp,
                                                        int *__restrict__ front0, Header *__restrict__ h) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t v = (int64_t)blockIdx.x * kB + threadIdx.x; v < N; v += stride) {
        d[v] = v == root ? 0ull : kInfBits;
        stamp[v] = 0xFFFFFFFFu;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        front0[0] = root;
        h->cnt[0] = 1;
        h->cnt[1] = h->cnt[2] = 0;
        h->rounds = 0;
    }
}

// Round r: kLanes lanes share each node u of the frontier; each takes every kLanes-th arc (u, v, w) and lowers d[v] to
// fl(d[u] + w).  A node whose d fell enters the next frontier once: the first lane to put r into its stamp.  The
// frontier's length was complete when this launch began (the launch before wrote it), nobody writes it now.
__global__ __launch_bounds__(kB) void graph_round_kernel(unsigned int r, Header *h, const int *__restrict__ fin, int *__restrict__ fout,
                                                         const unsigned long long *__restrict__ start, const int32_t *__restrict__ nbr,
                                                         const double *__restrict__ wgt, unsigned long long *d, unsigned int *stamp) {
    const unsigned int n = h->cnt[r % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        h->cnt[(r + 2) % 3] = 0;  // read by round r - 1, appended to by round r + 1; cleared by empty rounds too
        if (n) h->rounds = r + 1;
    }
    if (n == 0) return;
    unsigned int *next = &h->cnt[(r + 1) % 3];
    const unsigned int groups = gridDim.x * (kB / kLanes), lane = threadIdx.x % kLanes;
    for (unsigned int q = blockIdx.x * (kB / kLanes) + threadIdx.x / kLanes; q < n; q += groups) {
        const int u = fin[q];
        const double du = __longlong_as_double((long long)__hip_atomic_load(&d[u], DB_RLX));
        const unsigned long long a = start[u], b = start[u + 1];
        for (unsigned long long s = a + lane; s < b; s += kLanes) {
            const int v = nbr[s];
            const unsigned long long cand = (unsigned long long)__double_as_longlong(du + wgt[s]);
            if (cand >= __hip_atomic_load(&d[v], DB_RLX)) continue;  // most arcs lower nothing: no read-modify-write for them
            if (cand < __hip_atomic_fetch_min(&d[v], cand, DB_RLX) && __hip_atomic_exchange(&stamp[v], r, DB_RLX) != r)
                fout[__hip_atomic_fetch_add(next, 1u, DB_RLX)] = v;
        }
    }
}

// ---- components --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kB) void graph_parent_kernel(int N, int *__restrict__ parent) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t v = (int64_t)blockIdx.x * kB + threadIdx.x; v < N; v += stride) parent[v] = (int)v;
}

__global__ __launch_bounds__(kB) void graph_link_kernel(Arcs g, const int32_t *__restrict__ key, int *parent) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x; t < g.E + g.M; t += stride) {
        int i, j;
        double w;
        if (!arc_of(g, t, i, j, w)) continue;
        if (key) {
            const int ki = key[i];
            if (ki < 0 || ki != key[j]) continue;
        }
        unite(parent, i, j);
    }
}

// parent[] is final here (a kernel boundary lies behind the link launch) and is only read: plain loads.
__global__ __launch_bounds__(kB) void graph_flatten_kernel(int N, const int32_t *__restrict__ key, const int *__restrict__ parent,
                                                           int *__restrict__ rootof, int *__restrict__ isroot) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t v = (int64_t)blockIdx.x * kB + threadIdx.x; v < N; v += stride) {
        int r = (int)v;
        while (parent[r] != r) r = parent[r];
        const bool out = key && key[v] < 0;
        rootof[v] = out ? -1 : r;
        isroot[v] = !out && r == (int)v ? 1 : 0;
    }
}

// rank = exclusive sum of isroot: the number of roots with a smaller index, i.e. the component's place among the
// components ordered by their smallest member (roots are smallest members)
__global__ __launch_bounds__(kB) void graph_labels_kernel(int N, const int *__restrict__ rootof, const int *__restrict__ isroot,
                                                          const int *__restrict__ rank, int32_t *__restrict__ labels, int32_t *__restrict__ ncomp) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t v = (int64_t)blockIdx.x * kB + threadIdx.x; v < N; v += stride) {
        const int r = rootof[v];
        labels[v] = r < 0 ? -1 : rank[r];
        if (v == N - 1) *ncomp = rank[v] + isroot[v];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
WorkSlot g_slots[kUnitDevices];

bool host_weight_ok(double x) { return x >= 0.0 && std::isfinite(x); }

const char kBadLabelText[] = "label outside .. L - 1 (a negative label is an outside node)";

const char *flag_text(unsigned bad) {
    if (bad & kBadOffsets) return "offsets must rise from 0 to E";
    if (bad & kBadIndex) return "index outside -1 .. N - 1 (-1 only in rows of fixed length)";
    if (bad & kBadWeight) return "weights must be finite and not negative";
    if (bad & kBadExtra) return "extra pair outside 0 .. N - 1";
    if (bad & kBadLabel) return kBadLabelText;
    return "extra weights must be finite and not negative";
}

// What both entries refuse without reading an array, then (host arrays) what they hold.
int judge(int64_t N, const int64_t *offsets, int row_len, const int32_t *index, const double *weights, int want_weights, int64_t E,
          const int32_t *extra, const double *extra_w, int64_t M, int on_device, int device) {
    if (N < 0 || N >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "N must be 0 .. 2^31 - 1");
    if (E < 0 || E >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "E must be 0 .. 2^31 - 1");
    if (M < 0 || M >= ((int64_t)1 << 31) - E) return g_err.fail(SC_ERR_INVALID, "E + M must be 0 .. 2^31 - 1");
    if (device < 0 || device >= kUnitDevices) return g_err.fail(SC_ERR_INVALID, "device ordinal out of range");
    if (!offsets && (row_len < 1 || E != N * (int64_t)row_len))
        return g_err.fail(SC_ERR_INVALID, "rows of fixed length: row_len must be at least 1 and E == N * row_len");
    if (E > 0 && (!index || (want_weights && !weights))) return g_err.fail(SC_ERR_INVALID, "null argument (index, weights)");
    if (M > 0 && (!extra || (want_weights && !extra_w))) return g_err.fail(SC_ERR_INVALID, "null argument (extra, extra_w)");
    if (on_device) return SC_OK;
    unsigned bad = 0;
    if (offsets) {
        if (offsets[0] != 0 || offsets[N] != E) bad |= kBadOffsets;
        for (int64_t i = 0; i < N && !bad; ++i)
            if (offsets[i + 1] < offsets[i]) bad |= kBadOffsets;
    }
    for (int64_t e = 0; e < E && !bad; ++e) {
        const int j = index[e];
        if (j >= N || j < (offsets ? 0 : -1)) bad |= kBadIndex;
        else if (want_weights && j >= 0 && !host_weight_ok(weights[e])) bad |= kBadWeight;
    }
    for (int64_t m = 0; m < M && !bad; ++m) {
        if (extra[2 * m] < 0 || extra[2 * m] >= N || extra[2 * m + 1] < 0 || extra[2 * m + 1] >= N) bad |= kBadExtra;
        else if (want_weights && !host_weight_ok(extra_w[m])) bad |= kBadExtraWeight;
    }
    return bad ? g_err.fail(SC_ERR_INVALID, flag_text(bad)) : SC_OK;
}

// Buffers above kKeepMax are not kept between calls (vol2pcd's policy).
void give_back_if_large(UnitCall &call) {
    WorkSlot &sl = call.sl;
    if (sl.cap <= kKeepMax || !sl.base) return;
    (void)hipStreamSynchronize(call.stream);
    (void)hipFree(sl.base);
    sl.base = nullptr;
    sl.cap = 0;
}

// The caller's arrays where the kernels read them: in place, or copied behind `w + at[...]`.
struct Staged {
    size_t offsets = 0, index = 0, weights = 0, extra = 0, extra_w = 0;
    void plan(Layout &lay, int on_device, int64_t N, bool csr, int64_t E, bool want_weights, int64_t M) {
        if (on_device) return;
        offsets = lay.take(csr ? (size_t)(N + 1) * 8 : 0);
        index = lay.take((size_t)E * 4);
        weights = lay.take(want_weights ? (size_t)E * 8 : 0);
        extra = lay.take((size_t)M * 8);
        extra_w = lay.take(want_weights ? (size_t)M * 8 : 0);
    }
};

}  // namespace

extern "C" {

const char *sc_graph_error(void) { return g_err.msg; }

void sc_graph_set_blocks(int blocks) { g_blocks.store(blocks > 0 ? blocks : 0); }

int sc_graph_distances(int64_t N, const int64_t *offsets, int row_len, const int32_t *index, const double *weights, int64_t E,
                       int weights_squared, const int32_t *extra, const double *extra_w, int64_t M, int on_device, int64_t root,
                       int device, double *dist_out, int64_t *rounds_out, void *hip_stream) {
    if (!dist_out) return g_err.fail(SC_ERR_INVALID, "null argument (dist_out)");
    if (judge(N, offsets, row_len, index, weights, 1, E, extra, extra_w, M, on_device, device) != SC_OK) return SC_ERR_INVALID;
    if (root < 0 || root >= N) return g_err.fail(SC_ERR_INVALID, "root must be 0 .. N - 1");

    const int n = (int)N;
    const int64_t places = 2 * (E + M);  // directed arcs, at most
    int rc = SC_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    UnitCall call(g_err, g_slots, device, stream, rc);
    size_t tmp = 0;
    unsigned int bad = 0;
    Header head = {{0, 0, 0}, 0};
    int64_t launched = 0;

    Layout lay;
    const size_t o_hdr = lay.take(256);  // the flag, the Header at +64
    const size_t o_deg = lay.take((size_t)(N + 1) * 8), o_start = lay.take((size_t)(N + 1) * 8);
    const size_t o_nbr = lay.take((size_t)places * 4), o_wgt = lay.take((size_t)places * 8);
    const size_t o_f0 = lay.take((size_t)N * 4), o_f1 = lay.take((size_t)N * 4), o_stamp = lay.take((size_t)N * 4);
    const size_t o_d = lay.take(on_device ? 0 : (size_t)N * 8);
    Staged at;
    at.plan(lay, on_device, N, offsets != nullptr, E, true, M);
    size_t o_tmp = 0;

    if ((rc = call.enter()) != SC_OK) goto done;
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, n + 1, stream));
    o_tmp = lay.take(tmp);
    if ((rc = call.grow(lay.total)) != SC_OK) goto done;
    {
        char *const w = call.sl.base;
        unsigned int *flag = reinterpret_cast<unsigned int *>(w + o_hdr);
        Header *h = reinterpret_cast<Header *>(w + o_hdr + 64);
        unsigned long long *deg = reinterpret_cast<unsigned long long *>(w + o_deg), *start = reinterpret_cast<unsigned long long *>(w + o_start);
        int32_t *nbr = reinterpret_cast<int32_t *>(w + o_nbr);
        double *wgt = reinterpret_cast<double *>(w + o_wgt);
        int *front[2] = {reinterpret_cast<int *>(w + o_f0), reinterpret_cast<int *>(w + o_f1)};
        unsigned int *stamp = reinterpret_cast<unsigned int *>(w + o_stamp);
        unsigned long long *d = reinterpret_cast<unsigned long long *>(on_device ? (char *)dist_out : w + o_d);
        Arcs g;
        g.offsets = offsets ? (on_device ? offsets : reinterpret_cast<const int64_t *>(w + at.offsets)) : nullptr;
        g.index = on_device ? index : reinterpret_cast<const int32_t *>(w + at.index);
        g.w = on_device ? weights : reinterpret_cast<const double *>(w + at.weights);
        g.extra = on_device ? extra : reinterpret_cast<const int32_t *>(w + at.extra);
        g.extra_w = on_device ? extra_w : reinterpret_cast<const double *>(w + at.extra_w);
        g.E = E;
        g.M = M;
        g.N = n;
        g.row_len = offsets ? 0 : row_len;
        g.squared = weights_squared ? 1 : 0;

        UNIT_TRY(call.sl.wait(stream));
        if (!on_device) {
            if (offsets) UNIT_TRY(hipMemcpyAsync(w + at.offsets, offsets, (size_t)(N + 1) * 8, hipMemcpyHostToDevice, stream));
            if (E) UNIT_TRY(hipMemcpyAsync(w + at.index, index, (size_t)E * 4, hipMemcpyHostToDevice, stream));
            if (E) UNIT_TRY(hipMemcpyAsync(w + at.weights, weights, (size_t)E * 8, hipMemcpyHostToDevice, stream));
            if (M) UNIT_TRY(hipMemcpyAsync(w + at.extra, extra, (size_t)M * 8, hipMemcpyHostToDevice, stream));
            if (M) UNIT_TRY(hipMemcpyAsync(w + at.extra_w, extra_w, (size_t)M * 8, hipMemcpyHostToDevice, stream));
        } else {  // device arrays: the first kernel is the judge
            UNIT_TRY(hipMemsetAsync(flag, 0, 64, stream));
            hipLaunchKernelGGL(graph_flags_kernel, dim3(grid_for(std::max(std::max(E, M), N + 1))), dim3(kB), 0, stream, g, nullptr, 0, flag);
            UNIT_TRY(hipGetLastError());
            UNIT_TRY(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, stream));
            UNIT_TRY(call.sl.record(stream));
            UNIT_TRY(hipStreamSynchronize(stream));
            if (bad != 0u) {
                rc = g_err.fail(SC_ERR_INVALID, flag_text(bad));
                goto done;
            }
        }

        UNIT_TRY(hipMemsetAsync(deg, 0, (size_t)(N + 1) * 8, stream));
        hipLaunchKernelGGL(graph_degree_kernel, dim3(grid_for(E + M)), dim3(kB), 0, stream, g, deg);
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(w + o_tmp, tmp, deg, start, n + 1, stream));
        UNIT_TRY(hipMemcpyAsync(deg, start, (size_t)(N + 1) * 8, hipMemcpyDeviceToDevice, stream));  // the cursors
        hipLaunchKernelGGL(graph_scatter_kernel, dim3(grid_for(E + M)), dim3(kB), 0, stream, g, deg, nbr, wgt);
        hipLaunchKernelGGL(graph_init_kernel, dim3(grid_for(N)), dim3(kB), 0, stream, n, (int)root, d, stamp, front[0], h);
        UNIT_TRY(hipGetLastError());

        // A lowering walk visits no node twice (sums never decrease), so it has fewer than N arcs: the frontier of round N
        // is empty.  Rounds on an empty frontier return at once.
        const dim3 round_grid(grid_for(N * kLanes));
        for (;;) {
            for (int q = 0; q < kRoundsPerWait; ++q, ++launched)
                hipLaunchKernelGGL(graph_round_kernel, round_grid, dim3(kB), 0, stream, (unsigned int)launched, h, front[launched & 1],
                                   front[(launched + 1) & 1], start, nbr, wgt, d, stamp);
            UNIT_TRY(hipGetLastError());
            UNIT_TRY(hipMemcpyAsync(&head, h, sizeof head, hipMemcpyDeviceToHost, stream));
            UNIT_TRY(call.sl.record(stream));
            UNIT_TRY(hipStreamSynchronize(stream));
            if (head.cnt[launched % 3] == 0) break;
            if (launched >= N) {
                rc = g_err.fail(SC_ERR_DEVICE, "the frontier is not empty after N rounds");
                goto done;
            }
        }
        if (!on_device) {
            UNIT_TRY(hipMemcpyAsync(dist_out, d, (size_t)N * 8, hipMemcpyDeviceToHost, stream));
            UNIT_TRY(call.sl.record(stream));
            UNIT_TRY(hipStreamSynchronize(stream));
        }
        if (rounds_out) *rounds_out = head.rounds;
    }

done:
    give_back_if_large(call);
    return rc;
}

int sc_graph_components(int64_t N, const int64_t *offsets, int row_len, const int32_t *index, int64_t E, const int32_t *extra, int64_t M,
                        const int32_t *key, int on_device, int device, int32_t *labels_out, int32_t *ncomponents_out, void *hip_stream) {
    if (!labels_out) return g_err.fail(SC_ERR_INVALID, "null argument (labels_out)");
    if (judge(N, offsets, row_len, index, nullptr, 0, E, extra, nullptr, M, on_device, device) != SC_OK) return SC_ERR_INVALID;
    if (N == 0) {
        if (ncomponents_out) *ncomponents_out = 0;
        return SC_OK;
    }

    const int n = (int)N;
    int rc = SC_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    UnitCall call(g_err, g_slots, device, stream, rc);
    size_t tmp = 0;
    unsigned int bad = 0;
    int32_t ncomp = 0;

    Layout lay;
    const size_t o_hdr = lay.take(256);  // the flag, the count at +64
    const size_t o_parent = lay.take((size_t)N * 4), o_rootof = lay.take((size_t)N * 4), o_isroot = lay.take((size_t)N * 4),
                 o_rank = lay.take((size_t)N * 4);
    const size_t o_key = lay.take(on_device || !key ? 0 : (size_t)N * 4), o_lab = lay.take(on_device ? 0 : (size_t)N * 4);
    Staged at;
    at.plan(lay, on_device, N, offsets != nullptr, E, false, M);
    size_t o_tmp = 0;

    if ((rc = call.enter()) != SC_OK) goto done;
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, (const int *)nullptr, (int *)nullptr, n, stream));
    o_tmp = lay.take(tmp);
    if ((rc = call.grow(lay.total)) != SC_OK) goto done;
    {
        char *const w = call.sl.base;
        unsigned int *flag = reinterpret_cast<unsigned int *>(w + o_hdr);
        int32_t *ncomp_d = reinterpret_cast<int32_t *>(w + o_hdr + 64);
        int *parent = reinterpret_cast<int *>(w + o_parent), *rootof = reinterpret_cast<int *>(w + o_rootof),
            *isroot = reinterpret_cast<int *>(w + o_isroot), *rank = reinterpret_cast<int *>(w + o_rank);
        const int32_t *key_d = !key ? nullptr : on_device ? key : reinterpret_cast<const int32_t *>(w + o_key);
        int32_t *lab_d = on_device ? labels_out : reinterpret_cast<int32_t *>(w + o_lab);
        Arcs g;
        g.offsets = offsets ? (on_device ? offsets : reinterpret_cast<const int64_t *>(w + at.offsets)) : nullptr;
        g.index = on_device ? index : reinterpret_cast<const int32_t *>(w + at.index);
        g.w = nullptr;
        g.extra = on_device ? extra : reinterpret_cast<const int32_t *>(w + at.extra);
        g.extra_w = nullptr;
        g.E = E;
        g.M = M;
        g.N = n;
        g.row_len = offsets ? 0 : row_len;
        g.squared = 0;

        UNIT_TRY(call.sl.wait(stream));
        if (!on_device) {
            if (offsets) UNIT_TRY(hipMemcpyAsync(w + at.offsets, offsets, (size_t)(N + 1) * 8, hipMemcpyHostToDevice, stream));
            if (E) UNIT_TRY(hipMemcpyAsync(w + at.index, index, (size_t)E * 4, hipMemcpyHostToDevice, stream));
            if (M) UNIT_TRY(hipMemcpyAsync(w + at.extra, extra, (size_t)M * 8, hipMemcpyHostToDevice, stream));
            if (key) UNIT_TRY(hipMemcpyAsync(w + o_key, key, (size_t)N * 4, hipMemcpyHostToDevice, stream));
        } else {  // device arrays: the first kernel is the judge
            UNIT_TRY(hipMemsetAsync(flag, 0, 64, stream));
            hipLaunchKernelGGL(graph_flags_kernel, dim3(grid_for(std::max(std::max(E, M), N + 1))), dim3(kB), 0, stream, g, nullptr, 0, flag);
            UNIT_TRY(hipGetLastError());
            UNIT_TRY(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, stream));
            UNIT_TRY(call.sl.record(stream));
            UNIT_TRY(hipStreamSynchronize(stream));
            if (bad != 0u) {
                rc = g_err.fail(SC_ERR_INVALID, flag_text(bad));
                goto done;
            }
        }

        hipLaunchKernelGGL(graph_parent_kernel, dim3(grid_for(N)), dim3(kB), 0, stream, n, parent);
        hipLaunchKernelGGL(graph_link_kernel, dim3(grid_for(E + M)), dim3(kB), 0, stream, g, key_d, parent);
        hipLaunchKernelGGL(graph_flatten_kernel, dim3(grid_for(N)), dim3(kB), 0, stream, n, key_d, parent, rootof, isroot);
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(w + o_tmp, tmp, isroot, rank, n, stream));
        hipLaunchKernelGGL(graph_labels_kernel, dim3(grid_for(N)), dim3(kB), 0, stream, n, rootof, isroot, rank, lab_d, ncomp_d);
        UNIT_TRY(hipGetLastError());
        if (!on_device) UNIT_TRY(hipMemcpyAsync(labels_out, lab_d, (size_t)N * 4, hipMemcpyDeviceToHost, stream));
        if (ncomponents_out) UNIT_TRY(hipMemcpyAsync(&ncomp, ncomp_d, 4, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        if (!on_device || ncomponents_out) {
            UNIT_TRY(hipStreamSynchronize(stream));
            if (ncomponents_out) *ncomponents_out = ncomp;
        }
    }

done:
    give_back_if_large(call);
    return rc;
}

void sc_graph_release(void) { release_slots(g_slots); }

}  // extern "C"

#include "graph_quotient.inl"  // sc_graph_quotient
#include "graph_connect.inl"   // sc_graph_connect
