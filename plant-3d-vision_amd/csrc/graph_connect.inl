// graph_connect.inl -- the edges that connect the labels of a cloud to the root's, the fourth entry of
// graph.hip: Prim's algorithm over the labels, started at the root's, in its incremental form.  The rules C1..C5 are the
// contract in include/spacecarve.h.  Included at the end of graph.hip: it uses that file's grid_for, the slots,
// give_back_if_large and, through graph_quotient.inl, cub_run.
//
// Once per call the points are laid out in label order (count, scan, scatter: the places inside a label are handed out
// by integer atomics, and rule C2 makes that order irrelevant), so every label is one contiguous segment.  Then one
// launch per round: every block reduces the previous round's per-block minima of (d2, i, j) to the chosen edge -- the
// order is total, so all blocks agree -- block 0 stores it, and every point outside R that the block owns is offered
// the segment of the label that joined and lowers its own best (d2, j).  A point has one owner: no atomic.  The block's
// minimum over its outside points goes into the other of two partial buffers.  The kernel boundary is the only
// synchronisation between blocks; no floating-point atomic, no wavefront waits on another, no kernel spins; every loop
// is bounded by a count fixed before it starts.

namespace {

constexpr int kTile = 1024;          // points of the joined segment staged in LDS at a time (28 KiB)
constexpr int kNone = 0x7FFFFFFF;    // best_j of a point that has seen no inside point; the i and j of "nobody outside"
constexpr int kInside = -1;          // best_j of a point of R
constexpr int kWaves = kB / 64;

enum : unsigned { kBadConnectLabel = 1, kBadConnectPoint = 2 };

struct CHeader {
    int C;        // labels that have members
    int emitted;  // edges written so far
};

struct CPart {  // a key (d2, i, j); i == kNone: none
    double d2;
    int i, j;
};

__device__ __forceinline__ bool key_less(double da, int ia, int ja, double db, int ib, int jb) {
    return da < db || (da == db && (ia < ib || (ia == ib && ja < jb)));
}

__device__ __forceinline__ void part_min(CPart &a, double d2, int i, int j) {
    if (key_less(d2, i, j, a.d2, a.i, a.j)) {
        a.d2 = d2;
        a.i = i;
        a.j = j;
    }
}

// the least key of the wavefront, in every lane
__device__ __forceinline__ void wave_min(CPart &a) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double d2 = __shfl_xor(a.d2, m);
        const int i = __shfl_xor(a.i, m), j = __shfl_xor(a.j, m);
        part_min(a, d2, i, j);
    }
}

// the least key of the block, in every thread; slots: kWaves places of LDS
__device__ __forceinline__ void block_min(CPart &a, CPart *slots) {
    wave_min(a);
    __syncthreads();  // the slots may still be read from an earlier use
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = a;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) part_min(a, slots[w].d2, slots[w].i, slots[w].j);
}

// ---- the judge of device inputs (rule C3): reads labels[0 .. N) and points[0 .. 3 N), nothing else ------------------
__global__ __launch_bounds__(kB) void connect_flags_kernel(int N, int L, const int32_t *__restrict__ labels, const double *__restrict__ points,
                                                           unsigned int *flag) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    unsigned bad = 0;
    for (int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x; t < 3 * (int64_t)N; t += stride) {
        if (t < N && (labels[t] < 0 || labels[t] >= L)) bad |= kBadConnectLabel;
        if (!(fabs(points[t]) <= DBL_MAX)) bad |= kBadConnectPoint;
    }
    if (bad) atomicOr(flag, bad);
}

// ---- the label order ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kB) void connect_count_kernel(int N, const int32_t *__restrict__ labels, int *cnt) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t v = (int64_t)blockIdx.x * kB + threadIdx.x; v < N; v += stride) (void)__hip_atomic_fetch_add(&cnt[labels[v]], 1, DB_RLX);
}

// cursor = a copy of start.  Also the number of labels with members (h->C, zeroed before) and the state of every place.
__global__ __launch_bounds__(kB) void connect_scatter_kernel(int N, int L, const int32_t *__restrict__ labels, const double *__restrict__ points,
                                                             const int *__restrict__ cnt, int *cursor, double *__restrict__ sx,
                                                             double *__restrict__ sy, double *__restrict__ sz, int *__restrict__ sid,
                                                             double *__restrict__ bd, int *__restrict__ bj, CHeader *h) {
    const int64_t stride = (int64_t)gridDim.x * kB;
    int used = 0;
    for (int64_t v = (int64_t)blockIdx.x * kB + threadIdx.x; v < N; v += stride) {
        const int p = __hip_atomic_fetch_add(&cursor[labels[v]], 1, DB_RLX);
        sx[p] = points[3 * v];
        sy[p] = points[3 * v + 1];
        sz[p] = points[3 * v + 2];
        sid[p] = (int)v;
        bd[v] = __longlong_as_double((long long)kInfBits);  // (bd and bj belong to places, and every place is some v)
        bj[v] = kNone;
        if (v < L && cnt[v] > 0) ++used;
    }
    if (used) (void)__hip_atomic_fetch_add(&h->C, used, DB_RLX);
}

// ---- one round -----------------------------------------------------------------------------------------------------
// Round 0 lets the root's label join; round r > 0 writes edge r - 1 and lets its outside end's label join.  Place p
// belongs to block p % gridDim.x; a block takes its places kB at a time.
__global__ __launch_bounds__(kB) void connect_round_kernel(int r, int N, int root, const int32_t *__restrict__ labels,
                                                           const int *__restrict__ start, const double *__restrict__ sx,
                                                           const double *__restrict__ sy, const double *__restrict__ sz,
                                                           const int *__restrict__ sid, double *__restrict__ bd, int *__restrict__ bj,
                                                           const CPart *__restrict__ pin, CPart *__restrict__ pout,
                                                           int32_t *__restrict__ edges, double *__restrict__ weights, CHeader *h) {
    __shared__ double tx[kTile], ty[kTile], tz[kTile];
    __shared__ int tj[kTile];
    __shared__ CPart slots[kWaves];
    __shared__ double got_d[kB];
    __shared__ int got_j[kB], list[kB], count;

    const double inf = __longlong_as_double((long long)kInfBits);
    const int G = (int)gridDim.x, lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    int joined;
    if (r == 0) {
        joined = labels[root];
    } else {
        if (r > h->C - 1) return;  // every label has joined (C was written before the first round)
        CPart best = {inf, kNone, kNone};
        for (int q = (int)threadIdx.x; q < G; q += kB) part_min(best, pin[q].d2, pin[q].i, pin[q].j);
        block_min(best, slots);
        if (best.i == kNone) return;  // nobody outside
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            edges[2 * (int64_t)(r - 1)] = best.i;
            edges[2 * (int64_t)(r - 1) + 1] = best.j;
            weights[r - 1] = sqrt(best.d2);
            h->emitted = r;
        }
        joined = labels[best.i];
    }
    const int seg_a = start[joined], seg_b = start[joined + 1], S = seg_b - seg_a;

    CPart mine = {inf, kNone, kNone};  // the least key over this thread's outside points
    for (int64_t base = blockIdx.x; base < N; base += (int64_t)G * kB) {
        const int64_t p = base + (int64_t)threadIdx.x * G;
        __syncthreads();  // count, list and got_* of the trip before have been read
        if (threadIdx.x == 0) count = 0;
        __syncthreads();
        bool outside = false;
        double ax = 0.0, ay = 0.0, az = 0.0, d = inf;
        int j = kNone;
        if (p < N) {
            j = bj[p];
            if (j != kInside) {
                if (p >= seg_a && p < seg_b) {
                    bj[p] = kInside;
                } else {
                    outside = true;
                    d = bd[p];
                    ax = sx[p];
                    ay = sy[p];
                    az = sz[p];
                    list[atomicAdd(&count, 1)] = (int)threadIdx.x;
                }
            }
        }
        __syncthreads();
        const int n = count;  // the block's outside points of this trip
        if (n == 0) continue;
        // Few points against a long segment: a wavefront per point, its lanes stride the segment.  Many points
        // against a short one: a thread per point, the segment staged through LDS.  The costs compared are, per
        // wavefront, n / kWaves walks of S / 64 steps and a cross-lane minimum against one walk of S steps.
        if ((int64_t)n * (S / 64 + 8) < (int64_t)kWaves * S) {
            for (int e = wave; e < n; e += kWaves) {
                const int t = list[e];
                const int64_t q0 = base + (int64_t)t * G;
                const double qx = sx[q0], qy = sy[q0], qz = sz[q0];
                CPart w = {inf, 0, kNone};
                for (int q = seg_a + lane; q < seg_b; q += 64) part_min(w, dist2(qx, qy, qz, sx[q], sy[q], sz[q]), 0, sid[q]);
                wave_min(w);
                if (lane == 0) {
                    got_d[t] = w.d2;
                    got_j[t] = w.j;
                }
            }
            __syncthreads();
            if (outside && key_less(got_d[threadIdx.x], 0, got_j[threadIdx.x], d, 0, j)) {
                d = got_d[threadIdx.x];
                j = got_j[threadIdx.x];
            }
        } else {
            for (int t0 = 0; t0 < S; t0 += kTile) {
                const int len = S - t0 < kTile ? S - t0 : kTile;
                __syncthreads();  // the tile before has been read
                for (int q = (int)threadIdx.x; q < len; q += kB) {
                    tx[q] = sx[seg_a + t0 + q];
                    ty[q] = sy[seg_a + t0 + q];
                    tz[q] = sz[seg_a + t0 + q];
                    tj[q] = sid[seg_a + t0 + q];
                }
                __syncthreads();
                if (outside)
                    for (int q = 0; q < len; ++q) {
                        const double c = dist2(ax, ay, az, tx[q], ty[q], tz[q]);
                        if (key_less(c, 0, tj[q], d, 0, j)) {
                            d = c;
                            j = tj[q];
                        }
                    }
            }
        }
        if (outside) {
            bd[p] = d;
            bj[p] = j;
            part_min(mine, d, sid[p], j);
        }
    }
    block_min(mine, slots);
    if (threadIdx.x == 0) pout[blockIdx.x] = mine;
}

}  // namespace

extern "C" int sc_graph_connect(int64_t N, const double *points, const int32_t *labels, int64_t L, int64_t root, int on_device, int device,
                                int32_t *edges_out, double *weights_out, int64_t *nedges_out, void *hip_stream) {
    if (N < 0 || N >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "N must be 0 .. 2^31 - 1");
    if (device < 0 || device >= kUnitDevices) return g_err.fail(SC_ERR_INVALID, "device ordinal out of range");
    if (!nedges_out) return g_err.fail(SC_ERR_INVALID, "null argument (nedges_out)");
    if (N == 0) {
        *nedges_out = 0;
        return SC_OK;
    }
    if (L < 1 || L > N) return g_err.fail(SC_ERR_INVALID, "L must be 1 .. N");
    if (root < 0 || root >= N) return g_err.fail(SC_ERR_INVALID, "root must be 0 .. N - 1");
    if (!points || !labels) return g_err.fail(SC_ERR_INVALID, "null argument (points, labels)");
    if (L > 1 && (!edges_out || !weights_out)) return g_err.fail(SC_ERR_INVALID, "null argument (edges_out, weights_out)");
    if (!on_device) {
        for (int64_t v = 0; v < N; ++v)
            if (labels[v] < 0 || labels[v] >= L) return g_err.fail(SC_ERR_INVALID, "label outside 0 .. L - 1");
        if (first_non_finite(g_err, points, N, "point") != SC_OK) return SC_ERR_INVALID;
    }

    const int n = (int)N, nl = (int)L;
    const int G = grid_for(N);  // the blocks of every round: a place's owner and the partial buffers depend on it
    const int64_t most = L - 1;  // edges, at most
    int rc = SC_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    UnitCall call(g_err, g_slots, device, stream, rc);
    size_t tmp_cap = 0;
    unsigned int bad = 0;
    CHeader head = {0, 0};
    int64_t launched = 0;

    Layout lay;
    const size_t o_hdr = lay.take(256);  // the flag, the CHeader at +64
    const size_t o_cnt = lay.take((size_t)(L + 1) * 4), o_start = lay.take((size_t)(L + 1) * 4), o_cursor = lay.take((size_t)(L + 1) * 4);
    const size_t o_sx = lay.take((size_t)N * 8), o_sy = lay.take((size_t)N * 8), o_sz = lay.take((size_t)N * 8), o_sid = lay.take((size_t)N * 4);
    const size_t o_bd = lay.take((size_t)N * 8), o_bj = lay.take((size_t)N * 4);
    const size_t o_p0 = lay.take((size_t)G * sizeof(CPart)), o_p1 = lay.take((size_t)G * sizeof(CPart));
    // copies of host arrays, and the outputs before they go home
    const size_t o_pts = lay.take(on_device ? 0 : (size_t)N * 24), o_lab = lay.take(on_device ? 0 : (size_t)N * 4);
    const size_t o_edges = lay.take(on_device ? 0 : (size_t)most * 8), o_w = lay.take(on_device ? 0 : (size_t)most * 8);
    size_t o_tmp = 0;

    if ((rc = call.enter()) != SC_OK) goto done;
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_cap, (const int *)nullptr, (int *)nullptr, nl + 1, stream));
    o_tmp = lay.take(tmp_cap);
    if ((rc = call.grow(lay.total)) != SC_OK) goto done;
    {
        char *const w = call.sl.base;
        unsigned int *flag = reinterpret_cast<unsigned int *>(w + o_hdr);
        CHeader *h = reinterpret_cast<CHeader *>(w + o_hdr + 64);
        int *cnt = reinterpret_cast<int *>(w + o_cnt), *start = reinterpret_cast<int *>(w + o_start), *cursor = reinterpret_cast<int *>(w + o_cursor);
        double *sx = reinterpret_cast<double *>(w + o_sx), *sy = reinterpret_cast<double *>(w + o_sy), *sz = reinterpret_cast<double *>(w + o_sz);
        int *sid = reinterpret_cast<int *>(w + o_sid), *bj = reinterpret_cast<int *>(w + o_bj);
        double *bd = reinterpret_cast<double *>(w + o_bd);
        CPart *part[2] = {reinterpret_cast<CPart *>(w + o_p0), reinterpret_cast<CPart *>(w + o_p1)};
        const double *pts_d = on_device ? points : reinterpret_cast<const double *>(w + o_pts);
        const int32_t *lab_d = on_device ? labels : reinterpret_cast<const int32_t *>(w + o_lab);
        int32_t *edges_d = on_device ? edges_out : reinterpret_cast<int32_t *>(w + o_edges);
        double *w_d = on_device ? weights_out : reinterpret_cast<double *>(w + o_w);

        UNIT_TRY(call.sl.wait(stream));
        UNIT_TRY(hipMemsetAsync(w + o_hdr, 0, 256, stream));
        if (!on_device) {
            UNIT_TRY(hipMemcpyAsync(w + o_pts, points, (size_t)N * 24, hipMemcpyHostToDevice, stream));
            UNIT_TRY(hipMemcpyAsync(w + o_lab, labels, (size_t)N * 4, hipMemcpyHostToDevice, stream));
        } else {  // device arrays: the first kernel is the judge
            hipLaunchKernelGGL(connect_flags_kernel, dim3(grid_for(3 * N)), dim3(kB), 0, stream, n, nl, lab_d, pts_d, flag);
            UNIT_TRY(hipGetLastError());
            UNIT_TRY(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, stream));
            UNIT_TRY(call.sl.record(stream));
            UNIT_TRY(hipStreamSynchronize(stream));
            if (bad != 0u) {
                rc = g_err.fail(SC_ERR_INVALID, bad & kBadConnectLabel ? "label outside 0 .. L - 1" : "non-finite coordinate in the points");
                goto done;
            }
        }

        // the label order: every label one segment of places start[l] .. start[l + 1]
        UNIT_TRY(hipMemsetAsync(cnt, 0, (size_t)(L + 1) * 4, stream));
        hipLaunchKernelGGL(connect_count_kernel, dim3(grid_for(N)), dim3(kB), 0, stream, n, lab_d, cnt);
        UNIT_TRY(cub_run(w + o_tmp, tmp_cap, [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, cnt, start, nl + 1, stream); }));
        UNIT_TRY(hipMemcpyAsync(cursor, start, (size_t)(L + 1) * 4, hipMemcpyDeviceToDevice, stream));
        hipLaunchKernelGGL(connect_scatter_kernel, dim3(grid_for(N)), dim3(kB), 0, stream, n, nl, lab_d, pts_d, cnt, cursor, sx, sy, sz, sid, bd, bj, h);
        UNIT_TRY(hipGetLastError());

        // Round 0 and at most L - 1 rounds that write an edge.  The first SC_GRAPH_ROUNDS_PER_WAIT of them are followed
        // by a look at the header, which brings C; then the C - 1 - (rounds run) that remain are enqueued in one go.
        // Rounds behind the last edge return at once.
        for (int pass = 0; pass < 2; ++pass) {
            const int64_t upto = pass == 0 ? std::min<int64_t>(kRoundsPerWait, L) : (int64_t)head.C;
            for (; launched < upto; ++launched)
                hipLaunchKernelGGL(connect_round_kernel, dim3(G), dim3(kB), 0, stream, (int)launched, n, (int)root, lab_d, start, sx, sy, sz, sid,
                                   bd, bj, part[(launched + 1) & 1], part[launched & 1], edges_d, w_d, h);
            UNIT_TRY(hipGetLastError());
            if (pass == 1 && !on_device && head.C > 1) {
                UNIT_TRY(hipMemcpyAsync(edges_out, edges_d, (size_t)(head.C - 1) * 8, hipMemcpyDeviceToHost, stream));
                UNIT_TRY(hipMemcpyAsync(weights_out, w_d, (size_t)(head.C - 1) * 8, hipMemcpyDeviceToHost, stream));
            }
            UNIT_TRY(hipMemcpyAsync(&head, h, sizeof head, hipMemcpyDeviceToHost, stream));
            UNIT_TRY(call.sl.record(stream));
            UNIT_TRY(hipStreamSynchronize(stream));
            if (head.C < 1 || head.C > L || head.emitted < 0 || head.emitted > head.C - 1) {
                rc = g_err.fail(SC_ERR_DEVICE, "label or edge count out of range");
                goto done;
            }
            if (pass == 0 && head.emitted == head.C - 1 && (on_device || head.C == 1)) break;  // finished, and nothing goes home
        }
        if (head.emitted != head.C - 1) {
            rc = g_err.fail(SC_ERR_DEVICE, "labels are left outside after L - 1 rounds");
            goto done;
        }
        *nedges_out = head.emitted;
    }

done:
    give_back_if_large(call);
    return rc;
}
