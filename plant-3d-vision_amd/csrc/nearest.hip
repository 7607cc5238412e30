// nearest.hip -- the nearest point of another cloud, for the point-cloud evaluations.
//
// Replaces open3d's compute_point_cloud_distance, evaluate_registration and the one-query-per-point KDTreeFlann loop
// of CompareSegmentedPointClouds (plant3dvision/metrics.py:16-95, :384-519; tasks/evaluation.py:278-353) for Q float64
// queries against P float64 targets.  PARITY UNPINNED: open3d is not available, this restates what
// nanoflann's search computes in an order-free form:
//   N1. d2(q, t) = ((dx dx) + (dy dy)) + (dz dz) in IEEE binary64 without contraction (-ffp-contract=off), dx = qx - tx;
//   N2. the nearest target is the t of least d2; among equal d2 the smallest target index wins;
//   N3. with max_distance, a query is matched iff d2 < fl(max_distance * max_distance) (strict, the product rounded
//       once); an unmatched query reports index -1 and d2 = +inf;
//   N4. P = 0: every index -1, every d2 +inf; Q = 0: empty outputs; neither makes a device call;
//   N5. non-finite coordinates are refused, and a max_distance whose square is not a normal number;
//   N6. n, sum d2 and sum sqrt(d2) over the matched queries are added in an order the launch geometry alone fixes: a
//       tree per block, the block partials by one block, again a tree.  No floating-point atomics.
//
// Launches per call: box (targets: finite flag and bounding box), finite (queries), [box_final]; then histogram,
// [scan], scatter, rings, far, [sums, sums_final].  The grid is dense and bounded (sc_nearest.h: plan, cells, the
// stop rule and its proof).  Every launch reads what an earlier launch wrote or writes its own query's words; the
// only traffic between blocks inside a launch is integer atomics (the histogram, the cursors, the far list's
// length, the confusion counts), and nothing depends on their order.  Stand-alone unit: nothing shared with the engine;
// N1 (dist2), the finite launch and the host's judge of non-finite coordinates are sc_points.h, shared with dbscan.hip.
//
// sc_knn (rules K1-K6 in include/spacecarve.h) is the same search for the k nearest: the same launches up
// to the scatter on a grid planned for fewer, fuller cells, then knn_rings and knn_far, one wavefront per query.
//
// sc_radius (rules R1-R7 in include/spacecarve.h) returns ALL targets within a radius, nearest first, in
// CSR form: the same launches up to the scatter on a grid whose cells are at least the radius wide, then radius_count,
// a scan of the row lengths, a wait for their sum, radius_fill (rows sorted in LDS) and radius_long (longer rows,
// sorted in place in global memory), one wavefront per query.

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "sc_nearest.h"  // brings sc_points.h
#include "sc_unit.h"

namespace {

constexpr int kB = 256;
constexpr int kPartials = 256;     // blocks of the box and the sums launches: one final block takes a partial per thread
constexpr int kFarBlocks = 2048;   // blocks of the far pass: 4 wavefronts each, grid-stride over the far list
constexpr int kLdsTable = 1024;    // confusion counts with L * L up to this are gathered per block in LDS (L <= 32)
constexpr int kMaxLabels = 4096;

thread_local UnitError g_err;

// header of the work buffer
struct Header {
    unsigned int bad_targets, bad_queries, bad_labels, nfar;
    double box[6];   // lo x y z, hi x y z
    double sums[3];  // n, sum d2, sum sqrt(d2)
    unsigned int longest, nlong;  // sc_radius: the longest row, the rows on the long list
};

// ---- box: whether every target coordinate is finite, and the targets' bounding box --------------------------------
// One partial per block (6 doubles: lo, hi); min and max do not depend on any order.  Also the judge of device points.
__global__ __launch_bounds__(kB) void nearest_box_kernel(const double *__restrict__ pts, int P, unsigned int *flag, double *__restrict__ partial) {
    __shared__ double sh[6][kB];
    __shared__ int sbad;
    if (threadIdx.x == 0) sbad = 0;
    __syncthreads();
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < P; i += (int64_t)gridDim.x * kB)
        for (int a = 0; a < 3; ++a) {
            const double v = pts[3 * (size_t)i + a];
            if (!(fabs(v) <= DBL_MAX)) bad = 1;
            lo[a] = fmin(lo[a], v);
            hi[a] = fmax(hi[a], v);
        }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&sbad, 1);
    for (int a = 0; a < 3; ++a) {
        sh[a][threadIdx.x] = lo[a];
        sh[3 + a][threadIdx.x] = hi[a];
    }
    __syncthreads();
    for (int s = kB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < 3; ++a) {
                sh[a][threadIdx.x] = fmin(sh[a][threadIdx.x], sh[a][threadIdx.x + s]);
                sh[3 + a][threadIdx.x] = fmax(sh[3 + a][threadIdx.x], sh[3 + a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) partial[6 * blockIdx.x + threadIdx.x] = sh[threadIdx.x][0];
    if (threadIdx.x == 0 && sbad) atomicAdd(flag, 1u);
}

// one block: the partials of the launch before (a kernel boundary lies between) to the header's box
__global__ __launch_bounds__(kB) void nearest_box_final_kernel(const double *__restrict__ partial, int nparts, double *__restrict__ box) {
    __shared__ double sh[6][kB];
    const bool have = (int)threadIdx.x < nparts;
    for (int a = 0; a < 3; ++a) {
        sh[a][threadIdx.x] = have ? partial[6 * threadIdx.x + a] : HUGE_VAL;
        sh[3 + a][threadIdx.x] = have ? partial[6 * threadIdx.x + 3 + a] : -HUGE_VAL;
    }
    __syncthreads();
    for (int s = kB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < 3; ++a) {
                sh[a][threadIdx.x] = fmin(sh[a][threadIdx.x], sh[a][threadIdx.x + s]);
                sh[3 + a][threadIdx.x] = fmax(sh[3 + a][threadIdx.x], sh[3 + a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) box[threadIdx.x] = sh[threadIdx.x][0];
}

// ---- counting sort of the targets by cell --------------------------------------------------------------------------
__device__ __forceinline__ int cell_index(const nn::Grid &g, double x, double y, double z) {
    const int cx = nn::cell_of(x, g.lo[0], g.h, g.n[0]), cy = nn::cell_of(y, g.lo[1], g.h, g.n[1]), cz = nn::cell_of(z, g.lo[2], g.h, g.n[2]);
    return (cz * g.n[1] + cy) * g.n[0] + cx;  // below kMaxCells
}

__global__ __launch_bounds__(kB) void nearest_hist_kernel(const double *__restrict__ pts, int P, nn::Grid g, uint32_t *__restrict__ count) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;  // unsigned: P may be just below 2^31
    if (i >= (uint32_t)P) return;
    atomicAdd(&count[cell_index(g, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2])], 1u);
}

// cursor = a copy of start; afterwards cursor[c] == start[c + 1].  The order inside a cell is whatever the atomics
// give; no result depends on it (N2 decides by the ORIGINAL index, carried in sidx).
__global__ __launch_bounds__(kB) void nearest_scatter_kernel(const double *__restrict__ pts, int P, nn::Grid g, uint32_t *__restrict__ cursor,
                                                             double *__restrict__ spts, int *__restrict__ sidx) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;  // unsigned: P may be just below 2^31
    if (i >= (uint32_t)P) return;
    const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    const uint32_t t = atomicAdd(&cursor[cell_index(g, x, y, z)], 1u);  // below P: the cell's count is what the histogram saw
    spts[3 * (size_t)t] = x;
    spts[3 * (size_t)t + 1] = y;
    spts[3 * (size_t)t + 2] = z;
    sidx[t] = (int)i;
}

// ---- rings: one thread per query -------------------------------------------------------------------------------------
// A settled query writes its own two words; an unsettled one appends its number to the far list (capacity Q: it cannot
// overflow) and writes nothing.  nfar is only added to here and only read by the next launch.
__global__ __launch_bounds__(kB) void nearest_rings_kernel(const double *__restrict__ qs, int Q, nn::Grid g, const uint32_t *__restrict__ start,
                                                           const double *__restrict__ spts, const int *__restrict__ sidx,
                                                           int32_t *__restrict__ index, double *__restrict__ d2, int *__restrict__ far,
                                                           unsigned int *nfar) {
    const uint32_t q = blockIdx.x * kB + threadIdx.x;  // unsigned: Q may be just below 2^31
    if (q >= (uint32_t)Q) return;
    nn::Best best;
    if (nn::ring_search(g, start, spts, sidx, qs[3 * (size_t)q], qs[3 * (size_t)q + 1], qs[3 * (size_t)q + 2], best)) {
        const bool matched = best.d2 < g.md2;  // N3; false as well when nothing was found (d2 = +inf)
        index[q] = matched ? best.idx : -1;
        d2[q] = matched ? best.d2 : HUGE_VAL;
    } else {
        far[atomicAdd(nfar, 1u)] = (int)q;
    }
}

// ---- far: one wavefront per query of the far list, all P targets in their original order ----------------------------
// Costs O(P) per query whatever the data are.  A lane sees its targets in rising index, so `<` keeps the smallest
// index of its own ties; across lanes the pair (d2, index) is reduced lexicographically (N2).
__global__ __launch_bounds__(kB) void nearest_far_kernel(const double *__restrict__ qs, const double *__restrict__ pts, int P, double md2,
                                                         const int *__restrict__ far, const unsigned int *__restrict__ nfar,
                                                         int32_t *__restrict__ index, double *__restrict__ d2) {
    const int lane = (int)(threadIdx.x & 63);
    const unsigned int n = *nfar, waves = gridDim.x * (kB / 64);
    for (unsigned int w = blockIdx.x * (kB / 64) + (threadIdx.x >> 6); w < n; w += waves) {
        const int q = far[w];
        const double qx = qs[3 * (size_t)q], qy = qs[3 * (size_t)q + 1], qz = qs[3 * (size_t)q + 2];
        nn::Best best;
        best.d2 = HUGE_VAL;
        best.idx = 0x7fffffff;
        for (int t = lane; t < P; t += 64) {
            const double d = nn::dist2(qx, qy, qz, pts[3 * (size_t)t], pts[3 * (size_t)t + 1], pts[3 * (size_t)t + 2]);
            if (d < best.d2) {
                best.d2 = d;
                best.idx = t;
            }
        }
        for (int s = 32; s > 0; s >>= 1) best.take(__shfl_xor(best.d2, s, 64), __shfl_xor(best.idx, s, 64));
        if (lane == 0) {
            const bool matched = best.d2 < md2;
            index[q] = matched ? best.idx : -1;
            d2[q] = matched ? best.d2 : HUGE_VAL;
        }
    }
}

// ---- the k nearest: one wavefront per query --------------------------------------------------------------
// The list of a query -- up to k keys (d2, index) in rising order, sc_nearest.h's KList -- lives in LDS, private to its
// wavefront: k doubles and k ints of the block's dynamic LDS (12 k bytes per wavefront, 24 KiB per block at SC_KNN_MAX).
// Lanes exchange list entries through LDS only; lds_order() stands between every write of one lane and the read of
// another: a wavefront-scope fence, which keeps the compiler from moving a lane's accesses across it (the hardware
// runs a wavefront's LDS instructions in order), and the wavefront barrier.  Blocks and wavefronts never wait on one
// another: there is no __syncthreads() in these kernels, so a wavefront without a query simply leaves.
__device__ __forceinline__ void lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

struct WaveList {
    double *ld;     // LDS, [k]
    int *li;        // LDS, [k]
    int k, n, lane; // n: keys held, the same in every lane
    double kd;      // the k-th key once n == k, the same in every lane
    int ki;
    double md2;

    // Every lane brings one key or none (`have`).  Keys not below md2 (K3) or not below the k-th of a full list are
    // dropped by comparison; the survivors, found by ballot, are inserted one after the other, each tested again
    // against the k-th as it stands by then.  An insertion walks the list from its top in pieces of 64 places: a piece
    // is read, its keys above the new one are written one place up (the one pushed past place k - 1 is dropped), and
    // the first piece that holds a key below the new one gives its place.  At most ceil(k / 64) pieces per insertion.
    __device__ __forceinline__ void offer(double d, int i, bool have) {
        unsigned long long m = __ballot(have && d < md2 && (n < k || nn::key_less(d, i, kd, ki)));
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const double bd = __shfl(d, src, 64);
            const int bi = __shfl(i, src, 64);
            if (n == k && !nn::key_less(bd, bi, kd, ki)) continue;
            int pos = 0;
            for (int c = (n - 1) >> 6; c >= 0; --c) {  // n = 0: no piece
                const int j = (c << 6) + lane;
                const bool in = j < n;
                const double ed = in ? ld[j] : 0.0;
                const int ei = in ? li[j] : 0;
                const bool below = in && nn::key_less(ed, ei, bd, bi);  // a prefix of the piece: the list is sorted
                lds_order();
                if (in && !below && j + 1 < k) {
                    ld[j + 1] = ed;
                    li[j + 1] = ei;
                }
                lds_order();
                const int cnt = __popcll(__ballot(below));
                if (cnt) {
                    pos = (c << 6) + cnt;
                    break;
                }
            }
            if (lane == 0) {  // pos < k: the new key is below the k-th of a full list, or the list has room
                ld[pos] = bd;
                li[pos] = bi;
            }
            lds_order();
            if (n < k) n = __builtin_amdgcn_readfirstlane(n + 1);
            if (n == k) {
                kd = ld[k - 1];
                ki = li[k - 1];
            }
        }
    }

    // row q of the outputs: the keys held, then K4's unused places
    __device__ __forceinline__ void write_row(int32_t *__restrict__ index, double *__restrict__ d2, uint32_t q) const {
        for (int j = lane; j < k; j += 64) {
            index[(size_t)q * k + j] = j < n ? li[j] : -1;
            d2[(size_t)q * k + j] = j < n ? ld[j] : HUGE_VAL;
        }
    }
};

__device__ __forceinline__ WaveList wave_list(int k, double md2) {
    extern __shared__ double knn_lds[];  // [kB / 64][k] doubles, then as many ints
    const int wave = (int)(threadIdx.x >> 6);
    WaveList l;
    l.ld = knn_lds + (size_t)wave * k;
    l.li = reinterpret_cast<int *>(knn_lds + (size_t)(kB / 64) * k) + (size_t)wave * k;
    l.k = k;
    l.n = 0;
    l.lane = (int)(threadIdx.x & 63);
    l.kd = HUGE_VAL;
    l.ki = 0x7fffffff;
    l.md2 = md2;
    return l;
}

// rings: the walk of sc_nearest.h's knn_ring_search with the 64 lanes on 64 sorted slots at a time.  A settled query
// writes its own row; an unsettled one appends its number to the far list (capacity Q) and writes nothing.  nfar is
// only added to here and only read by the next launch.  The grid is not capped: ceil(Q / 4) blocks, below 2^29.
__global__ __launch_bounds__(kB) void knn_rings_kernel(const double *__restrict__ qs, int Q, nn::Grid g, const uint32_t *__restrict__ start,
                                                       const double *__restrict__ spts, const int *__restrict__ sidx, int k,
                                                       int32_t *__restrict__ index, double *__restrict__ d2, int *__restrict__ far,
                                                       unsigned int *nfar) {
    const uint32_t q = blockIdx.x * (kB / 64) + (threadIdx.x >> 6);  // the same in every lane of a wavefront
    if (q >= (uint32_t)Q) return;
    WaveList list = wave_list(k, g.md2);
    const double qx = qs[3 * (size_t)q], qy = qs[3 * (size_t)q + 1], qz = qs[3 * (size_t)q + 2];
    const int cx = nn::cell_of(qx, g.lo[0], g.h, g.n[0]), cy = nn::cell_of(qy, g.lo[1], g.h, g.n[1]), cz = nn::cell_of(qz, g.lo[2], g.h, g.n[2]);
    const int last = nn::last_ring(g, cx, cy, cz);
    bool settled = false;
    for (int r = 0; r <= nn::kNearRings && !settled; ++r) {
        nn::for_ring_runs(g, cx, cy, cz, r, start, [&](uint32_t t0, uint32_t t1) {
            for (uint32_t b = t0; b < t1; b += 64) {  // t1 <= P < 2^31: b + 64 does not wrap
                const uint32_t t = b + list.lane;
                const bool have = t < t1;
                const size_t s = have ? t : t0;
                list.offer(nn::dist2(qx, qy, qz, spts[3 * s], spts[3 * s + 1], spts[3 * s + 2]), sidx[s], have);
            }
        });
        settled = nn::knn_settled(g, r, last, list.n == list.k, list.kd);
    }
    if (settled)
        list.write_row(index, d2, q);
    else if (list.lane == 0)
        far[atomicAdd(nfar, 1u)] = (int)q;
}

// far: one wavefront per query of the far list, the list started empty, all P targets in their original order.
// O(P) per query whatever the data are.
__global__ __launch_bounds__(kB) void knn_far_kernel(const double *__restrict__ qs, const double *__restrict__ pts, int P, double md2, int k,
                                                     const int *__restrict__ far, const unsigned int *__restrict__ nfar,
                                                     int32_t *__restrict__ index, double *__restrict__ d2) {
    const unsigned int n = *nfar, waves = gridDim.x * (kB / 64);
    for (unsigned int w = blockIdx.x * (kB / 64) + (threadIdx.x >> 6); w < n; w += waves) {
        const int q = far[w];
        const double qx = qs[3 * (size_t)q], qy = qs[3 * (size_t)q + 1], qz = qs[3 * (size_t)q + 2];
        WaveList list = wave_list(k, md2);
        for (uint32_t b = 0; b < (uint32_t)P; b += 64) {
            const uint32_t t = b + list.lane;
            const bool have = t < (uint32_t)P;
            const size_t s = have ? t : 0;
            list.offer(nn::dist2(qx, qy, qz, pts[3 * s], pts[3 * s + 1], pts[3 * s + 2]), (int)s, have);
        }
        list.write_row(index, d2, (uint32_t)q);
        lds_order();  // the next query's list takes the same places
    }
}

// ---- all targets within a radius: one wavefront per query ---------------------------------------------------
// The walk of sc_nearest.h's radius_search with the 64 lanes on 64 sorted slots at a time: f(slot, d2, in) is called by
// the whole wavefront for every piece of every run, `in` being R2's predicate of the lane's slot.  The rings go on
// until radius_settled: at most last_ring + 1 of them.
template <class F>
__device__ __forceinline__ void radius_walk(const nn::Grid &g, const uint32_t *__restrict__ start, const double *__restrict__ spts,
                                            double qx, double qy, double qz, int lane, F &&f) {
    const int cx = nn::cell_of(qx, g.lo[0], g.h, g.n[0]), cy = nn::cell_of(qy, g.lo[1], g.h, g.n[1]), cz = nn::cell_of(qz, g.lo[2], g.h, g.n[2]);
    const int last = nn::last_ring(g, cx, cy, cz);
    for (int r = 0;; ++r) {
        nn::for_ring_runs(g, cx, cy, cz, r, start, [&](uint32_t t0, uint32_t t1) {
            for (uint32_t b = t0; b < t1; b += 64) {  // t1 <= P < 2^31: b + 64 does not wrap
                const uint32_t t = b + lane;
                const bool have = t < t1;
                const size_t s = have ? t : t0;
                const double d = nn::dist2(qx, qy, qz, spts[3 * s], spts[3 * s + 1], spts[3 * s + 2]);
                f(s, d, have && d < g.md2);
            }
        });
        if (nn::radius_settled(g, r, last)) return;
    }
}

// count: the length of every row.  Lane 0 writes it twice -- counts[q], and as a 64-bit number offsets[q], which the
// scan behind this launch turns into the row's first place -- and raises the header's longest row by an integer
// atomicMax: nothing depends on the order.  The atomic is skipped when a relaxed load already shows a row as long: the
// word only grows, so a stale value costs an atomic and changes nothing (one atomic per query on one word took 2.3 of
// the launch's 2.8 ms on the 226 689-point cloud of DESIGN.md 19).
__global__ __launch_bounds__(kB) void radius_count_kernel(const double *__restrict__ qs, int Q, nn::Grid g, const uint32_t *__restrict__ start,
                                                          const double *__restrict__ spts, int32_t *__restrict__ counts,
                                                          int64_t *__restrict__ offsets, unsigned int *longest) {
    const uint32_t q = blockIdx.x * (kB / 64) + (threadIdx.x >> 6);  // the same in every lane of a wavefront
    if (q >= (uint32_t)Q) return;
    const int lane = (int)(threadIdx.x & 63);
    int n = 0;  // at most P < 2^31
    radius_walk(g, start, spts, qs[3 * (size_t)q], qs[3 * (size_t)q + 1], qs[3 * (size_t)q + 2], lane,
                [&](size_t, double, bool in) { n += __popcll(__ballot(in)); });
    if (lane == 0) {
        counts[q] = n;
        offsets[q] = n;
        if ((unsigned int)n > __hip_atomic_load(longest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(longest, (unsigned int)n);
    }
}

// What stands between a lane's store to global memory and another lane's load of that word in radius_long_kernel: an
// agent-scope fence -- the stores are drained to the L2 and this compute unit's vector L1 is invalidated, so the load
// that follows cannot be served from a line fetched before the store -- and the wavefront barrier, which keeps the
// compiler from moving a lane's accesses across (the wavefront-scope fence behind it does the same for what follows and
// emits nothing).  lds_order()'s wavefront-scope fences emit no instruction: enough for LDS, which a wavefront accesses
// in order, not for loads and stores that return out of order through a cache.
__device__ __forceinline__ void global_order() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// fill: the same enumeration and the same predicate as count; the row's length n and first place are known.  A
// survivor's place is its rank among the ballot's set bits plus a running base.  Rows of up to lds_row keys (the
// places this launch gave each wavefront: min(SC_RADIUS_LDS_ROW, the longest row rounded up to a power of two)) are
// gathered in the wavefront's private piece of LDS, sorted there and written once, coalesced.  Longer rows go to
// their places in global memory in visiting order and onto the long list (capacity Q; only added to here, only read
// by the next launch).  `pos < n` holds by construction; the test keeps every write inside the row all the same.
__global__ __launch_bounds__(kB) void radius_fill_kernel(const double *__restrict__ qs, int Q, nn::Grid g, const uint32_t *__restrict__ start,
                                                         const double *__restrict__ spts, const int *__restrict__ sidx,
                                                         const int64_t *__restrict__ offsets, int lds_row, int32_t *__restrict__ index,
                                                         double *__restrict__ d2, int *__restrict__ longlist, unsigned int *nlong) {
    extern __shared__ double radius_lds[];  // [kB / 64][lds_row] doubles, then as many ints
    const uint32_t q = blockIdx.x * (kB / 64) + (threadIdx.x >> 6);
    if (q >= (uint32_t)Q) return;
    const int64_t first = offsets[q], len = offsets[q + 1] - first;
    if (len <= 0) return;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int n = (int)len;  // a row holds at most P < 2^31 keys
    const bool in_lds = n <= lds_row;
    double *kd = in_lds ? radius_lds + (size_t)wave * lds_row : d2 + first;
    int *ki = in_lds ? reinterpret_cast<int *>(radius_lds + (size_t)(kB / 64) * lds_row) + (size_t)wave * lds_row : index + first;
    int base = 0;
    radius_walk(g, start, spts, qs[3 * (size_t)q], qs[3 * (size_t)q + 1], qs[3 * (size_t)q + 2], lane, [&](size_t s, double d, bool in) {
        const unsigned long long m = __ballot(in);
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        if (in && pos < n) {
            kd[pos] = d;
            ki[pos] = sidx[s];
        }
        base += __popcll(m);
    });
    if (!in_lds) {
        if (lane == 0) longlist[atomicAdd(nlong, 1u)] = (int)q;
        return;
    }
    nn::sort_row(kd, ki, n, lane, 64, [] { lds_order(); });
    for (int j = lane; j < n; j += 64) {
        index[first + j] = ki[j];
        d2[first + j] = kd[j];
    }
}

// long: one wavefront per row of the long list, grid-stride; the same network over the row in place in global memory.
__global__ __launch_bounds__(kB) void radius_long_kernel(const int64_t *__restrict__ offsets, const int *__restrict__ longlist,
                                                         const unsigned int *__restrict__ nlong, int32_t *index, double *d2) {
    const int lane = (int)(threadIdx.x & 63);
    const unsigned int rows = *nlong, waves = gridDim.x * (kB / 64);
    for (unsigned int w = blockIdx.x * (kB / 64) + (threadIdx.x >> 6); w < rows; w += waves) {
        const int q = longlist[w];
        const int64_t first = offsets[q];
        nn::sort_row(d2 + first, index + first, (int)(offsets[q + 1] - first), lane, 64, [] { global_order(); });
    }
}

// ---- sums (N6) -----------------------------------------------------------------------------------------------------------
// A thread adds its queries in rising index, a block adds its threads by a tree, and block b leaves its three partials
// at partial[3 b]: the order is a function of Q, kB and the block count.
__device__ __forceinline__ void block_tree3(double (*sh)[kB], double a, double b, double c) {
    sh[0][threadIdx.x] = a;
    sh[1][threadIdx.x] = b;
    sh[2][threadIdx.x] = c;
    __syncthreads();
    for (int s = kB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < 3; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + s];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kB) void nearest_sums_kernel(const double *__restrict__ d2, int Q, double *__restrict__ partial) {
    __shared__ double sh[3][kB];
    double n = 0.0, s2 = 0.0, s1 = 0.0;  // n is a whole number below 2^31: exact
    for (int64_t q = (int64_t)blockIdx.x * kB + threadIdx.x; q < Q; q += (int64_t)gridDim.x * kB) {
        const double d = d2[q];
        if (d < HUGE_VAL) {
            n += 1.0;
            s2 += d;
            s1 += sqrt(d);
        }
    }
    block_tree3(sh, n, s2, s1);
    if (threadIdx.x < 3) partial[3 * blockIdx.x + threadIdx.x] = sh[threadIdx.x][0];
}

__global__ __launch_bounds__(kB) void nearest_sums_final_kernel(const double *__restrict__ partial, int nparts, double *__restrict__ sums) {
    __shared__ double sh[3][kB];
    const bool have = (int)threadIdx.x < nparts;
    block_tree3(sh, have ? partial[3 * threadIdx.x] : 0.0, have ? partial[3 * threadIdx.x + 1] : 0.0, have ? partial[3 * threadIdx.x + 2] : 0.0);
    if (threadIdx.x < 3) sums[threadIdx.x] = sh[threadIdx.x][0];
}

// ---- confusion counts ------------------------------------------------------------------------------------------------------
// labels: the judge of device arrays.  An index outside -1..P-1 or a label outside 0..L-1 raises the flag.
__global__ __launch_bounds__(kB) void nearest_labels_kernel(const int32_t *__restrict__ index, const int32_t *__restrict__ qlab, int Q,
                                                            const int32_t *__restrict__ tlab, int P, int L, unsigned int *flag) {
    int bad = 0;
    for (int64_t k = (int64_t)blockIdx.x * kB + threadIdx.x; k < Q; k += (int64_t)gridDim.x * kB)
        if (index[k] < -1 || index[k] >= P || qlab[k] < 0 || qlab[k] >= L) bad = 1;
    for (int64_t k = (int64_t)blockIdx.x * kB + threadIdx.x; k < P; k += (int64_t)gridDim.x * kB)
        if (tlab[k] < 0 || tlab[k] >= L) bad = 1;
    if (bad) atomicOr(flag, 1u);
}

// counts[a L + b] += 1 for a query of label a whose nearest target has label b.  Every access is checked again here:
// a refused call (the labels launch) still reads and writes inside its arrays.  kLds: L * L <= kLdsTable, the block
// counts in LDS (at most 2^31 per block: 32 bits) and adds its non-zero cells once.
template <bool kLds>
__global__ __launch_bounds__(kB) void nearest_confusion_kernel(const int32_t *__restrict__ index, const int32_t *__restrict__ qlab, int Q,
                                                               const int32_t *__restrict__ tlab, int P, int L, unsigned long long *counts) {
    __shared__ unsigned int tab[kLds ? kLdsTable : 1];
    if (kLds) {
        for (int k = (int)threadIdx.x; k < L * L; k += kB) tab[k] = 0u;
        __syncthreads();
    }
    for (int64_t q = (int64_t)blockIdx.x * kB + threadIdx.x; q < Q; q += (int64_t)gridDim.x * kB) {
        const int t = index[q], a = qlab[q];
        if (t < 0 || t >= P || a < 0 || a >= L) continue;
        const int b = tlab[t];
        if (b < 0 || b >= L) continue;
        if (kLds)
            atomicAdd(&tab[a * L + b], 1u);
        else
            atomicAdd(&counts[(size_t)a * L + b], 1ull);
    }
    if (kLds) {
        __syncthreads();
        for (int k = (int)threadIdx.x; k < L * L; k += kB)
            if (tab[k]) atomicAdd(&counts[k], (unsigned long long)tab[k]);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// Work buffers are kept per device: the slot protocol of sc_unit.h.  Both entries share the slot.
WorkSlot g_slots[kUnitDevices];

std::atomic<int> g_knn_aim{0};  // sc_knn_set_aim: targets per cell sc_knn's grid aims at; 0: nn::knn_aim(k)

uint32_t pow2ceil(uint32_t n) {  // the least power of two >= n, n <= 2^31
    uint32_t m = 1;
    while (m < n) m <<= 1;
    return m;
}

}  // namespace

extern "C" {

const char *sc_nearest_last_error(void) { return g_err.msg; }

int sc_nearest(const double *queries, int queries_on_device, int64_t Q, const double *targets, int targets_on_device, int64_t P,
               double max_distance, int device, int32_t *index_out, double *d2_out, int out_on_device, double *sums_out,
               void *hip_stream) {
    // every argument is judged before the first device call
    if (Q < 0 || Q >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "Q must be 0 .. 2^31 - 1");
    if (P < 0 || P >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "P must be 0 .. 2^31 - 1");
    if ((Q > 0 && !queries) || (P > 0 && !targets)) return g_err.fail(SC_ERR_INVALID, "null argument (queries, targets)");
    if (!index_out && !d2_out && !sums_out) return g_err.fail(SC_ERR_INVALID, "null argument (one of index_out, d2_out, sums_out is needed)");
    if (!std::isfinite(max_distance)) return g_err.fail(SC_ERR_INVALID, "max_distance must be finite (<= 0: unbounded)");
    if (max_distance > 0.0 && (!(max_distance * max_distance >= DBL_MIN) || !std::isfinite(max_distance * max_distance)))
        return g_err.fail(SC_ERR_INVALID, "max_distance * max_distance must be a normal number (max_distance out of range)");
    if (device < 0 || device >= kUnitDevices) return g_err.fail(SC_ERR_INVALID, "device ordinal out of range");
    if (P == 0 && Q > 0 && out_on_device && (index_out || d2_out))
        return g_err.fail(SC_ERR_INVALID, "P == 0 makes no device call: device outputs cannot be filled");
    if (!queries_on_device && first_non_finite(g_err, queries, Q, "query") != SC_OK) return SC_ERR_INVALID;
    if (!targets_on_device && first_non_finite(g_err, targets, P, "target") != SC_OK) return SC_ERR_INVALID;
    if (sums_out) sums_out[0] = sums_out[1] = sums_out[2] = 0.0;
    if (Q == 0) return SC_OK;
    if (P == 0) {  // N4
        for (int64_t q = 0; q < Q; ++q) {
            if (index_out) index_out[q] = -1;
            if (d2_out) d2_out[q] = HUGE_VAL;
        }
        return SC_OK;
    }

    const int nq = (int)Q, np = (int)P;
    const int64_t cap = nn::cell_cap(P);
    const uint32_t qblocks = (uint32_t)((Q + kB - 1) / kB), pblocks = (uint32_t)((P + kB - 1) / kB);
    const int box_parts = (int)std::min<uint32_t>(pblocks, kPartials), sum_parts = (int)std::min<uint32_t>(qblocks, kPartials);

    int rc = SC_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    UnitCall call(g_err, g_slots, device, stream, rc);
    size_t tmp = 0;
    Header hh;
    nn::Grid g;

    // layout of the work buffer
    Layout lay;
    const size_t o_hdr = lay.take(sizeof(Header)), o_part = lay.take((size_t)kPartials * 6 * 8);
    const size_t o_count = lay.take(((size_t)cap + 1) * 4), o_start = lay.take(((size_t)cap + 1) * 4), o_cursor = lay.take(((size_t)cap + 1) * 4);
    const size_t o_spts = lay.take((size_t)P * 24), o_sidx = lay.take((size_t)P * 4), o_far = lay.take((size_t)Q * 4);
    const size_t o_qs = lay.take(queries_on_device ? 0 : (size_t)Q * 24), o_ts = lay.take(targets_on_device ? 0 : (size_t)P * 24);
    const size_t o_idx = lay.take(index_out && out_on_device ? 0 : (size_t)Q * 4), o_d2 = lay.take(d2_out && out_on_device ? 0 : (size_t)Q * 8);
    size_t o_tmp = 0;  // the scan's temporary storage: the last buffer, sized below

    if ((rc = call.enter()) != SC_OK) goto done;
    // the scan's temporary storage for the largest table (a size query: no device work)
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)(cap + 1), stream));
    o_tmp = lay.take(tmp);
    if ((rc = call.grow(lay.total)) != SC_OK) goto done;
    {
        char *const w = call.sl.base;
        Header *hdr = reinterpret_cast<Header *>(w + o_hdr);
        double *partial = reinterpret_cast<double *>(w + o_part);
        uint32_t *count = reinterpret_cast<uint32_t *>(w + o_count), *start = reinterpret_cast<uint32_t *>(w + o_start),
                 *cursor = reinterpret_cast<uint32_t *>(w + o_cursor);
        double *spts = reinterpret_cast<double *>(w + o_spts);
        int *sidx = reinterpret_cast<int *>(w + o_sidx), *far = reinterpret_cast<int *>(w + o_far);
        const double *qs_d = queries_on_device ? queries : reinterpret_cast<const double *>(w + o_qs);
        const double *ts_d = targets_on_device ? targets : reinterpret_cast<const double *>(w + o_ts);
        int32_t *idx_d = index_out && out_on_device ? index_out : reinterpret_cast<int32_t *>(w + o_idx);
        double *d2_d = d2_out && out_on_device ? d2_out : reinterpret_cast<double *>(w + o_d2);
        void *tmp_d = w + o_tmp;

        UNIT_TRY(call.sl.wait(stream));
        if (!queries_on_device) UNIT_TRY(hipMemcpyAsync(w + o_qs, queries, (size_t)Q * 24, hipMemcpyHostToDevice, stream));
        if (!targets_on_device) UNIT_TRY(hipMemcpyAsync(w + o_ts, targets, (size_t)P * 24, hipMemcpyHostToDevice, stream));
        UNIT_TRY(hipMemsetAsync(hdr, 0, sizeof(Header), stream));
        hipLaunchKernelGGL(nearest_box_kernel, dim3(box_parts), dim3(kB), 0, stream, ts_d, np, &hdr->bad_targets, partial);
        hipLaunchKernelGGL(nearest_box_final_kernel, dim3(1), dim3(kB), 0, stream, partial, box_parts, hdr->box);
        launch_points_finite(stream, qs_d, Q, &hdr->bad_queries);
        UNIT_TRY(hipGetLastError());
        UNIT_TRY(hipMemcpyAsync(&hh, hdr, sizeof(Header), hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        UNIT_TRY(hipStreamSynchronize(stream));  // the call's one mid-way wait
        if (hh.bad_queries != 0u || hh.bad_targets != 0u) {  // device points: the first kernels are the judge
            rc = g_err.fail(SC_ERR_INVALID, hh.bad_queries ? "non-finite coordinate in the device queries" : "non-finite coordinate in the device targets");
            goto done;
        }
        nn::plan_grid(hh.box, hh.box + 3, P, max_distance, g);
        const int ncell = g.n[0] * g.n[1] * g.n[2];  // <= cap

        UNIT_TRY(hipMemsetAsync(count, 0, ((size_t)ncell + 1) * 4, stream));
        hipLaunchKernelGGL(nearest_hist_kernel, dim3(pblocks), dim3(kB), 0, stream, ts_d, np, g, count);
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(tmp_d, tmp, count, start, ncell + 1, stream));
        UNIT_TRY(hipMemcpyAsync(cursor, start, (size_t)ncell * 4, hipMemcpyDeviceToDevice, stream));
        hipLaunchKernelGGL(nearest_scatter_kernel, dim3(pblocks), dim3(kB), 0, stream, ts_d, np, g, cursor, spts, sidx);
        hipLaunchKernelGGL(nearest_rings_kernel, dim3(qblocks), dim3(kB), 0, stream, qs_d, nq, g, start, spts, sidx, idx_d, d2_d, far, &hdr->nfar);
        hipLaunchKernelGGL(nearest_far_kernel, dim3(std::min<uint32_t>((uint32_t)((Q + 3) / 4), kFarBlocks)), dim3(kB), 0, stream, qs_d, ts_d, np,
                           g.md2, far, &hdr->nfar, idx_d, d2_d);
        if (sums_out) {
            hipLaunchKernelGGL(nearest_sums_kernel, dim3(sum_parts), dim3(kB), 0, stream, d2_d, nq, partial);
            hipLaunchKernelGGL(nearest_sums_final_kernel, dim3(1), dim3(kB), 0, stream, partial, sum_parts, hdr->sums);
        }
        UNIT_TRY(hipGetLastError());
        if (index_out && !out_on_device) UNIT_TRY(hipMemcpyAsync(index_out, idx_d, (size_t)Q * 4, hipMemcpyDeviceToHost, stream));
        if (d2_out && !out_on_device) UNIT_TRY(hipMemcpyAsync(d2_out, d2_d, (size_t)Q * 8, hipMemcpyDeviceToHost, stream));
        if (sums_out) UNIT_TRY(hipMemcpyAsync(hh.sums, hdr->sums, sizeof hh.sums, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        if (sums_out || ((index_out || d2_out) && !out_on_device)) {
            UNIT_TRY(hipStreamSynchronize(stream));
            if (sums_out)
                for (int k = 0; k < 3; ++k) sums_out[k] = hh.sums[k];
        }
    }

done:
    return rc;
}

void sc_knn_set_aim(int aim) { g_knn_aim.store(aim > 0 ? aim : 0); }

int sc_knn(const double *queries, int queries_on_device, int64_t Q, const double *targets, int targets_on_device, int64_t P, int k,
           double max_distance, int device, int32_t *index_out, double *d2_out, int out_on_device, int64_t *far_out, void *hip_stream) {
    // every argument is judged before the first device call
    if (Q < 0 || Q >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "Q must be 0 .. 2^31 - 1");
    if (P < 0 || P >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "P must be 0 .. 2^31 - 1");
    if (k < 1 || k > SC_KNN_MAX) return g_err.fail(SC_ERR_INVALID, "k must be 1 .. SC_KNN_MAX (512)");
    if (Q * k >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "Q * k must be below 2^31");
    if ((Q > 0 && !queries) || (P > 0 && !targets)) return g_err.fail(SC_ERR_INVALID, "null argument (queries, targets)");
    if (!index_out || !d2_out) return g_err.fail(SC_ERR_INVALID, "null argument (index_out, d2_out)");
    if (!std::isfinite(max_distance)) return g_err.fail(SC_ERR_INVALID, "max_distance must be finite (<= 0: unbounded)");
    if (max_distance > 0.0 && (!(max_distance * max_distance >= DBL_MIN) || !std::isfinite(max_distance * max_distance)))
        return g_err.fail(SC_ERR_INVALID, "max_distance * max_distance must be a normal number (max_distance out of range)");
    if (device < 0 || device >= kUnitDevices) return g_err.fail(SC_ERR_INVALID, "device ordinal out of range");
    if (P == 0 && Q > 0 && out_on_device) return g_err.fail(SC_ERR_INVALID, "P == 0 makes no device call: device outputs cannot be filled");
    if (!queries_on_device && first_non_finite(g_err, queries, Q, "query") != SC_OK) return SC_ERR_INVALID;
    if (!targets_on_device && first_non_finite(g_err, targets, P, "target") != SC_OK) return SC_ERR_INVALID;
    if (far_out) *far_out = 0;
    if (Q == 0) return SC_OK;
    const int64_t words = Q * k;  // below 2^31
    if (P == 0) {  // K4
        for (int64_t w = 0; w < words; ++w) {
            index_out[w] = -1;
            d2_out[w] = HUGE_VAL;
        }
        return SC_OK;
    }

    const int nq = (int)Q, np = (int)P;
    const int64_t cap = nn::cell_cap(P);
    const uint32_t pblocks = (uint32_t)((P + kB - 1) / kB), qwave_blocks = (uint32_t)((Q + kB / 64 - 1) / (kB / 64));
    const int box_parts = (int)std::min<uint32_t>(pblocks, kPartials);
    const size_t lds = (size_t)(kB / 64) * (size_t)k * 12;  // the lists of a block: at most 24 KiB
    const int set_aim = g_knn_aim.load(), aim = set_aim > 0 ? set_aim : nn::knn_aim(k);

    int rc = SC_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    UnitCall call(g_err, g_slots, device, stream, rc);
    size_t tmp = 0;
    Header hh;
    nn::Grid g;

    // layout of the work buffer: sc_nearest's, with k places per query in the staged outputs
    Layout lay;
    const size_t o_hdr = lay.take(sizeof(Header)), o_part = lay.take((size_t)kPartials * 6 * 8);
    const size_t o_count = lay.take(((size_t)cap + 1) * 4), o_start = lay.take(((size_t)cap + 1) * 4), o_cursor = lay.take(((size_t)cap + 1) * 4);
    const size_t o_spts = lay.take((size_t)P * 24), o_sidx = lay.take((size_t)P * 4), o_far = lay.take((size_t)Q * 4);
    const size_t o_qs = lay.take(queries_on_device ? 0 : (size_t)Q * 24), o_ts = lay.take(targets_on_device ? 0 : (size_t)P * 24);
    const size_t o_idx = lay.take(out_on_device ? 0 : (size_t)words * 4), o_d2 = lay.take(out_on_device ? 0 : (size_t)words * 8);
    size_t o_tmp = 0;  // the scan's temporary storage: the last buffer, sized below

    if ((rc = call.enter()) != SC_OK) goto done;
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)(cap + 1), stream));
    o_tmp = lay.take(tmp);
    if ((rc = call.grow(lay.total)) != SC_OK) goto done;
    {
        char *const w = call.sl.base;
        Header *hdr = reinterpret_cast<Header *>(w + o_hdr);
        double *partial = reinterpret_cast<double *>(w + o_part);
        uint32_t *count = reinterpret_cast<uint32_t *>(w + o_count), *start = reinterpret_cast<uint32_t *>(w + o_start),
                 *cursor = reinterpret_cast<uint32_t *>(w + o_cursor);
        double *spts = reinterpret_cast<double *>(w + o_spts);
        int *sidx = reinterpret_cast<int *>(w + o_sidx), *far = reinterpret_cast<int *>(w + o_far);
        const double *qs_d = queries_on_device ? queries : reinterpret_cast<const double *>(w + o_qs);
        const double *ts_d = targets_on_device ? targets : reinterpret_cast<const double *>(w + o_ts);
        int32_t *idx_d = out_on_device ? index_out : reinterpret_cast<int32_t *>(w + o_idx);
        double *d2_d = out_on_device ? d2_out : reinterpret_cast<double *>(w + o_d2);
        void *tmp_d = w + o_tmp;

        UNIT_TRY(call.sl.wait(stream));
        if (!queries_on_device) UNIT_TRY(hipMemcpyAsync(w + o_qs, queries, (size_t)Q * 24, hipMemcpyHostToDevice, stream));
        if (!targets_on_device) UNIT_TRY(hipMemcpyAsync(w + o_ts, targets, (size_t)P * 24, hipMemcpyHostToDevice, stream));
        UNIT_TRY(hipMemsetAsync(hdr, 0, sizeof(Header), stream));
        hipLaunchKernelGGL(nearest_box_kernel, dim3(box_parts), dim3(kB), 0, stream, ts_d, np, &hdr->bad_targets, partial);
        hipLaunchKernelGGL(nearest_box_final_kernel, dim3(1), dim3(kB), 0, stream, partial, box_parts, hdr->box);
        launch_points_finite(stream, qs_d, Q, &hdr->bad_queries);
        UNIT_TRY(hipGetLastError());
        UNIT_TRY(hipMemcpyAsync(&hh, hdr, sizeof(Header), hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        UNIT_TRY(hipStreamSynchronize(stream));  // the call's one mid-way wait
        if (hh.bad_queries != 0u || hh.bad_targets != 0u) {  // device points: the first kernels are the judge
            rc = g_err.fail(SC_ERR_INVALID, hh.bad_queries ? "non-finite coordinate in the device queries" : "non-finite coordinate in the device targets");
            goto done;
        }
        nn::plan_grid(hh.box, hh.box + 3, std::max<int64_t>(1, P / aim), max_distance, g);  // about `aim` targets per cell
        const int ncell = g.n[0] * g.n[1] * g.n[2];  // <= cell_cap(P / aim) <= cap

        UNIT_TRY(hipMemsetAsync(count, 0, ((size_t)ncell + 1) * 4, stream));
        hipLaunchKernelGGL(nearest_hist_kernel, dim3(pblocks), dim3(kB), 0, stream, ts_d, np, g, count);
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(tmp_d, tmp, count, start, ncell + 1, stream));
        UNIT_TRY(hipMemcpyAsync(cursor, start, (size_t)ncell * 4, hipMemcpyDeviceToDevice, stream));
        hipLaunchKernelGGL(nearest_scatter_kernel, dim3(pblocks), dim3(kB), 0, stream, ts_d, np, g, cursor, spts, sidx);
        hipLaunchKernelGGL(knn_rings_kernel, dim3(qwave_blocks), dim3(kB), lds, stream, qs_d, nq, g, start, spts, sidx, k, idx_d, d2_d, far,
                           &hdr->nfar);
        hipLaunchKernelGGL(knn_far_kernel, dim3(std::min<uint32_t>(qwave_blocks, kFarBlocks)), dim3(kB), lds, stream, qs_d, ts_d, np, g.md2, k, far,
                           &hdr->nfar, idx_d, d2_d);
        UNIT_TRY(hipGetLastError());
        if (!out_on_device) {
            UNIT_TRY(hipMemcpyAsync(index_out, idx_d, (size_t)words * 4, hipMemcpyDeviceToHost, stream));
            UNIT_TRY(hipMemcpyAsync(d2_out, d2_d, (size_t)words * 8, hipMemcpyDeviceToHost, stream));
        }
        if (far_out) UNIT_TRY(hipMemcpyAsync(&hh.nfar, &hdr->nfar, 4, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        if (far_out || !out_on_device) {
            UNIT_TRY(hipStreamSynchronize(stream));
            if (far_out) *far_out = (int64_t)hh.nfar;
        }
    }

done:
    return rc;
}

int sc_radius(const double *queries, int queries_on_device, int64_t Q, const double *targets, int targets_on_device, int64_t P,
              double radius, int device, int32_t *counts_out, int64_t *offsets_out, int32_t *index_out, double *d2_out, int64_t capacity,
              int out_on_device, int64_t *total_out, int64_t *long_out, void *hip_stream) {
    // every argument is judged before the first device call
    if (Q < 0 || Q >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "Q must be 0 .. 2^31 - 1");
    if (P < 0 || P >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "P must be 0 .. 2^31 - 1");
    if ((Q > 0 && !queries) || (P > 0 && !targets) || !total_out) return g_err.fail(SC_ERR_INVALID, "null argument (queries, targets, total_out)");
    if (!index_out != !d2_out) return g_err.fail(SC_ERR_INVALID, "index_out and d2_out are given both or neither");
    if (capacity < 0) return g_err.fail(SC_ERR_INVALID, "capacity must not be negative");
    if (!std::isfinite(radius) || !(radius > 0.0)) return g_err.fail(SC_ERR_INVALID, "radius must be finite and positive");
    if (!(radius * radius >= DBL_MIN) || !std::isfinite(radius * radius))
        return g_err.fail(SC_ERR_INVALID, "radius * radius must be a normal number (radius out of range)");
    if (device < 0 || device >= kUnitDevices) return g_err.fail(SC_ERR_INVALID, "device ordinal out of range");
    if ((Q == 0 || P == 0) && out_on_device && (offsets_out || (Q > 0 && counts_out)))
        return g_err.fail(SC_ERR_INVALID, "Q == 0 or P == 0 makes no device call: device outputs cannot be filled");
    if (!queries_on_device && first_non_finite(g_err, queries, Q, "query") != SC_OK) return SC_ERR_INVALID;
    if (!targets_on_device && first_non_finite(g_err, targets, P, "target") != SC_OK) return SC_ERR_INVALID;
    *total_out = 0;
    if (long_out) *long_out = 0;
    if (Q == 0 || P == 0) {  // R4: empty rows; host outputs (device ones were refused above)
        if (offsets_out)
            for (int64_t q = 0; q <= Q; ++q) offsets_out[q] = 0;
        if (counts_out)
            for (int64_t q = 0; q < Q; ++q) counts_out[q] = 0;
        return SC_OK;
    }

    const int nq = (int)Q, np = (int)P;
    const int64_t cap = nn::cell_cap(P);
    const uint32_t pblocks = (uint32_t)((P + kB - 1) / kB), qwave_blocks = (uint32_t)((Q + kB / 64 - 1) / (kB / 64));
    const int box_parts = (int)std::min<uint32_t>(pblocks, kPartials);
    const bool rows = index_out != nullptr, stage_rows = rows && !out_on_device;

    int rc = SC_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    UnitCall call(g_err, g_slots, device, stream, rc);
    size_t tmp = 0, tmp2 = 0;
    Header hh;
    nn::Grid g;
    int64_t total = 0;

    // layout of the work buffer: sc_knn's (the far list is the long list), then the counts, the offsets and, for host
    // outputs, the staged rows
    Layout lay;
    const size_t o_hdr = lay.take(sizeof(Header)), o_part = lay.take((size_t)kPartials * 6 * 8);
    const size_t o_count = lay.take(((size_t)cap + 1) * 4), o_start = lay.take(((size_t)cap + 1) * 4), o_cursor = lay.take(((size_t)cap + 1) * 4);
    const size_t o_spts = lay.take((size_t)P * 24), o_sidx = lay.take((size_t)P * 4), o_long = lay.take((size_t)Q * 4);
    const size_t o_qs = lay.take(queries_on_device ? 0 : (size_t)Q * 24), o_ts = lay.take(targets_on_device ? 0 : (size_t)P * 24);
    const size_t o_cnt = lay.take(counts_out && out_on_device ? 0 : (size_t)Q * 4);
    const size_t o_off = lay.take(offsets_out && out_on_device ? 0 : ((size_t)Q + 1) * 8);
    const size_t o_idx = lay.take(stage_rows ? (size_t)capacity * 4 : 0), o_d2 = lay.take(stage_rows ? (size_t)capacity * 8 : 0);
    size_t o_tmp = 0;  // the scans' temporary storage: the last buffer, sized below

    if ((rc = call.enter()) != SC_OK) goto done;
    // the temporary storage of the larger of the two scans (size queries: no device work)
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)(cap + 1), stream));
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp2, (int64_t *)nullptr, (int64_t *)nullptr, (size_t)Q + 1, stream));
    tmp = std::max(tmp, tmp2);
    o_tmp = lay.take(tmp);
    if ((rc = call.grow(lay.total)) != SC_OK) goto done;
    {
        char *const w = call.sl.base;
        Header *hdr = reinterpret_cast<Header *>(w + o_hdr);
        double *partial = reinterpret_cast<double *>(w + o_part);
        uint32_t *count = reinterpret_cast<uint32_t *>(w + o_count), *start = reinterpret_cast<uint32_t *>(w + o_start),
                 *cursor = reinterpret_cast<uint32_t *>(w + o_cursor);
        double *spts = reinterpret_cast<double *>(w + o_spts);
        int *sidx = reinterpret_cast<int *>(w + o_sidx), *longlist = reinterpret_cast<int *>(w + o_long);
        const double *qs_d = queries_on_device ? queries : reinterpret_cast<const double *>(w + o_qs);
        const double *ts_d = targets_on_device ? targets : reinterpret_cast<const double *>(w + o_ts);
        int32_t *cnt_d = counts_out && out_on_device ? counts_out : reinterpret_cast<int32_t *>(w + o_cnt);
        int64_t *off_d = offsets_out && out_on_device ? offsets_out : reinterpret_cast<int64_t *>(w + o_off);
        int32_t *idx_d = stage_rows ? reinterpret_cast<int32_t *>(w + o_idx) : index_out;
        double *d2_d = stage_rows ? reinterpret_cast<double *>(w + o_d2) : d2_out;
        void *tmp_d = w + o_tmp;

        UNIT_TRY(call.sl.wait(stream));
        if (!queries_on_device) UNIT_TRY(hipMemcpyAsync(w + o_qs, queries, (size_t)Q * 24, hipMemcpyHostToDevice, stream));
        if (!targets_on_device) UNIT_TRY(hipMemcpyAsync(w + o_ts, targets, (size_t)P * 24, hipMemcpyHostToDevice, stream));
        UNIT_TRY(hipMemsetAsync(hdr, 0, sizeof(Header), stream));
        hipLaunchKernelGGL(nearest_box_kernel, dim3(box_parts), dim3(kB), 0, stream, ts_d, np, &hdr->bad_targets, partial);
        hipLaunchKernelGGL(nearest_box_final_kernel, dim3(1), dim3(kB), 0, stream, partial, box_parts, hdr->box);
        launch_points_finite(stream, qs_d, Q, &hdr->bad_queries);
        UNIT_TRY(hipGetLastError());
        UNIT_TRY(hipMemcpyAsync(&hh, hdr, sizeof(Header), hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        UNIT_TRY(hipStreamSynchronize(stream));  // the call's first wait: the finite flags and the box
        if (hh.bad_queries != 0u || hh.bad_targets != 0u) {  // device points: the first kernels are the judge
            rc = g_err.fail(SC_ERR_INVALID, hh.bad_queries ? "non-finite coordinate in the device queries" : "non-finite coordinate in the device targets");
            goto done;
        }
        nn::plan_radius_grid(hh.box, hh.box + 3, P, radius, g);
        const int ncell = g.n[0] * g.n[1] * g.n[2];  // <= cap

        UNIT_TRY(hipMemsetAsync(count, 0, ((size_t)ncell + 1) * 4, stream));
        hipLaunchKernelGGL(nearest_hist_kernel, dim3(pblocks), dim3(kB), 0, stream, ts_d, np, g, count);
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(tmp_d, tmp, count, start, ncell + 1, stream));
        UNIT_TRY(hipMemcpyAsync(cursor, start, (size_t)ncell * 4, hipMemcpyDeviceToDevice, stream));
        hipLaunchKernelGGL(nearest_scatter_kernel, dim3(pblocks), dim3(kB), 0, stream, ts_d, np, g, cursor, spts, sidx);
        UNIT_TRY(hipMemsetAsync(off_d + Q, 0, 8, stream));  // the scan reads Q + 1 lengths
        hipLaunchKernelGGL(radius_count_kernel, dim3(qwave_blocks), dim3(kB), 0, stream, qs_d, nq, g, start, spts, cnt_d, off_d, &hdr->longest);
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(tmp_d, tmp, off_d, off_d, (size_t)Q + 1, stream));  // in place: lengths to first places
        UNIT_TRY(hipGetLastError());
        UNIT_TRY(hipMemcpyAsync(&hh.longest, &hdr->longest, 4, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(hipMemcpyAsync(&total, off_d + Q, 8, hipMemcpyDeviceToHost, stream));
        if (counts_out && !out_on_device) UNIT_TRY(hipMemcpyAsync(counts_out, cnt_d, (size_t)Q * 4, hipMemcpyDeviceToHost, stream));
        if (offsets_out && !out_on_device) UNIT_TRY(hipMemcpyAsync(offsets_out, off_d, ((size_t)Q + 1) * 8, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        UNIT_TRY(hipStreamSynchronize(stream));  // the call's second wait: E and the longest row
        *total_out = total;
        if (!rows || capacity < total || total == 0) goto done;  // R6: the rows are written iff they fit

        const int lds_row = (int)std::min<uint32_t>(SC_RADIUS_LDS_ROW, pow2ceil(hh.longest));  // places per wavefront
        hipLaunchKernelGGL(radius_fill_kernel, dim3(qwave_blocks), dim3(kB), (size_t)(kB / 64) * 12 * (size_t)lds_row, stream, qs_d, nq, g, start,
                           spts, sidx, off_d, lds_row, idx_d, d2_d, longlist, &hdr->nlong);
        if (hh.longest > (uint32_t)SC_RADIUS_LDS_ROW)
            hipLaunchKernelGGL(radius_long_kernel, dim3(std::min<uint32_t>(qwave_blocks, kFarBlocks)), dim3(kB), 0, stream, off_d, longlist,
                               &hdr->nlong, idx_d, d2_d);
        UNIT_TRY(hipGetLastError());
        if (stage_rows) {
            UNIT_TRY(hipMemcpyAsync(index_out, idx_d, (size_t)total * 4, hipMemcpyDeviceToHost, stream));
            UNIT_TRY(hipMemcpyAsync(d2_out, d2_d, (size_t)total * 8, hipMemcpyDeviceToHost, stream));
        }
        if (long_out) UNIT_TRY(hipMemcpyAsync(&hh.nlong, &hdr->nlong, 4, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        if (long_out || stage_rows) {
            UNIT_TRY(hipStreamSynchronize(stream));
            if (long_out) *long_out = (int64_t)hh.nlong;
        }
    }

done:
    return rc;
}

int sc_nearest_confusion(const int32_t *index, const int32_t *query_labels, int on_device, int64_t Q, const int32_t *target_labels,
                         int target_labels_on_device, int64_t P, int L, int device, int64_t *counts_out, void *hip_stream) {
    // every argument is judged before the first device call
    if (Q < 0 || Q >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "Q must be 0 .. 2^31 - 1");
    if (P < 0 || P >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "P must be 0 .. 2^31 - 1");
    if (L < 1 || L > kMaxLabels) return g_err.fail(SC_ERR_INVALID, "L must be 1 .. 4096");
    if (!counts_out || (Q > 0 && (!index || !query_labels)) || (P > 0 && !target_labels))
        return g_err.fail(SC_ERR_INVALID, "null argument (index, query_labels, target_labels, counts_out)");
    if (device < 0 || device >= kUnitDevices) return g_err.fail(SC_ERR_INVALID, "device ordinal out of range");
    char msg[160];
    if (!on_device)
        for (int64_t q = 0; q < Q; ++q) {
            if (index[q] < -1 || index[q] >= P) {
                snprintf(msg, sizeof msg, "index %lld is outside -1 .. P - 1", (long long)q);
                return g_err.fail(SC_ERR_INVALID, msg);
            }
            if (query_labels[q] < 0 || query_labels[q] >= L) {
                snprintf(msg, sizeof msg, "query label %lld is outside 0 .. L - 1", (long long)q);
                return g_err.fail(SC_ERR_INVALID, msg);
            }
        }
    if (!target_labels_on_device)
        for (int64_t t = 0; t < P; ++t)
            if (target_labels[t] < 0 || target_labels[t] >= L) {
                snprintf(msg, sizeof msg, "target label %lld is outside 0 .. L - 1", (long long)t);
                return g_err.fail(SC_ERR_INVALID, msg);
            }
    const size_t cells = (size_t)L * L;
    for (size_t k = 0; k < cells; ++k) counts_out[k] = 0;
    if (Q == 0 || P == 0) return SC_OK;  // with no target every index is -1: nothing is counted

    const uint32_t blocks = (uint32_t)std::min<int64_t>((std::max(Q, P) + kB - 1) / kB, 1024);
    int rc = SC_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    UnitCall call(g_err, g_slots, device, stream, rc);
    unsigned int bad = 0;

    Layout lay;
    const size_t o_hdr = lay.take(sizeof(Header)), o_counts = lay.take(cells * 8);
    const size_t o_idx = lay.take(on_device ? 0 : (size_t)Q * 4), o_ql = lay.take(on_device ? 0 : (size_t)Q * 4);
    const size_t o_tl = lay.take(target_labels_on_device ? 0 : (size_t)P * 4);

    if ((rc = call.open(lay.total)) != SC_OK) goto done;
    {
        char *const w = call.sl.base;
        Header *hdr = reinterpret_cast<Header *>(w + o_hdr);
        unsigned long long *counts = reinterpret_cast<unsigned long long *>(w + o_counts);
        const int32_t *idx_d = on_device ? index : reinterpret_cast<const int32_t *>(w + o_idx);
        const int32_t *ql_d = on_device ? query_labels : reinterpret_cast<const int32_t *>(w + o_ql);
        const int32_t *tl_d = target_labels_on_device ? target_labels : reinterpret_cast<const int32_t *>(w + o_tl);

        UNIT_TRY(call.sl.wait(stream));
        if (!on_device) {
            UNIT_TRY(hipMemcpyAsync(w + o_idx, index, (size_t)Q * 4, hipMemcpyHostToDevice, stream));
            UNIT_TRY(hipMemcpyAsync(w + o_ql, query_labels, (size_t)Q * 4, hipMemcpyHostToDevice, stream));
        }
        if (!target_labels_on_device) UNIT_TRY(hipMemcpyAsync(w + o_tl, target_labels, (size_t)P * 4, hipMemcpyHostToDevice, stream));
        UNIT_TRY(hipMemsetAsync(hdr, 0, sizeof(Header), stream));
        UNIT_TRY(hipMemsetAsync(counts, 0, cells * 8, stream));
        hipLaunchKernelGGL(nearest_labels_kernel, dim3(blocks), dim3(kB), 0, stream, idx_d, ql_d, (int)Q, tl_d, (int)P, L, &hdr->bad_labels);
        if (cells <= (size_t)kLdsTable)
            hipLaunchKernelGGL(nearest_confusion_kernel<true>, dim3(blocks), dim3(kB), 0, stream, idx_d, ql_d, (int)Q, tl_d, (int)P, L, counts);
        else
            hipLaunchKernelGGL(nearest_confusion_kernel<false>, dim3(blocks), dim3(kB), 0, stream, idx_d, ql_d, (int)Q, tl_d, (int)P, L, counts);
        UNIT_TRY(hipGetLastError());
        UNIT_TRY(hipMemcpyAsync(&bad, &hdr->bad_labels, 4, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(hipMemcpyAsync(counts_out, counts, cells * 8, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        UNIT_TRY(hipStreamSynchronize(stream));
        if (bad != 0u) {  // device arrays: the labels launch is the judge
            for (size_t k = 0; k < cells; ++k) counts_out[k] = 0;
            rc = g_err.fail(SC_ERR_INVALID, "a label outside 0 .. L - 1 or an index outside -1 .. P - 1 in the device arrays");
        }
    }

done:
    return rc;
}

void sc_nearest_release(void) { release_slots(g_slots); }

}  // extern "C"
