// dbscan.hip -- the clustering of OrganSegmentation on the GPU.
//
// Replaces open3d's `cluster_dbscan(eps, min_points)` as plant3dvision/tasks/proc3d.py::OrganSegmentation.run
// (:419-521) calls it, for one cloud of P float64 points.  PARITY UNPINNED: open3d is not available,
// this restates what its sequential loop computes in an order-free form:
//   1. d2(i, j) = ((dx dx) + (dy dy)) + (dz dz) in IEEE binary64 without contraction (-ffp-contract=off);
//   2. j is a neighbour of i iff d2(i, j) < eps * eps (strict; the product rounded once; i is its own neighbour);
//   3. i is core iff it has at least min_points neighbours;
//   4. clusters = connected components of the core points under 2; id = rank of the component's smallest index;
//   5. a non-core point with core neighbours takes the smallest id among them;  6. every other point is -1.
//
// No neighbour list is stored: every pass finds its candidates again in a uniform grid of cells (points sorted by a
// hash of their cell, a counting sort) and decides each pair with rules 1 and 2 alone.  Launches per call: finite (sc_points.h),
// histogram, [scan], scatter, core, link, flatten, border, [scan], labels.  The link launch is the only one in
// which blocks exchange data (the parent array): every access to it there is a relaxed agent-scope atomic.
// Stand-alone unit: nothing shared with the carve's engine; rule 1 (dist2) and the judges of non-finite coordinates
// are sc_points.h, shared with nearest.hip.

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "sc_points.h"
#include "sc_unionfind.h"
#include "sc_unit.h"

namespace {

constexpr int kB = 256;

thread_local UnitError g_err;

// ---- the cell grid ---------------------------------------------------------------------------------------------
// Cell of a coordinate: c = floor(clamp(q, -2^40, 2^40)) with q = fl(fl(x - a) / edge), a = the coordinate of point
// 0 (the anchor; any finite number would do) and edge = fl(eps * kEdgeFactor), kEdgeFactor = 1 + 2^-8.
//
// Why the 27 cells around a point's own hold every neighbour.  Let d2(i, j) < eps2 = fl(eps * eps) as computed.
// Rounded sums of non-negative terms never fall below a term, so fl(dx dx) < eps2 for dx = fl(xi - xj); eps2 is a
// normal number (checked by the entry; a product that underflowed is below it anyway), hence |dx| < eps (1 + 2^-52),
// and |xi - xj| <= |dx| (1 + 2^-52) < eps (1 + 2^-50).  In exact arithmetic the two quotients r = (x - a) / edge
// then differ by less than (1 + 2^-50) / ((1 + 2^-8)(1 - 2^-53)) < 1 - 2^-9.  q carries two roundings:
// |q - r| <= |r| 2^-52 (a quotient that underflows is off by less than 2^-1074), at most 2^-11 while |r| <= 2^41.
// So if both |q| are below 2^41 they differ by less than 1 - 2^-9 + 2^-10 < 1, their floors by at most 1, and the
// clamp, being monotone, never separates what was adjacent.  If one |q| is 2^41 or more, the other is beyond
// 2^41 - 2 > 2^40 on the same side and both cells are that side's clamp.  (x - a may overflow to an infinity: the
// clamp again; it is never NaN for finite x.)  The clamp costs time only: what lies further than 2^40 cells from
// point 0 shares one layer of cells per axis and side.
//
// Cells are 3 x 41 bits and a sign: points are binned by a 64-bit hash of them, reduced to a power-of-two table, and
// carry the low 32 bits of their cell.  A bucket may hold several cells: a candidate is looked at only if the low
// 32 bits of its cell are those of the cell asked for.  The 27 cells asked for differ from one another by at most 2
// per axis, so no two of them share their low bits: a point of the 27 cells is visited exactly once, a stray point
// that collides in hash and low bits at most once, and only rule 2 decides what a visited pair is.
constexpr double kEdgeFactor = 1.0 + 1.0 / 256.0;
constexpr double kCellClamp = 1099511627776.0;  // 2^40
constexpr int64_t kCellMax = (int64_t)1 << 40;

struct Grid {
    double ax, ay, az, edge, eps2;
    uint32_t mask;  // buckets - 1
};

__device__ __forceinline__ int64_t cell_of(double x, double a, double edge) {
    const double q = (x - a) / edge;
    return (int64_t)floor(fmax(fmin(q, kCellClamp), -kCellClamp));
}

__device__ __forceinline__ uint32_t bucket_of(int64_t cx, int64_t cy, int64_t cz, uint32_t mask) {
    unsigned long long h = (unsigned long long)cx * 0x9E3779B97F4A7C15ull ^ (unsigned long long)cy * 0xC2B2AE3D27D4EB4Full ^
                           (unsigned long long)cz * 0x165667B19E3779F9ull;
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    return (uint32_t)h & mask;
}

// Calls f(t, original index of t) for every sorted slot t whose point is a neighbour (rules 1, 2) of the point at
// (x, y, z), itself included; f returns true to stop.
template <class F>
__device__ __forceinline__ void for_each_neighbour(const Grid &g, const uint32_t *__restrict__ start,
                                                   const uint4 *__restrict__ scell, const double *__restrict__ spts,
                                                   double x, double y, double z, F f) {
    const int64_t cx = cell_of(x, g.ax, g.edge), cy = cell_of(y, g.ay, g.edge), cz = cell_of(z, g.az, g.edge);
    for (int dzc = -1; dzc <= 1; ++dzc)
        for (int dyc = -1; dyc <= 1; ++dyc)
            for (int dxc = -1; dxc <= 1; ++dxc) {
                const int64_t tx = cx + dxc, ty = cy + dyc, tz = cz + dzc;
                if (tx < -kCellMax || ty < -kCellMax || tz < -kCellMax || tx > kCellMax || ty > kCellMax || tz > kCellMax) continue;
                const uint32_t b = bucket_of(tx, ty, tz, g.mask);
                const uint32_t t0 = start[b], t1 = start[b + 1];
                for (uint32_t t = t0; t < t1; ++t) {
                    const uint4 c = scell[t];
                    if (c.x != (uint32_t)tx || c.y != (uint32_t)ty || c.z != (uint32_t)tz) continue;
                    const double d2 = dist2(x, y, z, spts[3 * (size_t)t], spts[3 * (size_t)t + 1], spts[3 * (size_t)t + 2]);
                    if (d2 < g.eps2)
                        if (f(t, (int)c.w)) return;
                }
            }
}

// ---- counting sort by bucket -----------------------------------------------------------------------------------
__global__ __launch_bounds__(kB) void dbscan_hist_kernel(const double *__restrict__ pts, int P, Grid g, uint32_t *__restrict__ count) {
    const int i = (int)(blockIdx.x * kB + threadIdx.x);
    if (i >= P) return;
    const int64_t cx = cell_of(pts[3 * (size_t)i], g.ax, g.edge), cy = cell_of(pts[3 * (size_t)i + 1], g.ay, g.edge),
                  cz = cell_of(pts[3 * (size_t)i + 2], g.az, g.edge);
    atomicAdd(&count[bucket_of(cx, cy, cz, g.mask)], 1u);
}

// cursor = a copy of start; afterwards cursor[b] == start[b + 1].  The order inside a bucket is whatever the atomics
// give; no result depends on it.  Also sets every point's state by original index.
__global__ __launch_bounds__(kB) void dbscan_scatter_kernel(const double *__restrict__ pts, int P, Grid g, uint32_t *__restrict__ cursor,
                                                            uint4 *__restrict__ scell, double *__restrict__ spts,
                                                            int *__restrict__ parent, int *__restrict__ rootof, int *__restrict__ isroot) {
    const int i = (int)(blockIdx.x * kB + threadIdx.x);
    if (i >= P) return;
    const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    const int64_t cx = cell_of(x, g.ax, g.edge), cy = cell_of(y, g.ay, g.edge), cz = cell_of(z, g.az, g.edge);
    const uint32_t t = atomicAdd(&cursor[bucket_of(cx, cy, cz, g.mask)], 1u);
    scell[t] = make_uint4((uint32_t)cx, (uint32_t)cy, (uint32_t)cz, (uint32_t)i);  // the cell's low bits
    spts[3 * (size_t)t] = x;
    spts[3 * (size_t)t + 1] = y;
    spts[3 * (size_t)t + 2] = z;
    parent[i] = i;
    rootof[i] = -1;
    isroot[i] = 0;
}

// ---- core flags (rule 3) ---------------------------------------------------------------------------------------
// One thread per sorted slot.  The count stops at min_points: only whether it is reached matters.
__global__ __launch_bounds__(kB) void dbscan_core_kernel(int P, Grid g, int64_t minp, const uint32_t *__restrict__ start,
                                                         const uint4 *__restrict__ scell, const double *__restrict__ spts,
                                                         uint8_t *__restrict__ core) {
    const int s = (int)(blockIdx.x * kB + threadIdx.x);
    if (s >= P) return;
    int64_t n = 0;
    for_each_neighbour(g, start, scell, spts, spts[3 * (size_t)s], spts[3 * (size_t)s + 1], spts[3 * (size_t)s + 2],
                       [&](uint32_t, int) { return ++n >= minp; });
    core[s] = n >= minp ? 1 : 0;
}

// ---- link (rule 4) ---------------------------------------------------------------------------------------------
// parent[] is indexed by ORIGINAL index; find_root / unite and the rule every access to it obeys inside this launch are
// sc_unionfind.h, shared with graph.hip: min-index roots, so each component's root is its smallest index.
__global__ __launch_bounds__(kB) void dbscan_link_kernel(int P, Grid g, const uint32_t *__restrict__ start, const uint4 *__restrict__ scell,
                                                         const double *__restrict__ spts, const uint8_t *__restrict__ core, int *parent) {
    const int s = (int)(blockIdx.x * kB + threadIdx.x);
    if (s >= P || !core[s]) return;
    const int i = (int)scell[s].w;
    for_each_neighbour(g, start, scell, spts, spts[3 * (size_t)s], spts[3 * (size_t)s + 1], spts[3 * (size_t)s + 2],
                       [&](uint32_t t, int j) {
                           if (j < i && core[t]) unite(parent, i, j);  // each pair once, from its larger index
                           return false;
                       });
}

// ---- flatten, border (rule 5), labels --------------------------------------------------------------------------
// parent[] is final here (a kernel boundary lies behind the link launch) and is only read: plain loads.
__global__ __launch_bounds__(kB) void dbscan_flatten_kernel(int P, const uint4 *__restrict__ scell, const uint8_t *__restrict__ core,
                                                            const int *__restrict__ parent, int *__restrict__ rootof, int *__restrict__ isroot) {
    const int s = (int)(blockIdx.x * kB + threadIdx.x);
    if (s >= P || !core[s]) return;
    const int i = (int)scell[s].w;
    int r = i;
    while (parent[r] != r) r = parent[r];
    rootof[i] = r;
    if (r == i) isroot[i] = 1;
}

// A non-core point reads rootof[] of core points only (written by the launch before) and writes its own.  Ids rise
// with the roots' indices (rule 4), so the smallest root is the smallest id.
__global__ __launch_bounds__(kB) void dbscan_border_kernel(int P, Grid g, const uint32_t *__restrict__ start, const uint4 *__restrict__ scell,
                                                           const double *__restrict__ spts, const uint8_t *__restrict__ core, int *rootof) {
    const int s = (int)(blockIdx.x * kB + threadIdx.x);
    if (s >= P || core[s]) return;
    int best = 0x7fffffff;
    for_each_neighbour(g, start, scell, spts, spts[3 * (size_t)s], spts[3 * (size_t)s + 1], spts[3 * (size_t)s + 2],
                       [&](uint32_t t, int j) {
                           if (core[t]) best = min(best, rootof[j]);
                           return false;
                       });
    if (best != 0x7fffffff) rootof[(int)scell[s].w] = best;
}

// rank = exclusive sum of isroot: the number of roots with a smaller index, i.e. the cluster id of rule 4
__global__ __launch_bounds__(kB) void dbscan_labels_kernel(int P, const int *__restrict__ rootof, const int *__restrict__ isroot,
                                                           const int *__restrict__ rank, int32_t *__restrict__ labels,
                                                           int32_t *__restrict__ nclusters) {
    const int i = (int)(blockIdx.x * kB + threadIdx.x);
    if (i >= P) return;
    const int r = rootof[i];
    labels[i] = r < 0 ? -1 : rank[r];
    if (i == P - 1) *nclusters = rank[i] + isroot[i];
}

// ---- host side -------------------------------------------------------------------------------------------------
// Work buffers are kept per device: the slot protocol of sc_unit.h.
WorkSlot g_slots[kUnitDevices];

}  // namespace

extern "C" {

const char *sc_dbscan_last_error(void) { return g_err.msg; }

int sc_dbscan(const double *points, int points_on_device, int64_t P, double eps, int64_t min_points, int device,
              int32_t *labels_out, int labels_on_device, int32_t *nclusters_out, void *hip_stream) {
    // every argument is judged before the first device call
    if (!points || !labels_out) return g_err.fail(SC_ERR_INVALID, "null argument (points, labels_out)");
    if (P < 0 || P >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "P must be 0 .. 2^31 - 1");
    if (!std::isfinite(eps) || !(eps > 0.0)) return g_err.fail(SC_ERR_INVALID, "eps must be finite and positive");
    if (!(eps * eps >= DBL_MIN) || !std::isfinite(eps * eps))
        return g_err.fail(SC_ERR_INVALID, "eps * eps must be a normal number (eps out of range)");
    if (min_points < 0) return g_err.fail(SC_ERR_INVALID, "min_points must not be negative");
    if (device < 0 || device >= kUnitDevices) return g_err.fail(SC_ERR_INVALID, "device ordinal out of range");
    if (!points_on_device && first_non_finite(g_err, points, P, "point") != SC_OK) return SC_ERR_INVALID;
    if (P == 0) {
        if (nclusters_out) *nclusters_out = 0;
        return SC_OK;
    }

    const int n = (int)P;
    uint32_t nb = 64;  // buckets: a power of two, at least P (at most 2^30)
    while (nb < (uint32_t)std::min<int64_t>(P, (int64_t)1 << 30)) nb <<= 1;
    const uint32_t blocks = (uint32_t)((P + kB - 1) / kB);
    const int64_t minp = std::max<int64_t>(min_points, 1);  // a point is its own neighbour: 0 behaves as 1

    int rc = SC_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    UnitCall call(g_err, g_slots, device, stream, rc);
    size_t tmp1 = 0, tmp2 = 0;
    double anchor[3] = {0, 0, 0};
    unsigned int bad = 0;
    int32_t ncl = 0;
    Grid g;

    // layout of the work buffer
    Layout lay;
    const size_t o_hdr = lay.take(256);  // the non-finite flag, nclusters
    const size_t o_count = lay.take(((size_t)nb + 1) * 4), o_start = lay.take(((size_t)nb + 1) * 4),
                 o_cursor = lay.take(((size_t)nb + 1) * 4);
    const size_t o_scell = lay.take((size_t)P * 16), o_spts = lay.take((size_t)P * 24), o_core = lay.take((size_t)P);
    const size_t o_parent = lay.take((size_t)P * 4), o_rootof = lay.take((size_t)P * 4), o_isroot = lay.take((size_t)P * 4),
                 o_rank = lay.take((size_t)P * 4);
    const size_t o_pts = lay.take(points_on_device ? 0 : (size_t)P * 24), o_lab = lay.take(labels_on_device ? 0 : (size_t)P * 4);
    size_t o_tmp = 0;  // the scans' temporary storage: the last buffer, sized below

    if ((rc = call.enter()) != SC_OK) goto done;
    // the scans' temporary storage (a size query: no device work)
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp1, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)(nb + 1), stream));
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp2, (const int *)nullptr, (int *)nullptr, n, stream));
    o_tmp = lay.take(std::max(tmp1, tmp2));
    if ((rc = call.grow(lay.total)) != SC_OK) goto done;
    {
        char *const w = call.sl.base;
        unsigned int *flag = reinterpret_cast<unsigned int *>(w + o_hdr);
        uint32_t *count = reinterpret_cast<uint32_t *>(w + o_count), *start = reinterpret_cast<uint32_t *>(w + o_start),
                 *cursor = reinterpret_cast<uint32_t *>(w + o_cursor);
        uint4 *scell = reinterpret_cast<uint4 *>(w + o_scell);
        double *spts = reinterpret_cast<double *>(w + o_spts);
        uint8_t *core = reinterpret_cast<uint8_t *>(w + o_core);
        int *parent = reinterpret_cast<int *>(w + o_parent), *rootof = reinterpret_cast<int *>(w + o_rootof),
            *isroot = reinterpret_cast<int *>(w + o_isroot), *rank = reinterpret_cast<int *>(w + o_rank);
        int32_t *ncl_d = reinterpret_cast<int32_t *>(w + o_hdr + 64);
        const double *pts_d = points_on_device ? points : reinterpret_cast<const double *>(w + o_pts);
        int32_t *lab_d = labels_on_device ? labels_out : reinterpret_cast<int32_t *>(w + o_lab);
        void *tmp_d = w + o_tmp;

        UNIT_TRY(call.sl.wait(stream));
        if (!points_on_device)
            UNIT_TRY(hipMemcpyAsync(w + o_pts, points, (size_t)P * 24, hipMemcpyHostToDevice, stream));
        UNIT_TRY(hipMemsetAsync(flag, 0, 128, stream));
        launch_points_finite(stream, pts_d, P, flag);
        UNIT_TRY(hipGetLastError());
        UNIT_TRY(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(hipMemcpyAsync(anchor, pts_d, 24, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        UNIT_TRY(hipStreamSynchronize(stream));
        if (bad != 0u) {  // device points: the first kernel is the judge
            rc = g_err.fail(SC_ERR_INVALID, "non-finite coordinate in the device points");
            goto done;
        }
        g.ax = anchor[0];
        g.ay = anchor[1];
        g.az = anchor[2];
        g.edge = eps * kEdgeFactor;
        g.eps2 = eps * eps;
        g.mask = nb - 1;

        UNIT_TRY(hipMemsetAsync(count, 0, ((size_t)nb + 1) * 4, stream));
        hipLaunchKernelGGL(dbscan_hist_kernel, dim3(blocks), dim3(kB), 0, stream, pts_d, n, g, count);
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(tmp_d, tmp1, count, start, (int)(nb + 1), stream));
        UNIT_TRY(hipMemcpyAsync(cursor, start, (size_t)nb * 4, hipMemcpyDeviceToDevice, stream));
        hipLaunchKernelGGL(dbscan_scatter_kernel, dim3(blocks), dim3(kB), 0, stream, pts_d, n, g, cursor, scell, spts, parent, rootof,
                           isroot);
        hipLaunchKernelGGL(dbscan_core_kernel, dim3(blocks), dim3(kB), 0, stream, n, g, minp, start, scell, spts, core);
        hipLaunchKernelGGL(dbscan_link_kernel, dim3(blocks), dim3(kB), 0, stream, n, g, start, scell, spts, core, parent);
        hipLaunchKernelGGL(dbscan_flatten_kernel, dim3(blocks), dim3(kB), 0, stream, n, scell, core, parent, rootof, isroot);
        hipLaunchKernelGGL(dbscan_border_kernel, dim3(blocks), dim3(kB), 0, stream, n, g, start, scell, spts, core, rootof);
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(tmp_d, tmp2, isroot, rank, n, stream));
        hipLaunchKernelGGL(dbscan_labels_kernel, dim3(blocks), dim3(kB), 0, stream, n, rootof, isroot, rank, lab_d, ncl_d);
        UNIT_TRY(hipGetLastError());
        if (!labels_on_device) UNIT_TRY(hipMemcpyAsync(labels_out, lab_d, (size_t)P * 4, hipMemcpyDeviceToHost, stream));
        if (nclusters_out) UNIT_TRY(hipMemcpyAsync(&ncl, ncl_d, 4, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        if (!labels_on_device || nclusters_out) {
            UNIT_TRY(hipStreamSynchronize(stream));
            if (nclusters_out) *nclusters_out = ncl;
        }
    }

done:
    return rc;
}

void sc_dbscan_release(void) { release_slots(g_slots); }

}  // extern "C"
