// sc_nearest.h -- the arithmetic of nearest.hip that does not depend on how threads are laid out: the
// plan of the dense grid over the targets, the cell of a coordinate, the ring walk of one query with its stop rule.
// (N1's dist2 is sc_points.h's, shared with dbscan.hip.)
// Host and device: nearest.hip runs it one thread per query; tools/nearest_rehearsal.cpp runs the same text on the
// CPU, one query after the other, against all pairs.  The k nearest follow at the end: the stop rule
// for the k-th place, the enumeration of a ring's runs, and the serial form of the list nearest.hip keeps per wavefront.
// Last, all targets within a radius: its plan, its stop rule and the serial walk of one query.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "sc_points.h"

namespace nn {

using ::dist2;  // N1

constexpr int64_t kMaxCells = (int64_t)1 << 22;  // cap on nx * ny * nz: three 16 MiB tables at most
constexpr int kNearRings = 3;                    // rings 0..3 (at most 7^3 cells) per thread; what is left goes to the far pass
constexpr double kShrink = 1.0 - 1.0 / 1048576.0;  // 1 - 2^-20: the margin of the stop rule, see ring_bound
constexpr double kEdgeMin = 0x1p-480, kEdgeMax = 0x1p480;  // outside this range of cell edges the grid is one cell

struct Grid {
    double lo[3];  // the targets' least coordinate per axis
    double h;      // the edge of a cell, the same on every axis
    int n[3];      // cells per axis; n[0] * n[1] * n[2] <= kMaxCells
    double md2;    // fl(max_distance * max_distance), +inf when unbounded (N3)
};

// The cells a call may use at most: known from P alone, so the work buffer is sized before the box is.
inline int64_t cell_cap(int64_t P) {
    int64_t c = 2 * P;
    if (c < 64) c = 64;
    return c < kMaxCells ? c : kMaxCells;
}

// u(x) = fl(fl(x - lo) / h): the cell coordinate before the floor.  x - lo may overflow to an infinity (the clamp
// takes it); it is never NaN for finite x and lo, and h is a normal number.
SC_HD int cell_of(double x, double lo, double h, int n) {
    const double u = floor((x - lo) / h);
    return (int)fmin(fmax(u, 0.0), (double)(n - 1));
}

// The plan.  One edge h for all axes, n[a] = floor(fl(fl(hi[a] - lo[a]) / h)) + 1: by the monotonicity of rounding
// every target's u lies in [0, n[a]), so a TARGET IS NEVER CLAMPED (cell_of's clamp is a belt for them) -- the proof
// below needs that.  An axis of zero extent gets one cell.  h aims at cell_cap(P) / 2 cells in the box spanned by the
// axes of non-zero extent and grows by a quarter until the product of the counts fits under cell_cap(P): at most
// kPlanSteps times, after which (or when an extent is not finite, or h leaves [kEdgeMin, kEdgeMax]) the grid is ONE
// cell and ring 0 is the whole search.
constexpr int kPlanSteps = 8192;

inline void plan_grid(const double lo[3], const double hi[3], int64_t P, double max_distance, Grid &g) {
    const double cap = (double)cell_cap(P);
    double ext[3], logsum = 0.0;
    int k = 0;
    bool ok = true;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = lo[a];
        g.n[a] = 1;
        ext[a] = hi[a] - lo[a];
        if (!(ext[a] >= 0.0) || !std::isfinite(ext[a])) ok = false;
        if (ext[a] > 0.0) {
            logsum += std::log(ext[a]);
            ++k;
        }
    }
    g.h = 1.0;
    g.md2 = max_distance > 0.0 ? max_distance * max_distance : HUGE_VAL;
    if (!ok || k == 0) return;
    double h = std::exp((logsum - std::log(cap / 2.0)) / k);
    for (int step = 0; step < kPlanSteps; ++step, h *= 1.25) {
        if (!(h >= kEdgeMin)) continue;  // grows into the range
        if (!(h <= kEdgeMax)) return;    // one cell
        double prod = 1.0, cnt[3];
        for (int a = 0; a < 3; ++a) {
            cnt[a] = floor(ext[a] / h) + 1.0;
            prod *= cnt[a];
        }
        if (prod <= cap) {  // also false for an infinite or NaN product
            g.h = h;
            for (int a = 0; a < 3; ++a) g.n[a] = (int)cnt[a];
            return;
        }
    }
}

// N2: the pair (d2, index) is kept lexicographically.
struct Best {
    double d2;
    int idx;
    SC_HD void take(double d, int i) {
        if (d < d2 || (d == d2 && i < idx)) {
            d2 = d;
            idx = i;
        }
    }
};

// ---- the stop rule -----------------------------------------------------------------------------------------------
// Claim.  Let the query's cell be c (cell_of per axis, clamped into the grid) and let rings 0..r around c have been
// visited, r >= 1, ring k = the cells at Chebyshev distance k from c, clipped to the grid.  Then every target t that
// was not visited has a computed d2(q, t) >= ring_bound(h, r) = fl(fl(fl(h r) fl(h r)) kShrink), kShrink = 1 - 2^-20.
//
// Proof.  An unvisited t has a cell ct with |ct[a] - c[a]| >= r + 1 on some axis a.  Write u(x) = fl(fl(x - lo) / h)
// and rho(x) = (x - lo) / h in exact arithmetic.  u carries two roundings: |u - rho| <= |u| 2^-52 (1 + 2^-52) (a
// quotient that underflows is off by less than 2^-1074, and fl(x - lo), the quotient and rho share their sign).
//   Targets are never clamped (plan_grid), so ct = floor(u(tx)) with 0 <= u(tx) < n <= 2^22, |u(tx) - rho(tx)| < 2^-29.
//   High side, ct >= c + r + 1: then u(tx) >= c + r + 1.  The query's cell was not clamped from above (there is no
//   cell beyond n - 1 for t to be in), so floor(u(qx)) <= c, u(qx) < c + 1.  If u(qx) >= -1 then |u(qx)| < 2^22 and
//   rho(qx) < c + 1 + 2^-29; if u(qx) < -1 (a query left of the box, -inf included) then rho(qx) < 0 < c + 1.  Either
//   way rho(tx) - rho(qx) > r - 2^-28.
//   Low side, ct <= c - r - 1: then u(tx) < c - r, rho(tx) < c - r + 2^-29.  The query's cell was not clamped from below,
//   so u(qx) >= c.  If u(qx) <= 2^23, rho(qx) > c - 2^-28; otherwise (a query right of the box, +inf included)
//   rho(qx) > 2^23 - 1 >= c + 2^22 > c.  Either way rho(qx) - rho(tx) > r - 2^-27.
// So the clamped query needs no case of its own: a query outside the box still has every unvisited target more than
// r - 2^-27 cell edges away on that axis, |qx - tx| > h (r - 2^-27) >= h r (1 - 2^-27).
//   N1: dx = fl(qx - tx), |dx| >= |qx - tx| (1 - 2^-53); fl(dx dx) >= dx^2 (1 - 2^-53) (normal: h r >= kEdgeMin =
//   2^-480, so the square is above 2^-961); rounded sums of non-negative terms never fall below a term.  Hence
//   d2 >= h^2 r^2 (1 - 2^-27)^2 (1 - 2^-53)^3 > h^2 r^2 (1 - 2^-25).
//   ring_bound carries three roundings upward at most: <= h^2 r^2 (1 - 2^-20) (1 + 2^-53)^3 < h^2 r^2 (1 - 2^-21), and
//   h r <= kEdgeMax 2^22 = 2^502 does not overflow when squared.  The margin taken is 2^-21 against a need of 2^-25.
//
// Use.  A query stops after ring r when ring_bound > best d2 STRICTLY -- at equality a tie with a smaller index may
// sit in the next ring (N2) -- or when ring_bound >= md2: nothing unvisited can be matched (N3).  It also stops when
// ring r reached the grid's far faces on every axis: nothing is unvisited then, whatever the numbers are.  After
// ring 0 the bound is 0 and stops nobody.
SC_HD double ring_bound(double h, int r) {
    const double hr = h * (double)r;
    return (hr * hr) * kShrink;
}

// Visits ring r of the query cell (cx, cy, cz).  Cells are numbered (z ny + y) nx + x, so a run of cells along x is
// a run of sorted slots: start[first cell] .. start[last cell + 1].  Every loop is bounded by the cell counts or P.
SC_HD void visit_ring(const Grid &g, int cx, int cy, int cz, int r, const uint32_t *__restrict__ start,
                      const double *__restrict__ spts, const int *__restrict__ sidx, double qx, double qy, double qz, Best &best) {
    const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
    const int x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < nx - 1 ? cx + r : nx - 1;
    const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < ny - 1 ? cy + r : ny - 1;
    const int z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < nz - 1 ? cz + r : nz - 1;
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
            const int row = (z * ny + y) * nx;
            const bool face = z - cz == r || cz - z == r || y - cy == r || cy - y == r;
            // a face row is visited whole; of an inner row only its two end cells belong to ring r
            for (int part = 0; part < 2; ++part) {
                int a, b;  // cells a..b of the row
                if (face) {
                    if (part) break;
                    a = x0;
                    b = x1;
                } else {
                    a = b = part ? cx + r : cx - r;
                    if (a < 0 || a > nx - 1) continue;
                }
                const uint32_t t0 = start[row + a], t1 = start[row + b + 1];
                for (uint32_t t = t0; t < t1; ++t)
                    best.take(dist2(qx, qy, qz, spts[3 * (size_t)t], spts[3 * (size_t)t + 1], spts[3 * (size_t)t + 2]), sidx[t]);
            }
        }
}

// The ring walk of one query.  Returns true when the answer is final (best holds it, before N3's test); false when
// kNearRings rings did not settle it: the far pass then searches all P targets.
SC_HD bool ring_search(const Grid &g, const uint32_t *__restrict__ start, const double *__restrict__ spts,
                       const int *__restrict__ sidx, double qx, double qy, double qz, Best &best) {
    const int cx = cell_of(qx, g.lo[0], g.h, g.n[0]), cy = cell_of(qy, g.lo[1], g.h, g.n[1]), cz = cell_of(qz, g.lo[2], g.h, g.n[2]);
    int last = cx > g.n[0] - 1 - cx ? cx : g.n[0] - 1 - cx;  // the ring that reaches the far faces on every axis
    last = cy > last ? cy : last;
    last = g.n[1] - 1 - cy > last ? g.n[1] - 1 - cy : last;
    last = cz > last ? cz : last;
    last = g.n[2] - 1 - cz > last ? g.n[2] - 1 - cz : last;
    best.d2 = HUGE_VAL;
    best.idx = 0x7fffffff;
    for (int r = 0; r <= kNearRings; ++r) {
        visit_ring(g, cx, cy, cz, r, start, spts, sidx, qx, qy, qz, best);
        if (r >= last) return true;
        const double b = ring_bound(g.h, r);
        if (b > best.d2 || b >= g.md2) return true;
    }
    return false;
}

// ---- the k nearest --------------------------------------------------------------------------------
// K2: the key of a target is (d2, index), compared lexicographically; keys of one query are distinct.
SC_HD bool key_less(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

// The least ring that reaches the grid's far faces on every axis: after it nothing is unvisited.
SC_HD int last_ring(const Grid &g, int cx, int cy, int cz) {
    int last = cx > g.n[0] - 1 - cx ? cx : g.n[0] - 1 - cx;
    last = cy > last ? cy : last;
    last = g.n[1] - 1 - cy > last ? g.n[1] - 1 - cy : last;
    last = cz > last ? cz : last;
    return g.n[2] - 1 - cz > last ? g.n[2] - 1 - cz : last;
}

// The stop rule after ring r, the claim above put to use for the k-th place: every unvisited target has a computed
// d2 >= ring_bound(h, r).  The search is over when the list is full and the bound exceeds the k-th d2 STRICTLY (at
// equality an unvisited target of a smaller index would take the k-th place, K2), when the bound has reached md2
// (nothing unvisited counts, K3), or when ring r reached the far faces.  With k = 1 this is ring_search's rule.
SC_HD bool knn_settled(const Grid &g, int r, int last, bool full, double kth_d2) {
    if (r >= last) return true;
    const double b = ring_bound(g.h, r);
    return (full && b > kth_d2) || b >= g.md2;
}

// Calls f(t0, t1) for every run of sorted slots of ring r: visit_ring's enumeration (a face row whole, of an inner
// row its two end cells), without what is done per slot.
template <class F>
SC_HD void for_ring_runs(const Grid &g, int cx, int cy, int cz, int r, const uint32_t *__restrict__ start, F &&f) {
    const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
    const int x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < nx - 1 ? cx + r : nx - 1;
    const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < ny - 1 ? cy + r : ny - 1;
    const int z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < nz - 1 ? cz + r : nz - 1;
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
            const int row = (z * ny + y) * nx;
            const bool face = z - cz == r || cz - z == r || y - cy == r || cy - y == r;
            if (face) {
                f(start[row + x0], start[row + x1 + 1]);
            } else {
                if (cx - r >= 0) f(start[row + cx - r], start[row + cx - r + 1]);
                if (r > 0 && cx + r <= nx - 1) f(start[row + cx + r], start[row + cx + r + 1]);
            }
        }
}

// The serial form of the list: up to k keys in rising order in the caller's arrays.  offer() keeps the k smallest of
// the keys below md2 it was given, whatever their order (K2, K3).  nearest.hip holds the same list in LDS and inserts
// with a wavefront; the answer is the same set in the same order.
struct KList {
    double *d2;
    int *idx;
    int k, n;
    SC_HD bool full() const { return n == k; }
    SC_HD double kth() const { return n == k ? d2[k - 1] : HUGE_VAL; }
    SC_HD void offer(double d, int i, double md2) {
        if (!(d < md2) || (n == k && !key_less(d, i, d2[k - 1], idx[k - 1]))) return;
        int j = n < k ? n : k - 1;  // the place that is freed: behind the list, or the k-th
        for (; j > 0 && key_less(d, i, d2[j - 1], idx[j - 1]); --j) {
            d2[j] = d2[j - 1];
            idx[j] = idx[j - 1];
        }
        d2[j] = d;
        idx[j] = i;
        if (n < k) ++n;
    }
};

// The ring walk of one query for its k nearest, serial.  True when the list is final; false when kNearRings rings did
// not settle it: the far pass then starts again from an empty list over all P targets.
SC_HD bool knn_ring_search(const Grid &g, const uint32_t *__restrict__ start, const double *__restrict__ spts,
                           const int *__restrict__ sidx, double qx, double qy, double qz, KList &list) {
    const int cx = cell_of(qx, g.lo[0], g.h, g.n[0]), cy = cell_of(qy, g.lo[1], g.h, g.n[1]), cz = cell_of(qz, g.lo[2], g.h, g.n[2]);
    const int last = last_ring(g, cx, cy, cz);
    list.n = 0;
    for (int r = 0; r <= kNearRings; ++r) {
        for_ring_runs(g, cx, cy, cz, r, start, [&](uint32_t t0, uint32_t t1) {
            for (uint32_t t = t0; t < t1; ++t)
                list.offer(dist2(qx, qy, qz, spts[3 * (size_t)t], spts[3 * (size_t)t + 1], spts[3 * (size_t)t + 2]), sidx[t], g.md2);
        });
        if (knn_settled(g, r, last, list.full(), list.kth())) return true;
    }
    return false;
}

// The grid of a k-nearest call aims at `aim` targets per cell, so that four rings can hold k of them: plan_grid is
// given max(1, P / aim) as its count.  cell_cap is monotone, so the cells stay under cell_cap(P), from which the
// buffer was sized, and no target is clamped whatever the count is (plan_grid's n[a] comes from the box alone).
// Measured (tools/bench_knn.py, a surface cloud of 226 689 points): at k = 1, 8, 16 and 32 the least
// aim tried, 1, was the fastest and sent nothing to the far pass; at k = 300 aims of 16 and 32 were equal within 1 %
// and 64 slower, and k / 10 lies between them.  Between 32 and 300 nothing was measured: k / 10 is used there too.
inline int knn_aim(int k) { return k <= 32 ? 1 : k / 10; }

// ---- all targets within a radius ----------------------------------------------------------------------
// R2: t is a neighbour of q iff d2(q, t) < md2 = fl(radius * radius), strict.  The claim above ring_bound holds for any
// planned grid: after rings 0..r every unvisited target has a computed d2 >= ring_bound(h, r).  So the row of a query
// is complete after the first ring r with ring_bound(h, r) >= md2 -- nothing unvisited can be a neighbour -- or with
// r >= last_ring: nothing is unvisited.  There is no cap on the rings and no pass over all targets: the walk ends at
// last_ring at the latest, which is below the largest cell count.  Correctness rests on this rule alone, whatever h is.
SC_HD bool radius_settled(const Grid &g, int r, int last) { return r >= last || ring_bound(g.h, r) >= g.md2; }

// The plan, for speed only: plan_grid as it is; then, if its cells are so small that ring 1 does not close the search
// (ring_bound(h, 1) < md2), the edge is widened to just above the radius -- h = fl(radius (1 + 2^-18)), for which
// ring_bound(h, 1) > radius^2 (1 + 2^-17) (1 - 2^-19) > md2; the inequality is tested, not trusted -- and the counts
// are computed anew from the box and the new h, n[a] = floor(fl(ext[a] / h)) + 1, exactly as plan_grid does: NO TARGET
// IS CLAMPED, whatever h is.  A wider edge can only shrink the product of the counts; it is compared with cell_cap(P)
// all the same (plan_grid's one-cell answer has h = 1, which says nothing about the box).  Whatever does not fit --
// h outside [kEdgeMin, kEdgeMax], an extent that is not finite, a product over the cap -- is ONE cell: ring 0 is then
// the last ring.  Rings 0 and 1 (27 cells) are the whole search in every ordinary case.
inline void plan_radius_grid(const double lo[3], const double hi[3], int64_t P, double radius, Grid &g) {
    plan_grid(lo, hi, P, radius, g);
    if (ring_bound(g.h, 1) >= g.md2) return;
    const double h = radius * (1.0 + 0x1p-18);
    double prod = 1.0, cnt[3] = {1.0, 1.0, 1.0};
    bool ok = h >= kEdgeMin && h <= kEdgeMax && ring_bound(h, 1) >= g.md2;
    for (int a = 0; a < 3 && ok; ++a) {
        const double ext = hi[a] - lo[a];
        if (!(ext >= 0.0) || !std::isfinite(ext)) ok = false;
        cnt[a] = floor(ext / h) + 1.0;
        prod *= cnt[a];
    }
    if (!ok || !(prod <= (double)cell_cap(P))) {  // also an infinite or NaN product
        g.h = 1.0;
        g.n[0] = g.n[1] = g.n[2] = 1;
        return;
    }
    g.h = h;
    for (int a = 0; a < 3; ++a) g.n[a] = (int)cnt[a];
}

// R3: n keys (d2, index) into rising order by a bitonic network over the next power of two whose comparators all point
// upwards (a merge step's first exchange is with the mirror place i ^ (k - 1), the others with i ^ j): the places from
// n on hold, virtually, the largest key (+inf, INT_MAX), which such a comparator never moves, so an exchange with a
// place >= n is simply skipped.  Lane `lane` of `lanes` takes the places i = lane, lane + lanes, ... whose partner lies
// above them; within a step every place belongs to one pair, so only between steps does a lane read what another one
// wrote: order() stands there (nearest.hip: a fence fit for where the keys live; the rehearsal, one lane, nothing).
// ceil(log2 n) (ceil(log2 n) + 1) / 2 steps of at most ceil(n / lanes) exchanges per lane; n < 2^31.
template <class Order>
SC_HD void sort_row(double *kd, int *ki, int n, int lane, int lanes, Order &&order) {
    const uint32_t un = (uint32_t)n;
    for (uint32_t k = 2; (k >> 1) < un; k <<= 1)  // k <= 2^31
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            order();
            const uint32_t flip = j == (k >> 1) ? k - 1 : j;
            for (uint32_t i = (uint32_t)lane; i < un; i += (uint32_t)lanes) {
                const uint32_t l = i ^ flip;
                if (l > i && l < un) {
                    const double di = kd[i], dl = kd[l];
                    const int ii = ki[i], il = ki[l];
                    if (key_less(dl, il, di, ii)) {
                        kd[i] = dl;
                        ki[i] = il;
                        kd[l] = di;
                        ki[l] = ii;
                    }
                }
            }
        }
    order();
}

// The serial walk of one query: f(d2, index) for every neighbour (R2), in visiting order (R3's order is the caller's
// sort).  Every loop is bounded by the cell counts or P.
template <class F>
SC_HD void radius_search(const Grid &g, const uint32_t *__restrict__ start, const double *__restrict__ spts,
                         const int *__restrict__ sidx, double qx, double qy, double qz, F &&f) {
    const int cx = cell_of(qx, g.lo[0], g.h, g.n[0]), cy = cell_of(qy, g.lo[1], g.h, g.n[1]), cz = cell_of(qz, g.lo[2], g.h, g.n[2]);
    const int last = last_ring(g, cx, cy, cz);
    for (int r = 0;; ++r) {
        for_ring_runs(g, cx, cy, cz, r, start, [&](uint32_t t0, uint32_t t1) {
            for (uint32_t t = t0; t < t1; ++t) {
                const double d = dist2(qx, qy, qz, spts[3 * (size_t)t], spts[3 * (size_t)t + 1], spts[3 * (size_t)t + 2]);
                if (d < g.md2) f(d, sidx[t]);
            }
        });
        if (radius_settled(g, r, last)) return;
    }
}

}  // namespace nn
