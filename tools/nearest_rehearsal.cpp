// nearest_rehearsal.cpp -- the logic of csrc/nearest.hip on the CPU: the same sc_nearest.h (grid plan,
// cells, ring walk, stop rule), one query after the other, against all pairs under rules N1-N3.  No GPU, no runtime.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I plant-3d-vision_amd/csrc \
//       tools/nearest_rehearsal.cpp -o build/nearest_rehearsal && build/nearest_rehearsal
// A query the ring walk does not settle is counted as "far" (the device's far pass IS the all-pairs loop below).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "sc_nearest.h"

typedef std::vector<double> Cloud;  // x y z x y z ...

static int g_fail = 0;

static void run(const char *name, const Cloud &qs, const Cloud &ts, double max_distance) {
    const int64_t Q = (int64_t)qs.size() / 3, P = (int64_t)ts.size() / 3;
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int64_t t = 0; t < P; ++t)
        for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], ts[3 * t + a]);
            hi[a] = fmax(hi[a], ts[3 * t + a]);
        }
    nn::Grid g;
    nn::plan_grid(lo, hi, P, max_distance, g);
    const int64_t ncell = (int64_t)g.n[0] * g.n[1] * g.n[2];
    if (ncell > nn::cell_cap(P) || ncell < 1) {
        printf("%s: %lld cells over the cap\n", name, (long long)ncell);
        ++g_fail;
        return;
    }
    auto cell = [&](const double *p) {
        return (nn::cell_of(p[2], g.lo[2], g.h, g.n[2]) * g.n[1] + nn::cell_of(p[1], g.lo[1], g.h, g.n[1])) * g.n[0] +
               nn::cell_of(p[0], g.lo[0], g.h, g.n[0]);
    };
    std::vector<uint32_t> start(ncell + 1, 0), cursor(ncell + 1, 0);
    for (int64_t t = 0; t < P; ++t) ++start[cell(&ts[3 * t]) + 1];
    for (int64_t c = 0; c < ncell; ++c) start[c + 1] += start[c];
    cursor = start;
    Cloud spts(3 * P);
    std::vector<int> sidx(P);
    for (int64_t t = P - 1; t >= 0; --t) {  // backwards: the order inside a cell must not matter
        const uint32_t s = cursor[cell(&ts[3 * t])]++;
        for (int a = 0; a < 3; ++a) spts[3 * s + a] = ts[3 * t + a];
        sidx[s] = (int)t;
    }
    int64_t far = 0, wrong = 0, ties = 0, unmatched = 0;
    for (int64_t q = 0; q < Q; ++q) {
        nn::Best want;
        want.d2 = HUGE_VAL;
        want.idx = 0x7fffffff;
        int equal = 0;
        for (int64_t t = 0; t < P; ++t) {
            const double d = nn::dist2(qs[3 * q], qs[3 * q + 1], qs[3 * q + 2], ts[3 * t], ts[3 * t + 1], ts[3 * t + 2]);
            if (d < want.d2) {
                want.d2 = d;
                want.idx = (int)t;
                equal = 0;
            } else if (d == want.d2) {
                ++equal;
            }
        }
        ties += equal > 0;
        nn::Best got;
        if (!nn::ring_search(g, start.data(), spts.data(), sidx.data(), qs[3 * q], qs[3 * q + 1], qs[3 * q + 2], got)) {
            ++far;
            continue;
        }
        const bool m_want = want.d2 < g.md2, m_got = got.d2 < g.md2;
        unmatched += !m_want;
        if (m_want != m_got || (m_want && (got.d2 != want.d2 || got.idx != want.idx))) ++wrong;
    }
    printf("%-28s Q %6lld P %6lld grid %d x %d x %d h %.4g: far %lld, ties %lld, unmatched %lld, wrong %lld\n", name, (long long)Q,
           (long long)P, g.n[0], g.n[1], g.n[2], g.h, (long long)far, (long long)ties, (long long)unmatched, (long long)wrong);
    if (wrong) ++g_fail;
}

int main() {
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    auto box = [&](int64_t n, double lo, double hi) {
        Cloud c(3 * n);
        for (auto &v : c) v = lo + (hi - lo) * uni(rng);
        return c;
    };
    for (int64_t P : {1, 2, 63, 257, 5000}) run("uniform", box(2000, -0.5, 1.5), box(P, 0.0, 1.0), 0.0);
    run("uniform, max_distance", box(2000, -0.5, 1.5), box(5000, 0.0, 1.0), 0.05);
    Cloud lattice, centres;
    for (int x = 0; x < 6; ++x)
        for (int y = 0; y < 6; ++y)
            for (int z = 0; z < 6; ++z) {
                for (double v : {(double)x, (double)y, (double)z}) lattice.push_back(v);
                for (double v : {x + 0.5, y + 0.5, z + 0.5}) centres.push_back(v);
                for (double v : {x + 0.5, (double)y, (double)z}) centres.push_back(v);
                for (double v : {(double)x, (double)y, (double)z}) centres.push_back(v);
            }
    for (int k = 0; k < 12; ++k) lattice.push_back(lattice[k]);  // duplicates with larger indices
    run("lattice ties", centres, lattice, 0.0);
    run("lattice ties, max 0.5", centres, lattice, 0.5);  // the edge midpoints lie at exactly 0.5: unmatched
    Cloud shifted = lattice, qshift = centres;
    for (size_t k = 0; k < shifted.size(); ++k) shifted[k] += (k % 3 == 0 ? 1e6 : k % 3 == 1 ? -1e6 : 0.5);
    for (size_t k = 0; k < qshift.size(); ++k) qshift[k] += (k % 3 == 0 ? 1e6 : k % 3 == 1 ? -1e6 : 0.5);
    run("lattice shifted", qshift, shifted, 0.0);
    Cloud one;
    for (int k = 0; k < 300; ++k)
        for (double v : {1.25, -2.5, 0.75}) one.push_back(v);
    run("300 copies", box(500, -5.0, 5.0), one, 0.0);
    Cloud line, diag, plane;
    for (int k = 0; k < 400; ++k) {
        const double s = uni(rng) * 10.0;
        for (double v : {s, 2.0, -1.0}) line.push_back(v);
        for (double v : {s, s, s}) diag.push_back(v);
        for (double v : {uni(rng) * 10.0, uni(rng) * 10.0, 3.0}) plane.push_back(v);
    }
    run("line", box(1000, -3.0, 13.0), line, 0.0);
    run("diagonal", box(1000, -3.0, 13.0), diag, 0.0);
    run("plane", box(1000, -3.0, 13.0), plane, 0.0);
    Cloud two = box(200, 0.0, 1.0), other = box(200, 1e4, 1e4 + 1.0);
    two.insert(two.end(), other.begin(), other.end());
    Cloud mid = box(200, 4999.0, 5002.0), in_a = box(200, -1.0, 2.0);
    mid.insert(mid.end(), in_a.begin(), in_a.end());
    run("two clusters", mid, two, 0.0);
    run("far queries", box(500, 1000.0, 1001.0), box(600, 0.0, 1.0), 0.0);
    Cloud outlier = box(600, 0.0, 10.0);
    for (double v : {1e12, -1e12, 1e12}) outlier.push_back(v);
    run("outlier at 1e12", box(500, -2.0, 12.0), outlier, 0.0);
    run("huge coordinates", box(300, -1e308, 1e308), box(300, -1e308, 1e308), 0.0);
    run("tiny extent", box(300, 0.0, 1e-300), box(300, 0.0, 1e-300), 0.0);
    printf(g_fail ? "FAILED\n" : "ok\n");
    return g_fail ? 1 : 0;
}
