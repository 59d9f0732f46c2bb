// Host build of csrc/ot_spline.hpp, path against path (tests/test_spline_host.py writes the tables and points):
//   * the cached path with arithmetic knot cells (what the trace kernel runs), the table path (FITPACK's order on the stored
//     knots) and the leaf path (arithmetic cells, no cache) against a long double de Boor sum with analytic derivatives,
//     within the bars of tests/spline_cases.py: V = K u A0 + (|S_x| + |S_y|) delta, G = K u A{x,y} + h2 delta
//   * the cache protocol: cell A, its neighbour B, A again through one cache gives the bits of three fresh caches
//   * when spl2_grad_cached / spl1_grad_cached apply: if and only if the cached key is the point's cell and that cell lies
//     in the equidistant part; never after an evaluation in the neighbouring cell, for a NaN or with an empty cache
//   * clamping: arguments at and beyond the knot range; every index any path forms is checked against its array
// usage: spline_paths_test FILE.  FILE: float64 words -- number of tables, then per table: kind (1, 2), n, table length,
// delta, h2, number of points, the table (layout: include/optrace_amd.h), the points (x y pairs; 1-D: y unused).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#define OT_HD
#define OT_SPL_K 4
static long g_bad_index = 0;

// a pointer that checks every index formed through it against its array
struct Chk {
    const double* base;
    long off, len;
    double operator[](long i) const {
        const long j = off + i;
        if (j < 0 || j >= len) {
            g_bad_index++;
            return 0.0;
        }
        return base[j];
    }
    Chk operator+(long d) const { return Chk{base, off + d, len}; }
    explicit operator const double*() const { return base + off; }
};

#include "ot_spline.hpp"

static_assert(LDBL_MANT_DIG >= 64, "the truth of this test needs a 64-bit mantissa");
typedef long double LD;
static const int K = OT_SPL_K, K1 = K + 1;
static const double KU = 32 * 0x1p-53;
static int g_fail = 0;

#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (g_fail < 20) {            \
                std::printf("FAIL: ");    \
                std::printf(__VA_ARGS__); \
                std::printf("\n");        \
            }                             \
            g_fail++;                     \
        }                                 \
    } while (0)

struct Table {
    int kind, n, nc;
    double delta, h2, inv_h;
    std::vector<double> tab, pts;
    UniformKnots uk;
    const double* t() const { return tab.data(); }
    Chk T() const { return Chk{tab.data(), 0, n}; }
    Chk C() const { return Chk{tab.data() + n, 0, kind == 1 ? n : nc * nc}; }
    Chk DC() const { return Chk{tab.data() + 2 * n, 0, n}; }
    Chk CX() const { return Chk{tab.data() + n + nc * nc, 0, (nc - 1) * nc}; }
    Chk CY() const { return Chk{tab.data() + n + nc * nc + (nc - 1) * nc, 0, nc * (nc - 1)}; }
    // cell of the stored knots: t[i] <= x < t[i + 1], clamped to [K, n - K - 2]
    int cell(double x) const {
        int i = K;
        while (i < n - K - 2 && x >= t()[i + 1]) i++;
        return i;
    }
    bool arithmetic(int i) const { return i >= uk.ulo + K - 1 && i <= uk.uhi - K; }
    // within a few units of a knot the stored and the arithmetic cell may differ
    bool near_knot(double x) const {
        const int i = cell(x);
        const double tol = 4 * delta + 8 * DBL_EPSILON * std::fabs(x);
        return std::fabs(x - t()[i]) <= tol || std::fabs(x - t()[i + 1]) <= tol;
    }
};

// the K + 1 B-splines on cell i and their derivatives, Cox-de Boor in long double
static void basis(const Table& tb, LD x, int i, LD* h, LD* d) {
    const double* t = tb.t();
    LD hh[K1], h3[K1] = {0};
    h[0] = 1;
    for (int j = 1; j <= K; j++) {
        for (int q = 0; q < j; q++) hh[q] = h[q];
        for (int q = 0; q <= j; q++) h[q] = 0;
        for (int q = 0; q < j; q++) {
            const LD tli = t[i + q + 1], tlj = t[i + q + 1 - j];
            const LD f = hh[q] / (tli - tlj);
            h[q] += f * (tli - x);
            h[q + 1] = f * (x - tlj);
        }
        if (j == K - 1)
            for (int q = 0; q < K; q++) h3[q] = h[q];
    }
    for (int m = 0; m <= K; m++) {
        const LD a = m >= 1 ? h3[m - 1] / ((LD)t[i + m] - (LD)t[i + m - K]) : 0;
        const LD b = m <= K - 1 ? h3[m] / ((LD)t[i + m + 1] - (LD)t[i + m + 1 - K]) : 0;
        d[m] = K * (a - b);
    }
}

struct Truth {
    LD S, Sx, Sy, A0, Ax, Ay;
};

static Truth truth2(const Table& tb, double x, double y) {
    const double lo = tb.t()[K], hi = tb.t()[tb.nc];
    x = x < lo ? lo : (x > hi ? hi : x);
    y = y < lo ? lo : (y > hi ? hi : y);
    const int ix = tb.cell(x), iy = tb.cell(y);
    LD hx[K1], dx[K1], hy[K1], dy[K1];
    basis(tb, x, ix, hx, dx);
    basis(tb, y, iy, hy, dy);
    Truth r = {0, 0, 0, 0, 0, 0};
    const double* c = tb.tab.data() + tb.n;
    for (int a = 0; a <= K; a++)
        for (int b = 0; b <= K; b++) {
            const LD cc = c[(ix - K + a) * tb.nc + (iy - K + b)], ac = fabsl(cc);
            r.S += cc * hx[a] * hy[b];
            r.Sx += cc * dx[a] * hy[b];
            r.Sy += cc * hx[a] * dy[b];
            r.A0 += ac * hx[a] * hy[b];
            r.Ax += ac * fabsl(dx[a]) * hy[b];
            r.Ay += ac * hx[a] * fabsl(dy[b]);
        }
    return r;
}

static Truth truth1(const Table& tb, double x) {
    const int i = tb.cell(x);
    LD h[K1], d[K1];
    basis(tb, x, i, h, d);
    Truth r = {0, 0, 0, 0, 0, 0};
    const double* c = tb.tab.data() + tb.n;
    for (int a = 0; a <= K; a++) {
        const LD cc = c[i - K + a];
        r.S += cc * h[a];
        r.Sx += cc * d[a];
        r.A0 += fabsl(cc) * h[a];
        r.Ax += fabsl(cc) * fabsl(d[a]);
    }
    return r;
}

// one lane's patch among four, the others filled with a pattern that must survive
struct Lane {
    static const int STRIDE = 4, MINE = 1;
    double lds[25 * STRIDE];
    PatchCache pc;
    Lane() {
        for (int i = 0; i < 25 * STRIDE; i++) lds[i] = -777.0 - i;
        pc = PatchCache{lds + MINE, STRIDE, nullptr};
    }
    bool others_untouched() const {
        for (int i = 0; i < 25 * STRIDE; i++)
            if (i % STRIDE != MINE && lds[i] != -777.0 - i) return false;
        return true;
    }
};

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

struct Worst {
    double v_cached = 0, v_table = 0, v_leaf = 0, g_cached = 0, g_table = 0;
    long applied = 0, refused = 0, protocol = 0;
};

static void run2(const Table& tb, int ti) {
    const Chk t = tb.T(), c = tb.C();
    const UniformKnots* uk = &tb.uk;
    const int n = tb.n, np = (int)tb.pts.size() / 2;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Worst w;
    for (int p = 0; p < np; p++) {
        const double x = tb.pts[2 * p], y = tb.pts[2 * p + 1];
        const Truth tr = truth2(tb, x, y);
        const LD V = KU * tr.A0 + (fabsl(tr.Sx) + fabsl(tr.Sy)) * tb.delta;
        const LD Gx = KU * tr.Ax + (LD)tb.h2 * tb.delta, Gy = KU * tr.Ay + (LD)tb.h2 * tb.delta;
        Lane a;
        const double vc = spl2_eval<K, K>(t, n, t, n, c, tb.inv_h, x, y, &a.pc, uk);
        const double vt = spl2_eval<K, K>(t, n, t, n, c, tb.inv_h, x, y);
        const double vl = spl2_eval<K, K>(t, n, t, n, c, tb.inv_h, x, y, nullptr, uk);
        w.v_cached = std::fmax(w.v_cached, (double)(fabsl(vc - tr.S) / V));
        w.v_table = std::fmax(w.v_table, (double)(fabsl(vt - tr.S) / V));
        w.v_leaf = std::fmax(w.v_leaf, (double)(fabsl(vl - tr.S) / V));
        CHECK(fabsl(vc - tr.S) <= V && fabsl(vt - tr.S) <= V && fabsl(vl - tr.S) <= V, "table %d point %d (%.17g, %.17g): value off by %.3g %.3g %.3g of V = %.3Lg",
              ti, p, x, y, (double)fabsl(vc - tr.S), (double)fabsl(vt - tr.S), (double)fabsl(vl - tr.S), V);
        // the table gradient (the leaf path and the cached gradient's fallback)
        const double tx = spl2_eval<K - 1, K>(t + 1, n - 2, t, n, tb.CX(), tb.inv_h, x, y);
        const double ty = spl2_eval<K, K - 1>(t, n, t + 1, n - 2, tb.CY(), tb.inv_h, x, y);
        w.g_table = std::fmax(w.g_table, std::fmax((double)(fabsl(tx - tr.Sx) / Gx), (double)(fabsl(ty - tr.Sy) / Gy)));
        CHECK(fabsl(tx - tr.Sx) <= Gx && fabsl(ty - tr.Sy) <= Gy, "table %d point %d: table gradient off by %.3g %.3g of %.3Lg %.3Lg", ti, p,
              (double)fabsl(tx - tr.Sx), (double)fabsl(ty - tr.Sy), Gx, Gy);
        // when the cached gradient applies
        const double lo = tb.uk.lo, hi = tb.uk.hi;
        const double cx = x < lo ? lo : (x > hi ? hi : x), cy = y < lo ? lo : (y > hi ? hi : y);
        int lx, ly;
        double ux, uy;
        const bool fast = uniform_cell<K>(tb.uk, cx, lx, ux) & uniform_cell<K>(tb.uk, cy, ly, uy);
        if (!tb.near_knot(cx) && !tb.near_knot(cy)) {
            const bool stored = tb.arithmetic(tb.cell(cx)) && tb.arithmetic(tb.cell(cy));
            CHECK(stored == fast, "table %d point %d: arithmetic and stored cells disagree on the equidistant part", ti, p);
            if (fast) CHECK(lx - 1 == tb.cell(cx) && ly - 1 == tb.cell(cy), "table %d point %d: arithmetic cell %d %d, stored %d %d", ti, p, lx - 1, ly - 1, tb.cell(cx), tb.cell(cy));
        }
        double sx = nan, sy = nan;
        const bool applied = spl2_grad_cached(t, n, c, tb.inv_h, x, y, &a.pc, sx, sy, uk);
        CHECK(applied == fast, "table %d point %d (%.17g, %.17g): cached gradient %s, cell %s the equidistant part", ti, p, x, y,
              applied ? "applied" : "refused", fast ? "in" : "outside");
        if (applied) {
            w.applied++;
            w.g_cached = std::fmax(w.g_cached, std::fmax((double)(fabsl(sx - tr.Sx) / Gx), (double)(fabsl(sy - tr.Sy) / Gy)));
            CHECK(fabsl(sx - tr.Sx) <= Gx && fabsl(sy - tr.Sy) <= Gy, "table %d point %d: cached gradient off by %.3g %.3g of %.3Lg %.3Lg", ti, p,
                  (double)fabsl(sx - tr.Sx), (double)fabsl(sy - tr.Sy), Gx, Gy);
        } else {
            w.refused++;
        }
        Lane empty;
        CHECK(!spl2_grad_cached(t, n, c, tb.inv_h, x, y, &empty.pc, sx, sy, uk), "table %d point %d: applied with an empty cache", ti, p);
        CHECK(!spl2_grad_cached(t, n, c, tb.inv_h, nan, y, &a.pc, sx, sy, uk) && !spl2_grad_cached(t, n, c, tb.inv_h, x, nan, &a.pc, sx, sy, uk),
              "table %d point %d: applied for a NaN", ti, p);
        // the protocol: A, the neighbouring cell B, A again
        for (int dir = 0; dir < 2; dir++) {
            const double bx = x + (dir == 0 ? tb.uk.h : 0.0), by = y + (dir == 1 ? tb.uk.h : 0.0);
            if (bx > hi || by > hi) continue;
            Lane one, f1, f2, f3;
            const double a1 = spl2_eval<K, K>(t, n, t, n, c, tb.inv_h, x, y, &one.pc, uk);
            const double b1 = spl2_eval<K, K>(t, n, t, n, c, tb.inv_h, bx, by, &one.pc, uk);
            CHECK(!spl2_grad_cached(t, n, c, tb.inv_h, x, y, &one.pc, sx, sy, uk) || one.pc.key == a.pc.key,
                  "table %d point %d: the cached gradient applied after an evaluation in the neighbouring cell", ti, p);
            const double a2 = spl2_eval<K, K>(t, n, t, n, c, tb.inv_h, x, y, &one.pc, uk);
            const bool ok = same_bits(a1, spl2_eval<K, K>(t, n, t, n, c, tb.inv_h, x, y, &f1.pc, uk)) &&
                            same_bits(b1, spl2_eval<K, K>(t, n, t, n, c, tb.inv_h, bx, by, &f2.pc, uk)) &&
                            same_bits(a2, spl2_eval<K, K>(t, n, t, n, c, tb.inv_h, x, y, &f3.pc, uk)) && same_bits(a1, a2);
            CHECK(ok, "table %d point %d: A, B, A through one cache differs from three fresh caches", ti, p);
            CHECK(one.others_untouched(), "table %d point %d: the cache wrote into another lane's entries", ti, p);
            double s2x, s2y, s1x, s1y;
            if (spl2_grad_cached(t, n, c, tb.inv_h, x, y, &one.pc, s2x, s2y, uk) && applied) {
                Lane g;
                (void)spl2_eval<K, K>(t, n, t, n, c, tb.inv_h, x, y, &g.pc, uk);
                (void)spl2_grad_cached(t, n, c, tb.inv_h, x, y, &g.pc, s1x, s1y, uk);
                CHECK(same_bits(s1x, s2x) && same_bits(s1y, s2y), "table %d point %d: gradient after A, B, A differs from a fresh one", ti, p);
            }
            w.protocol++;
        }
    }
    // clamping: at and beyond the range, in every path
    const double lo = tb.uk.lo, hi = tb.uk.hi, inf = std::numeric_limits<double>::infinity();
    const double edge[] = {lo, hi, std::nextafter(lo, -inf), std::nextafter(hi, inf), lo - 1e-10, hi + 1e-10, lo - 1.0, hi + 1.0, -1e300, 1e300, -inf, inf, nan, 0.0};
    for (double x : edge)
        for (double y : edge) {
            Lane a;
            double sx, sy;
            const double vc = spl2_eval<K, K>(t, n, t, n, c, tb.inv_h, x, y, &a.pc, uk);
            const double vt = spl2_eval<K, K>(t, n, t, n, c, tb.inv_h, x, y);
            (void)spl2_grad_cached(t, n, c, tb.inv_h, x, y, &a.pc, sx, sy, uk);
            (void)spl2_eval<K - 1, K>(t + 1, n - 2, t, n, tb.CX(), tb.inv_h, x, y);
            (void)spl2_eval<K, K - 1>(t, n, t + 1, n - 2, tb.CY(), tb.inv_h, x, y);
            if (x == x && y == y) {
                const Truth tr = truth2(tb, x, y);
                const LD V = KU * tr.A0 + (fabsl(tr.Sx) + fabsl(tr.Sy)) * tb.delta;
                CHECK(fabsl(vc - tr.S) <= V && fabsl(vt - tr.S) <= V, "table %d: clamped value at (%g, %g) off", ti, x, y);
            }
            CHECK(a.others_untouched(), "table %d: clamped evaluation wrote into another lane's entries", ti);
        }
    std::printf("table %d (2-D, %d knots, %d points): values cached %.3f table %.3f leaf %.3f of V; gradient cached %.3f (%ld applied, %ld refused) "
                "table %.3f of G; %ld A-B-A sequences\n", ti, n, np, w.v_cached, w.v_table, w.v_leaf, w.g_cached, w.applied, w.refused, w.g_table, w.protocol);
    CHECK(w.applied > 0 && w.refused > 0 && w.protocol > 0, "table %d: the points reach only one side", ti);
}

static void run1(const Table& tb, int ti) {
    const Chk t = tb.T(), c = tb.C();
    const UniformKnots* uk = &tb.uk;
    const int n = tb.n, np = (int)tb.pts.size() / 2;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Worst w;
    for (int p = 0; p < np; p++) {
        const double x = tb.pts[2 * p];
        const Truth tr = truth1(tb, x);
        const LD V = KU * tr.A0 + fabsl(tr.Sx) * tb.delta, G = KU * tr.Ax + (LD)tb.h2 * tb.delta;
        Lane a;
        const double vc = spl1_eval<K>(t, n, c, tb.inv_h, x, uk, &a.pc);
        const double vt = spl1_eval<K>(t, n, c, tb.inv_h, x);
        const double vl = spl1_eval<K>(t, n, c, tb.inv_h, x, uk);
        w.v_cached = std::fmax(w.v_cached, (double)(fabsl(vc - tr.S) / V));
        w.v_table = std::fmax(w.v_table, (double)(fabsl(vt - tr.S) / V));
        w.v_leaf = std::fmax(w.v_leaf, (double)(fabsl(vl - tr.S) / V));
        CHECK(fabsl(vc - tr.S) <= V && fabsl(vt - tr.S) <= V && fabsl(vl - tr.S) <= V, "table %d point %d (%.17g): value off by %.3g %.3g %.3g of V = %.3Lg", ti, p, x,
              (double)fabsl(vc - tr.S), (double)fabsl(vt - tr.S), (double)fabsl(vl - tr.S), V);
        const double dt = spl1_eval<K - 1>(t, n, tb.DC(), tb.inv_h, x, uk);   // as data_gradient calls it
        const double dp = spl1_eval<K - 1>(t, n, tb.DC(), tb.inv_h, x);
        w.g_table = std::fmax(w.g_table, std::fmax((double)(fabsl(dt - tr.Sx) / G), (double)(fabsl(dp - tr.Sx) / G)));
        CHECK(fabsl(dt - tr.Sx) <= G && fabsl(dp - tr.Sx) <= G, "table %d point %d (%.17g): table derivative off by %.3g %.3g of %.3Lg", ti, p, x,
              (double)fabsl(dt - tr.Sx), (double)fabsl(dp - tr.Sx), G);
        int l;
        double u;
        const bool fast = uniform_cell<K>(tb.uk, x, l, u);
        if (!tb.near_knot(x) && x >= tb.uk.lo && x <= tb.uk.hi) {
            CHECK(tb.arithmetic(tb.cell(x)) == fast, "table %d point %d: arithmetic and stored cells disagree on the equidistant part", ti, p);
            if (fast) CHECK(l - 1 == tb.cell(x), "table %d point %d: arithmetic cell %d, stored %d", ti, p, l - 1, tb.cell(x));
        }
        double d = nan;
        const bool applied = spl1_grad_cached(c, x, uk, &a.pc, d);
        CHECK(applied == fast, "table %d point %d (%.17g): cached derivative %s, cell %s the equidistant part", ti, p, x, applied ? "applied" : "refused",
              fast ? "in" : "outside");
        if (applied) {
            w.applied++;
            w.g_cached = std::fmax(w.g_cached, (double)(fabsl(d - tr.Sx) / G));
            CHECK(fabsl(d - tr.Sx) <= G, "table %d point %d (%.17g): cached derivative off by %.3g of %.3Lg", ti, p, x, (double)fabsl(d - tr.Sx), G);
        } else {
            w.refused++;
        }
        Lane empty;
        CHECK(!spl1_grad_cached(c, x, uk, &empty.pc, d), "table %d point %d: applied with an empty cache", ti, p);
        CHECK(!spl1_grad_cached(c, nan, uk, &a.pc, d), "table %d point %d: applied for a NaN", ti, p);
        const double bx = x + tb.uk.h;
        if (bx <= tb.uk.hi) {
            Lane one, f1, f2, f3;
            const double a1 = spl1_eval<K>(t, n, c, tb.inv_h, x, uk, &one.pc);
            const double b1 = spl1_eval<K>(t, n, c, tb.inv_h, bx, uk, &one.pc);
            CHECK(!spl1_grad_cached(c, x, uk, &one.pc, d) || one.pc.key == a.pc.key, "table %d point %d: the cached derivative applied after an evaluation in the neighbouring cell", ti, p);
            const double a2 = spl1_eval<K>(t, n, c, tb.inv_h, x, uk, &one.pc);
            const bool ok = same_bits(a1, spl1_eval<K>(t, n, c, tb.inv_h, x, uk, &f1.pc)) && same_bits(b1, spl1_eval<K>(t, n, c, tb.inv_h, bx, uk, &f2.pc)) &&
                            same_bits(a2, spl1_eval<K>(t, n, c, tb.inv_h, x, uk, &f3.pc)) && same_bits(a1, a2);
            CHECK(ok, "table %d point %d: A, B, A through one cache differs from three fresh caches", ti, p);
            CHECK(one.others_untouched(), "table %d point %d: the cache wrote into another lane's entries", ti, p);
            w.protocol++;
        }
    }
    // beyond the knots the end polynomial is continued (ext = 0); the kernel's arguments stay within N_EPS of the range
    const double edge[] = {tb.uk.lo, tb.uk.hi, tb.uk.hi + 1e-10, tb.uk.hi + 1e-9, tb.uk.lo - 1e-9, 0.0, nan};
    for (double x : edge) {
        Lane a;
        double d;
        const double vc = spl1_eval<K>(t, n, c, tb.inv_h, x, uk, &a.pc);
        const double vt = spl1_eval<K>(t, n, c, tb.inv_h, x);
        (void)spl1_grad_cached(c, x, uk, &a.pc, d);
        (void)spl1_eval<K - 1>(t, n, tb.DC(), tb.inv_h, x, uk);
        if (x == x) {
            const Truth tr = truth1(tb, x);
            const LD V = KU * tr.A0 + fabsl(tr.Sx) * tb.delta;
            CHECK(fabsl(vc - tr.S) <= V && fabsl(vt - tr.S) <= V, "table %d: value at the end %g off", ti, x);
        }
        CHECK(a.others_untouched(), "table %d: evaluation at the end wrote into another lane's entries", ti);
    }
    std::printf("table %d (1-D, %d knots, %d points): values cached %.3f table %.3f leaf %.3f of V; derivative cached %.3f (%ld applied, %ld refused) "
                "table %.3f of G; %ld A-B-A sequences\n", ti, n, np, w.v_cached, w.v_table, w.v_leaf, w.g_cached, w.applied, w.refused, w.g_table, w.protocol);
    CHECK(w.applied > 0 && w.refused > 0 && w.protocol > 0, "table %d: the points reach only one side", ti);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<double> w;
    double buf[4096];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), 4096, f)) > 0) w.insert(w.end(), buf, buf + got);
    std::fclose(f);
    size_t at = 0;
    const int ntab = (int)w[at++];
    for (int ti = 0; ti < ntab; ti++) {
        Table tb;
        tb.kind = (int)w[at++];
        tb.n = (int)w[at++];
        const long len = (long)w[at++];
        tb.delta = w[at++];
        tb.h2 = w[at++];
        const long np = (long)w[at++];
        tb.nc = tb.n - K1;
        tb.tab.assign(w.begin() + at, w.begin() + at + len);
        at += len;
        tb.pts.assign(w.begin() + at, w.begin() + at + 2 * np);
        at += 2 * np;
        if (len != (tb.kind == 1 ? 3L * tb.n : (long)tb.n + (long)tb.nc * tb.nc + 2L * (tb.nc - 1) * tb.nc)) return 2;
        // the equidistant part as compile_surface (csrc/ot_scene_api.hip) describes it
        const double* t = tb.t();
        const int ulo = K + 1, uhi = tb.n - K - 2;
        const double span = t[tb.nc] - t[K];
        tb.inv_h = (double)(tb.nc - K - 1 > 0 ? tb.nc - K - 1 : 1) / span;
        const double h = (t[uhi] - t[ulo]) / (double)(uhi - ulo);
        bool uniform = uhi - ulo >= 2 * K && h > 0.0;
        for (int i = ulo; i <= uhi && uniform; i++) uniform = std::fabs(t[i] - (t[ulo] + (i - ulo) * h)) <= 1e-9 * h;
        if (!uniform) {
            std::printf("table %d has no equidistant part\n", ti);
            return 1;
        }
        tb.uk = UniformKnots{t[ulo], h, 1.0 / h, t[K], t[tb.nc], ulo, uhi};
        if (tb.kind == 1)
            run1(tb, ti);
        else
            run2(tb, ti);
    }
    CHECK(g_bad_index == 0, "%ld indices outside their array", g_bad_index);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ok %d tables\n", ntab);
    return 0;
}
