// emi_plan_route.hpp -- the arithmetic of emi_plan_route (include/emi355x.h), one text for the host function (emi_host.cpp) and for
// the kernels of emi_start_guess_dev (emi_start_guess.hip): the box and the grid, clearance / cell cost / blocked bits of a cell, the
// predecessor rule of the backtrack, the smoothing and arc length of a path, the resampling at a node.  How the distances are
// reached is NOT here: Dijkstra on the host, a relaxation to the fixed point on the device -- the header of emi355x.h says why
// both give the same bits.  Every function keeps contraction off: single rounded operations, nothing fused.
#pragma once
#include <cmath>

#include "emi355x.h"

#if defined(__HIPCC__)
#define EMI_PLAN_HD __host__ __device__ inline
#else
#define EMI_PLAN_HD inline
#endif
#if defined(__clang__)
#define EMI_PLAN_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define EMI_PLAN_NO_CONTRACT        // g++: built with -ffp-contract=off (Makefile)
#endif

namespace emi_plan {

constexpr int GRID_DEFAULT = 161, GRID_MIN = 9, GRID_MAX = 161, LEVELS = 3;
constexpr double UNREACHED = HUGE_VAL;

EMI_PLAN_HD double grow_of(int level) { return level == 0 ? 0.25 : level == 1 ? 0.1 : 0.0; }

// the box, the grid and the cells of the two end points; level -2 where there is nothing to plan on
struct Geom {
    double x0, y0, x1, y1, xl, yl, hx, hy, sd, span, room;
    int N, start, goal, level;       // level: 0 so far, or -2
};

EMI_PLAN_HD int cell_index(double v, double lo, double h, int N) {
    EMI_PLAN_NO_CONTRACT
    const double q = floor((v - lo) / h + 0.5);
    if (!(q > 0.0)) return 0;
    if (q > (double)(N - 1)) return N - 1;
    return (int)q;
}

EMI_PLAN_HD Geom geom(const double* ends, const double* box, double clearance, int N) {
    EMI_PLAN_NO_CONTRACT
    Geom g;
    g.N = N; g.level = 0; g.start = g.goal = 0;
    g.x0 = ends[0]; g.y0 = ends[1]; g.x1 = ends[2]; g.y1 = ends[3];
    const double ax = fabs(g.x1 - g.x0), ay = fabs(g.y1 - g.y0);
    g.span = ax > ay ? ax : ay;
    g.room = clearance * g.span;
    double xl = box ? box[0] : -HUGE_VAL, xu = box ? box[1] : HUGE_VAL, yl = box ? box[2] : -HUGE_VAL, yu = box ? box[3] : HUGE_VAL;
    if (!(xl > -1e18) || !(xu < 1e18)) { xl = (g.x0 < g.x1 ? g.x0 : g.x1) - g.span; xu = (g.x0 < g.x1 ? g.x1 : g.x0) + g.span; }
    if (!(yl > -1e18) || !(yu < 1e18)) { yl = (g.y0 < g.y1 ? g.y0 : g.y1) - g.span; yu = (g.y0 < g.y1 ? g.y1 : g.y0) + g.span; }
    g.xl = xl; g.yl = yl;
    g.hx = (xu - xl) / (double)(N - 1);
    g.hy = (yu - yl) / (double)(N - 1);
    g.sd = sqrt(g.hx * g.hx + g.hy * g.hy);
    if (!(g.span > 0.0) || !(g.hx > 0.0) || !(g.hy > 0.0)) { g.level = -2; return g; }
    g.start = cell_index(g.x0, xl, g.hx, N) * N + cell_index(g.y0, yl, g.hy, N);
    g.goal = cell_index(g.x1, xl, g.hx, N) * N + cell_index(g.y1, yl, g.hy, N);
    return g;
}

// a record the planner goes round: an ellipse or a disc with positive squares (tracks move and are left to the repair)
EMI_PLAN_HD bool static_record(const double* r, double* xc, double* yc, double* ct, double* st, double* asq, double* bsq) {
    const int kind = (int)r[0];
    if (kind == EMI_PATH_ELLIPSE) { *xc = r[1]; *yc = r[2]; *ct = r[3]; *st = r[4]; *asq = r[5]; *bsq = r[6]; }
    else if (kind == EMI_PATH_DISC) { *xc = r[1]; *yc = r[2]; *ct = 1.0; *st = 0.0; *asq = *bsq = r[3]; }
    else return false;
    return *asq > 0.0 && *bsq > 0.0;
}

EMI_PLAN_HD int count_static(int np, const double* recs) {
    int n = 0;
    double xc, yc, ct, st, asq, bsq;
    for (int j = 0; j < np; ++j) n += static_record(recs + (size_t)j * EMI_PATH_REC, &xc, &yc, &ct, &st, &asq, &bsq) ? 1 : 0;
    return n;
}

// cell cost and the blocked bits (bit l: blocked at grow_of(l)) of cell (i, j)
EMI_PLAN_HD void cell_eval(const Geom& g, int np, const double* recs, int i, int j, double* cost, unsigned char* bits) {
    EMI_PLAN_NO_CONTRACT
    const double x = g.xl + (double)i * g.hx, y = g.yl + (double)j * g.hy;
    double clear = 1e300;
    unsigned char blocked = 0;
    for (int q = 0; q < np; ++q) {
        double xc, yc, ct, st, asq, bsq;
        if (!static_record(recs + (size_t)q * EMI_PATH_REC, &xc, &yc, &ct, &st, &asq, &bsq)) continue;
        const double rmin = sqrt(asq < bsq ? asq : bsq);
        const double dx = x - xc, dy = y - yc;
        const double ex = ct * dx - st * dy, ey = st * dx + ct * dy;
        const double c = (sqrt(ex * ex / asq + ey * ey / bsq) - 1.0) * rmin;
        if (c < clear) clear = c;
        for (int l = 0; l < LEVELS; ++l) {
            const double G = (1.0 + grow_of(l)) * (1.0 + grow_of(l));
            if (ex * ex / (asq * G) + ey * ey / (bsq * G) < 1.0) blocked |= (unsigned char)(1u << l);
        }
    }
    const double lo = 1e-3 * g.span, cl = clear > lo ? clear : lo;
    *cost = 1.0 + (g.room > 0.0 ? (g.room / cl) * (g.room / cl) : 0.0);
    *bits = blocked;
}

EMI_PLAN_HD bool is_blocked(const Geom& g, const unsigned char* bits, int c, int level) {
    return ((bits[c] >> level) & 1) && c != g.start && c != g.goal;
}

EMI_PLAN_HD double step_of(const Geom& g, int di, int dj) { return di == 0 ? g.hy : dj == 0 ? g.hx : g.sd; }

// the least fl(dist[a] + w(a -> c)) over the neighbours a of the unblocked cell c = (i, j), and dist[c] itself
EMI_PLAN_HD double relaxed(const Geom& g, const double* dist, double costc, int i, int j) {
    EMI_PLAN_NO_CONTRACT
    const int N = g.N;
    double best = dist[i * N + j];
    for (int di = -1; di <= 1; ++di)
        for (int dj = -1; dj <= 1; ++dj) {
            const int a = i + di, b = j + dj;
            if ((!di && !dj) || a < 0 || b < 0 || a >= N || b >= N) continue;
            const double w = step_of(g, di, dj) * costc;
            const double d = dist[a * N + b] + w;
            if (d < best) best = d;
        }
    return best;
}

// the predecessor of c on the backtrack: the first neighbour whose distance plus the step into c is dist[c]; -1: none
EMI_PLAN_HD int predecessor(const Geom& g, const double* dist, const double* cost, int c) {
    EMI_PLAN_NO_CONTRACT
    const int N = g.N, i = c / N, j = c % N;
    for (int di = -1; di <= 1; ++di)
        for (int dj = -1; dj <= 1; ++dj) {
            const int a = i + di, b = j + dj;
            if ((!di && !dj) || a < 0 || b < 0 || a >= N || b >= N) continue;
            const double w = step_of(g, di, dj) * cost[c];
            if (dist[a * N + b] + w == dist[c]) return a * N + b;
        }
    return -1;
}

// The route of finite distance dist[goal] as points: backtrack into cells[] (room for N^2; start first on return), the points with the
// true end points at both ends, three in-place smoothing passes, the arc length prefix.  Returns the number of points L, or 0 where
// there is no usable route (a backtrack beyond N^2 cells or into a cell without predecessor, fewer than 2 points, no length).
// px, py, arc: room for N^2 each.  They may lie over dist and cost (the kernel's do): the backtrack, the only reader of those two, is
// complete before the first point is written.
EMI_PLAN_HD int trace(const Geom& g, const double* dist, const double* cost, int* cells, double* px, double* py, double* arc) {
    EMI_PLAN_NO_CONTRACT
    const int N = g.N, cap = N * N;
    int L = 0;
    for (int c = g.goal;; ) {
        if (L == cap) return 0;
        cells[L++] = c;
        if (c == g.start) break;
        c = predecessor(g, dist, cost, c);
        if (c < 0) return 0;
    }
    for (int a = 0, b = L - 1; a < b; ++a, --b) { const int t = cells[a]; cells[a] = cells[b]; cells[b] = t; }
    if (L < 2) return 0;
    for (int n = 0; n < L; ++n) {
        px[n] = g.xl + (double)(cells[n] / N) * g.hx;
        py[n] = g.yl + (double)(cells[n] % N) * g.hy;
    }
    px[0] = g.x0; py[0] = g.y0; px[L - 1] = g.x1; py[L - 1] = g.y1;
    for (int pass = 0; pass < 3; ++pass)
        for (int n = 1; n + 1 < L; ++n) {
            px[n] = 0.25 * px[n - 1] + 0.5 * px[n] + 0.25 * px[n + 1];
            py[n] = 0.25 * py[n - 1] + 0.5 * py[n] + 0.25 * py[n + 1];
        }
    arc[0] = 0.0;
    for (int n = 1; n < L; ++n) {
        const double dx = px[n] - px[n - 1], dy = py[n] - py[n - 1];
        arc[n] = arc[n - 1] + sqrt(dx * dx + dy * dy);
    }
    return arc[L - 1] > 0.0 ? L : 0;
}

// the point of the path at the node abscissa tau: arc length 0.5 (tau + 1) arc[L - 1]
EMI_PLAN_HD void resample(int L, const double* px, const double* py, const double* arc, double tau, double* x, double* y) {
    EMI_PLAN_NO_CONTRACT
    const double s = 0.5 * (tau + 1.0) * arc[L - 1];
    // the first segment with arc[seg + 1] >= s, the last one if there is none (arc never decreases: bisection finds what the host's scan does)
    int lo = 0, hi = L - 2;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (arc[mid + 1] < s) lo = mid + 1; else hi = mid;
    }
    const int seg = lo;
    double w = arc[seg + 1] > arc[seg] ? (s - arc[seg]) / (arc[seg + 1] - arc[seg]) : 0.0;
    w = w > 0.0 ? w : 0.0;          // min(1, max(0, w)) in std::'s order of arguments
    w = w < 1.0 ? w : 1.0;
    *x = px[seg] + w * (px[seg + 1] - px[seg]);
    *y = py[seg] + w * (py[seg + 1] - py[seg]);
}

// the straight line of a state and the bend of the position rows (mi355x::initial_guess)
EMI_PLAN_HD double line_at(double a, double b, double tau) {
    EMI_PLAN_NO_CONTRACT
    return a + (b - a) * 0.5 * (tau + 1.0);
}
// (lx, ly) the line's point at this node, (dx, dy) its end-to-end vector, s the sine of the node; box NULL: no clip
EMI_PLAN_HD void bend_at(double lx, double ly, double dx, double dy, double bend, double s, const double* box, double* x, double* y) {
    EMI_PLAN_NO_CONTRACT
    const double len = sqrt(dx * dx + dy * dy);
    *x = lx; *y = ly;
    if (!(len > 0.0)) return;
    double xv = lx - bend * dy / len * s, yv = ly + bend * dx / len * s;
    if (box) {      // std::min(std::max(v, lower), upper)
        xv = xv < box[0] ? box[0] : xv; xv = box[1] < xv ? box[1] : xv;
        yv = yv < box[2] ? box[2] : yv; yv = box[3] < yv ? box[3] : yv;
    }
    *x = xv; *y = yv;
}

}  // namespace emi_plan
