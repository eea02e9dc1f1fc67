// emi_start_guess.hip -- the starts of a context's whole batch (emi_start_guess_dev): the straight line of every state, the bent
// line and the route planned past the static keep-outs for the two position states.  The arithmetic is emi_plan_route.hpp's, the
// text the host function emi_plan_route is made of, so the bits are that function's.
//
//   emi_start_line_kernel   one thread per (instance, node): the line of every state; for EMI_START_BEND the bend of rows px, py;
//                           level -2 for the kinds that plan nothing.
//   emi_plan_grid_kernel    one thread per (instance, cell): loops over the instance's records (wave-uniform loads) and writes the
//                           cell cost and one byte with the three blocked bits.
//   emi_plan_route_kernel   one workgroup per instance, the three grows one after the other until one has a route (what the host
//                           does; most instances stop at the first).  Relaxation: every thread takes the cells tid, tid + T, ..
//                           and lowers dist[c] to the least fl(dist[a] + w) over its neighbours, in place, sweep after sweep until
//                           a sweep lowers nothing.  No atomics: a distance is one 8-byte load or store, values only fall, each is
//                           the cost of a real path, and a sweep without a store has read a consistent state -- the fixed point.
//                           The distances stay in the context's workspace: 161^2 doubles are 207 KB against 160 KB of LDS, and a
//                           tiled form would need a halo exchange per sweep through the same memory; one instance's 207 KB sit in
//                           the L2 of the XCD its workgroup runs on.  One barrier per sweep: the changed flag rotates over three
//                           LDS words (the one written in sweep s is cleared in sweep s - 1, two barriers after its last reader),
//                           every thread reads it after the barrier, so the exit is uniform.  Sweeps are capped at grid^2 (level
//                           -1; in theory never reached).  (Relaxing 8 cells per round, all loads ahead of the stores, was slower:
//                           23.9 against 21.4 ms for 64 instances -- what a store within a sweep hands to the next cell is lost.)
//                           Then one lane backtracks, smooths and sums the arc length in the
//                           host's order -- sequential recurrences on a few hundred points, over the arrays the relaxation is done
//                           with -- and all threads resample at the nodes.  Instances without a route take the bend where one is
//                           asked for.
// Contraction is off in all of it (emi_plan_route.hpp).
#include <hip/hip_runtime.h>

#include <vector>

#include "emi_ctx.hpp"
#include "emi_plan_route.hpp"

namespace emi {
namespace {

namespace P = emi_plan;

constexpr int LINE_T = 256;         // nodes per block
constexpr int GRID_T = 256;         // cells per block
constexpr int ROUTE_T = 1024;       // threads of an instance's workgroup

// the parameters of instance b: xa [ns] | xb [ns] | box [4]
__device__ inline const double* params_of(const StartArgs& a, int b) { return a.par + (size_t)(a.nsets > 1 ? b : 0) * (2 * a.ns + 4); }
__device__ inline const double* box_of(const StartArgs& a, const double* par) { return a.has_box ? par + 2 * a.ns : nullptr; }
__device__ inline void ends_of(const StartArgs& a, const double* par, double* ends) {
    ends[0] = par[a.px]; ends[1] = par[a.py]; ends[2] = par[a.ns + a.px]; ends[3] = par[a.ns + a.py];
}

// rows px, py of node k bent: the line's point, its end-to-end vector from the line at the first and the last node
__device__ inline void bend_node(const StartArgs& a, const double* par, int b, int k) {
    const double ax = par[a.px], bx = par[a.ns + a.px], ay = par[a.py], by = par[a.ns + a.py];
    const double dx = P::line_at(ax, bx, a.tau[a.M - 1]) - P::line_at(ax, bx, a.tau[0]);
    const double dy = P::line_at(ay, by, a.tau[a.M - 1]) - P::line_at(ay, by, a.tau[0]);
    double x, y;
    P::bend_at(P::line_at(ax, bx, a.tau[k]), P::line_at(ay, by, a.tau[k]), dx, dy, a.bend, a.sine[k], box_of(a, par), &x, &y);
    a.X[((size_t)b * a.ns + a.px) * a.M + k] = x;
    a.X[((size_t)b * a.ns + a.py) * a.M + k] = y;
}

__global__ __launch_bounds__(LINE_T) void emi_start_line_kernel(StartArgs a) {
    const int k = blockIdx.x * LINE_T + threadIdx.x, b = blockIdx.y;
    if (k >= a.M) return;
    const double* par = params_of(a, b);
    const double tau = a.tau[k];
    for (int i = 0; i < a.ns; ++i) a.X[((size_t)b * a.ns + i) * a.M + k] = P::line_at(par[i], par[a.ns + i], tau);
    if (a.kind == EMI_START_BEND) bend_node(a, par, b, k);
    if (k == 0 && a.level && a.kind != EMI_START_PLANNED) a.level[b] = -2;
}

__global__ __launch_bounds__(GRID_T) void emi_plan_grid_kernel(StartArgs a) {
    const int c = blockIdx.x * GRID_T + threadIdx.x, b = blockIdx.y, n2 = a.N * a.N;
    if (c >= n2) return;
    const double* par = params_of(a, b);
    double ends[4];
    ends_of(a, par, ends);
    const P::Geom g = P::geom(ends, box_of(a, par), a.clearance, a.N);
    if (g.level == -2) return;
    const double* recs = a.recs + (size_t)(a.path_sets > 1 ? b : 0) * a.np * EMI_PATH_REC;
    double cost;
    unsigned char bits;
    P::cell_eval(g, a.np, recs, c / a.N, c % a.N, &cost, &bits);
    a.cost[(size_t)b * n2 + c] = cost;
    a.bits[(size_t)b * n2 + c] = bits;
}

__global__ __launch_bounds__(ROUTE_T) void emi_plan_route_kernel(StartArgs a) {
    __shared__ int changed[3];
    __shared__ int points;
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N, n2 = N * N;
    const double* par = params_of(a, b);
    const double* recs = a.recs + (size_t)(a.path_sets > 1 ? b : 0) * a.np * EMI_PATH_REC;
    double ends[4];
    ends_of(a, par, ends);
    const P::Geom g = P::geom(ends, box_of(a, par), a.clearance, N);
    double* cost = a.cost + (size_t)b * n2;
    double* dist = a.dist + (size_t)b * n2;
    double* extra = a.extra + (size_t)b * n2;
    int* cells = a.cells + (size_t)b * n2;
    const unsigned char* bits = a.bits + (size_t)b * n2;
    // everything that decides a branch around a barrier below is the same in every thread: g, the record count, the sweep counter,
    // the flags and dist[goal] as read after a barrier
    int level = (g.level == -2 || P::count_static(a.np, recs) == 0) ? -2 : -1;
    for (int lv = 0; level == -1 && lv < P::LEVELS; ++lv) {
        for (int c = tid; c < n2; c += ROUTE_T) dist[c] = c == g.start ? 0.0 : P::UNREACHED;
        if (tid < 3) changed[tid] = 0;
        __syncthreads();
        bool capped = false;
        for (int sweep = 0;; ++sweep) {
            if (sweep == n2) { capped = true; break; }
            if (tid == 0) changed[(sweep + 1) % 3] = 0;
            bool lowered = false;
            for (int c = tid; c < n2; c += ROUTE_T) {
                if (P::is_blocked(g, bits, c, lv)) continue;
                const double old = dist[c], best = P::relaxed(g, dist, cost[c], c / N, c % N);
                if (best < old) { dist[c] = best; lowered = true; }
            }
            if (lowered) changed[sweep % 3] = 1;
            __syncthreads();
            if (!changed[sweep % 3]) break;
        }
        if (capped) break;
        const bool reached = dist[g.goal] < P::UNREACHED;
        __syncthreads();                // dist[goal] is read by all before the next grow resets it
        if (!reached) continue;
        // cost becomes the abscissae of the path, dist its arc length: the backtrack has read both before the first is written
        if (tid == 0) points = P::trace(g, dist, cost, cells, cost, extra, dist);
        __syncthreads();
        const int L = points;
        if (L == 0) break;
        for (int k = tid; k < a.M; k += ROUTE_T) {
            double x, y;
            P::resample(L, cost, extra, dist, a.tau[k], &x, &y);
            a.X[((size_t)b * a.ns + a.px) * a.M + k] = x;
            a.X[((size_t)b * a.ns + a.py) * a.M + k] = y;
        }
        level = lv;
    }
    if (level < 0 && a.bend != 0.0)
        for (int k = tid; k < a.M; k += ROUTE_T) bend_node(a, par, b, k);
    if (tid == 0 && a.level) a.level[b] = level;
}

}  // namespace

// the arrays of emi_start_guess_dev: what went up with the call (per set xa | xb | box, then the node abscissae and the sines of the
// bend) and, per instance, grid^2 cell costs, distances, one more array of that size for the path, the cells of the backtrack and
// the blocked bits
struct StartGuessWs {
    DevBuf par;
    // the host side of `par`: page-locked, so that the copy is asynchronous on the context's stream as the header promises, and an
    // event recorded behind that copy -- the next call fills par_h only once the copy of this one has read it
    PinnedArray<double> par_h;
    hipEvent_t par_up = nullptr;
    DeviceArray<double> cost, dist, extra;
    DeviceArray<int> cells;
    DeviceArray<unsigned char> bits;
};

void start_guess_destroy(StartGuessWs* w) {
    if (w && w->par_up) (void)hipEventDestroy(w->par_up);
    delete w;
}

int start_guess(emi_ctx_t c, const emi_start_t& st, void* dX, void* dLevel) {
    const char* who = "emi_start_guess_dev";
    if (!c->start_guess) c->start_guess = new StartGuessWs;
    StartGuessWs& w = *c->start_guess;
    const int ns = c->ns, M = c->M, B = c->B, N = st.grid == 0 ? P::GRID_DEFAULT : st.grid;
    const bool planned = st.kind == EMI_START_PLANNED;
    // what goes up: a few doubles per set, and the mesh's abscissae with the sines of the bend (the host's sin: one table for both forms)
    const size_t per = (size_t)2 * ns + 4;
    const size_t nh = per * st.nsets + 2 * (size_t)M;
    if (!w.par_up) HIP_TRY_AS(c, who, hipEventCreateWithFlags(&w.par_up, hipEventDisableTiming));
    HIP_TRY_AS(c, who, hipEventSynchronize(w.par_up));          // (an event that was never recorded is complete)
    HIP_TRY_AS(c, who, w.par_h.reserve(nh));
    EMI_TRY(emi_api::ensure(c, w.par, nh * 8));
    double* h = w.par_h.p;
    std::fill(h, h + nh, 0.0);
    for (int s = 0; s < st.nsets; ++s) {
        std::copy(st.xa + (size_t)s * ns, st.xa + (size_t)(s + 1) * ns, h + s * per);
        std::copy(st.xb + (size_t)s * ns, st.xb + (size_t)(s + 1) * ns, h + s * per + ns);
        if (st.box) std::copy(st.box + (size_t)s * 4, st.box + (size_t)(s + 1) * 4, h + s * per + 2 * ns);
    }
    double* tau = h + per * st.nsets;
    for (int k = 0; k < M; ++k) { tau[k] = c->h_tau[k]; tau[M + k] = std::sin(1.5707963267948966 * (c->h_tau[k] + 1.0)); }
    HIP_TRY_AS(c, who, hipMemcpyAsync(w.par.p, h, nh * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY_AS(c, who, hipEventRecord(w.par_up, c->stream));
    StartArgs a{};
    a.X = (double*)dX; a.level = (int*)dLevel;
    a.recs = (const double*)c->d_path.p;
    a.par = (const double*)w.par.p; a.tau = a.par + per * st.nsets; a.sine = a.tau + M;
    a.B = B; a.ns = ns; a.M = M; a.np = c->np; a.path_sets = c->path_sets; a.px = c->px; a.py = c->py;
    a.nsets = st.nsets; a.kind = st.kind; a.N = N; a.has_box = st.box ? 1 : 0;
    a.bend = st.bend; a.clearance = st.clearance;
    hipLaunchKernelGGL(emi_start_line_kernel, dim3((M + LINE_T - 1) / LINE_T, B), dim3(LINE_T), 0, c->stream, a);
    HIP_TRY_AS(c, who, hipGetLastError());
    if (!planned) return EMI_OK;
    const size_t n2 = (size_t)N * N, cells = n2 * B;
    HIP_TRY_AS(c, who, w.cost.reserve(cells));
    HIP_TRY_AS(c, who, w.dist.reserve(cells));
    HIP_TRY_AS(c, who, w.extra.reserve(cells));
    HIP_TRY_AS(c, who, w.cells.reserve(cells));
    HIP_TRY_AS(c, who, w.bits.reserve(cells));
    a.cost = w.cost.p; a.dist = w.dist.p; a.extra = w.extra.p; a.cells = w.cells.p; a.bits = w.bits.p;
    hipLaunchKernelGGL(emi_plan_grid_kernel, dim3(((int)n2 + GRID_T - 1) / GRID_T, B), dim3(GRID_T), 0, c->stream, a);
    HIP_TRY_AS(c, who, hipGetLastError());
    hipLaunchKernelGGL(emi_plan_route_kernel, dim3(B), dim3(ROUTE_T), 0, c->stream, a);
    HIP_TRY_AS(c, who, hipGetLastError());
    return EMI_OK;
}

}  // namespace emi
