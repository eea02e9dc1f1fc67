// emi_ipm_ladder.hip -- the mesh ladder of a context's whole batch (emi_ipm_solve_ladder_*, emi_ipm_solve_refine_*,
// emi_ipm_solve_restart_*): prolongation between LGL meshes, the repair of a guess that lies inside keep-outs, the moving discs'
// centres per mesh, the one driver that takes the B instances from rung to rung, with or without retiring those that meet the ODE
// tolerance, and the loop that runs that driver again, from the next start, on the instances an attempt did not solve.
//
//   emi_prolong_rows_kernel  Vf[r][q] = sum_j PT[j][q] Vc[src(r)][j]: a thread owns one fine node and PROLONG_ROWS rows, reads PT[j][q]
//                            once per j (coalesced along q), the coarse values as wave-uniform loads, and accumulates with fma
//                            in ascending j.  One writer per output; a row's bits depend on nothing but its source row and P.  The
//                            source row comes from a list (the gather that compacts a batch and the prolongation are one pass);
//                            without a list it is the row itself (emi_prolong_dev)
//   emi_repair_guess_kernel  mi355x::repair_guess (host/eMI355X.cpp) with one thread per (instance, interior node): nodes do not
//                            interact, so the sweeps of a node are the host's sweeps of that node.  Contraction off.
//   emi_shard_move_kernel    the instances of a list copied between two sets of up to 4 arrays [instance][rows][ld] whose leading
//                            dimensions differ (compact M against padded ldm): a thread owns one node and walks the rows, so every
//                            access of a wave is a run of consecutive doubles along the node axis.  No arithmetic.
//   emi_track_waypoints_kernel  the centres of the track rows on the context's mesh from waypoint tables kept on the device:
//                            emi_track_centres (emi_host.cpp) with one thread per (result set, track, node), the waypoint set of a
//                            result set taken from a list, so the compaction of a batch is part of the launch.  Contraction off.
//   LadderRun                the driver: one loop over the rungs in named phases, for the ladder with refinement and, as the run that
//                            checks on no rung, for the plain ladder.  Who is live and who goes where is kept by a RefineBook
//                            (emi_refine_book.hpp, host-only).  Nothing of a trajectory's size crosses to the host between rungs.
//   ipm_solve_restart        one LadderRun per attempt on the pending instances, who they are kept by a RestartBook
//                            (emi_restart_book.hpp, host-only).  A restart adds no kernel: the start of a compact batch is
//                            emi_start_guess_dev on that batch, its controls come through emi_shard_move_kernel.
// emi_prolong_matrix and emi_ipm_refine_decide, which need no device, are in emi_host.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "emi_ctx.hpp"
#include "emi_refine_book.hpp"
#include "emi_restart_book.hpp"

namespace emi {
namespace {

constexpr int PROLONG_T = 256;      // fine nodes per block
constexpr int PROLONG_ROWS = 4;     // rows per thread
constexpr int REPAIR_T = 256;
constexpr int MOVE_T = 256;         // nodes per block
constexpr int TRACK_T = 256;        // nodes per block

// the source row of output row r: map[r / group] * group + r % group (map null: r)
__global__ __launch_bounds__(PROLONG_T) void emi_prolong_rows_kernel(const double* __restrict__ PT, const double* __restrict__ Vc,
                                                                     const int* __restrict__ map, int group, double* __restrict__ Vf, int Mc,
                                                                     int Mf, int R) {
    const int q = blockIdx.x * PROLONG_T + threadIdx.x;
    if (q >= Mf) return;
    for (int r0 = blockIdx.y * PROLONG_ROWS; r0 < R; r0 += gridDim.y * PROLONG_ROWS) {
        const double* v[PROLONG_ROWS];
        double acc[PROLONG_ROWS];
#pragma unroll
        for (int i = 0; i < PROLONG_ROWS; ++i) {
            const int r = r0 + i < R ? r0 + i : r0;                     // a row past the end reads the group's first (not stored)
            const size_t src = map ? (size_t)map[r / group] * group + r % group : (size_t)r;
            v[i] = Vc + src * Mc;
            acc[i] = 0.0;
        }
        for (int j = 0; j < Mc; ++j) {
            const double p = PT[(size_t)j * Mf + q];
#pragma unroll
            for (int i = 0; i < PROLONG_ROWS; ++i) acc[i] = fma(p, v[i][j], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < PROLONG_ROWS; ++i)
            if (r0 + i < R) Vf[(size_t)(r0 + i) * Mf + q] = acc[i];
    }
}

// Grid (chunks of MOVE_T nodes, list entries): one writer per element, nothing shared between threads
__global__ __launch_bounds__(MOVE_T) void emi_shard_move_kernel(ShardMoveArgs a) {
    const int i = a.first + blockIdx.y, k = blockIdx.x * MOVE_T + threadIdx.x;
    if (i >= a.n || k >= a.len) return;
    const size_t from = a.sidx ? (size_t)a.sidx[i] : (size_t)i, to = a.didx ? (size_t)a.didx[i] : (size_t)i;
#pragma unroll
    for (int q = 0; q < SHARD_MOVE_ARRAYS; ++q) {
        if (q >= a.narrays) break;
        const int rows = a.rows[q];
        const double* s = a.src[q] + from * rows * a.sld[q] + k;
        double* d = a.dst[q] + to * rows * a.dld[q] + k;
        for (int r = 0; r < rows; ++r) d[(size_t)r * a.dld[q]] = s[(size_t)r * a.sld[q]];
    }
}

__global__ __launch_bounds__(REPAIR_T) void emi_repair_guess_kernel(RepairArgs a) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * REPAIR_T + threadIdx.x, b = blockIdx.y;
    if (k < 1 || k + 1 >= a.M) return;                      // end nodes are never touched
    double* xp = a.X + ((size_t)b * a.ns + a.px) * a.M + k;
    double* yp = a.X + ((size_t)b * a.ns + a.py) * a.M + k;
    const double* recs = a.recs + (size_t)(a.path_sets > 1 ? b : 0) * a.np * EMI_PATH_REC;
    const int tset = a.track_sets > 1 ? b : 0;
    const double margin = 0.05;
    double x = *xp, y = *yp;
    bool any = false;
    for (int sweep = 0; sweep < 50; ++sweep) {
        bool moved = false;
        for (int j = 0; j < a.np; ++j) {
            const double* r = recs + (size_t)j * EMI_PATH_REC;
            const int kind = (int)r[0];
            double xc, yc, ct = 1, st = 0, asq, bsq;
            if (kind == EMI_PATH_ELLIPSE) { xc = r[1]; yc = r[2]; ct = r[3]; st = r[4]; asq = r[5]; bsq = r[6]; }
            else if (kind == EMI_PATH_DISC) { xc = r[1]; yc = r[2]; asq = bsq = r[3]; }
            else {
                const int t = (int)r[1];
                if (t < 0 || t >= a.ntracks) continue;
                const size_t off = ((size_t)tset * a.ntracks + t) * a.M + k;
                xc = a.trkx[off]; yc = a.trky[off]; asq = bsq = r[2];
            }
            if (!(asq > 0) || !(bsq > 0)) continue;
            const double dx = x - xc, dy = y - yc;
            double ex = ct * dx - st * dy, ey = st * dx + ct * dy;
            const double q = ex * ex / asq + ey * ey / bsq;
            if (q >= 1.0 + 0.5 * margin) continue;
            if (q < 1e-12) { ex = 0; ey = sqrt(bsq * (1.0 + margin)); }        // dead centre: minor axis
            else { const double g = sqrt((1.0 + margin) / q); ex *= g; ey *= g; }
            x = xc + ct * ex + st * ey;
            y = yc - st * ex + ct * ey;
            moved = true;
        }
        if (!moved) break;
        any = true;
    }
    if (any) { *xp = x; *yp = y; }
}

// Grid (chunks of TRACK_T nodes, result sets x tracks): one writer per output, nothing shared between threads.  The statements of
// emi_track_centres, each operation rounded once (contraction off, a true division): the stores are that function's bits, in an
// f32 context after the conversion emi_set_tracks applies.  The waypoint row of a block is wave-uniform
template <typename T>
__global__ __launch_bounds__(TRACK_T) void emi_track_waypoints_kernel(TrackWaypointArgs a) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * TRACK_T + threadIdx.x, pair = a.first + blockIdx.y;
    if (k >= a.M || pair >= a.n * a.ntracks) return;
    const int i = pair / a.ntracks, trk = pair % a.ntracks;
    const size_t row = (size_t)(a.map ? a.map[i] : i) * a.ntracks + trk;
    const double *t = a.t + row * a.ld, *x = a.x + row * a.ld, *y = a.y + row * a.ld;
    const int nway = a.cnt[row];
    const double tv = a.node_t[k];
    int j = 0;
    if (tv > t[nway - 1]) {
        j = nway - 2;
    } else if (tv >= t[0]) {
        for (int s = 0; s + 1 < nway; ++s)
            if (tv >= t[s] && tv <= t[s + 1]) j = s;
    }
    const double dt = t[j + 1] - t[j];
    const size_t out = (size_t)pair * a.M + k;
    ((T*)a.xc)[out] = (T)((tv - t[j]) * (x[j + 1] - x[j]) / dt + x[j]);
    ((T*)a.yc)[out] = (T)((tv - t[j]) * (y[j + 1] - y[j]) / dt + y[j]);
}

}  // namespace

template <typename T>
hipError_t launch_track_waypoints(TrackWaypointArgs a, hipStream_t s) {
    if (a.n <= 0 || a.ntracks <= 0 || a.M <= 0) return hipSuccess;
    if (a.ld < 2 || (long long)a.n * a.ntracks > 0x7fffffffLL) return hipErrorInvalidValue;
    const int pairs = a.n * a.ntracks;
    for (a.first = 0; a.first < pairs; a.first += 65535) {
        const int ny = pairs - a.first < 65535 ? pairs - a.first : 65535;
        hipLaunchKernelGGL(emi_track_waypoints_kernel<T>, dim3((a.M + TRACK_T - 1) / TRACK_T, ny), dim3(TRACK_T), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
template hipError_t launch_track_waypoints<double>(TrackWaypointArgs, hipStream_t);
template hipError_t launch_track_waypoints<float>(TrackWaypointArgs, hipStream_t);

hipError_t launch_prolong_rows(const double* PT, const double* Vc, const int* map, int group, double* Vf, int Mc, int Mf, int R, hipStream_t s) {
    if (R <= 0) return hipSuccess;
    if (group < 1) return hipErrorInvalidValue;
    const int groups = (R + PROLONG_ROWS - 1) / PROLONG_ROWS;
    const dim3 grid((Mf + PROLONG_T - 1) / PROLONG_T, groups < 65535 ? groups : 65535);
    hipLaunchKernelGGL(emi_prolong_rows_kernel, grid, dim3(PROLONG_T), 0, s, PT, Vc, map, group, Vf, Mc, Mf, R);
    return hipGetLastError();
}

hipError_t launch_shard_move(ShardMoveArgs a, hipStream_t s) {
    if (a.n <= 0 || a.len <= 0) return hipSuccess;
    if (a.narrays < 1 || a.narrays > SHARD_MOVE_ARRAYS) return hipErrorInvalidValue;
    for (a.first = 0; a.first < a.n; a.first += 65535) {
        const int ny = a.n - a.first < 65535 ? a.n - a.first : 65535;
        hipLaunchKernelGGL(emi_shard_move_kernel, dim3((a.len + MOVE_T - 1) / MOVE_T, ny), dim3(MOVE_T), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_repair_guess(const RepairArgs& a, hipStream_t s) {
    if (a.np <= 0 || a.M <= 2 || a.B <= 0) return hipSuccess;
    if (a.B > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(emi_repair_guess_kernel, dim3((a.M + REPAIR_T - 1) / REPAIR_T, a.B), dim3(REPAIR_T), 0, s, a);
    return hipGetLastError();
}

// the arrays of a run between its rungs: P transposed for the present pair of rungs, the compact iterates and multipliers of two
// consecutive rungs (a fall-back returns the older set), the gathered bounds of the live instances, the estimates, and the lists
// [7][B]: row map | live | two (source, destination) pairs | the levels of emi_start_guess_dev
struct IpmLadderWs {
    DeviceArray<double> PT, X[2], U[2], LamF[2], LamC[2], zl, zu, err;
    DeviceArray<int> lists;
};

void ipm_ladder_destroy(IpmLadderWs* w) { delete w; }

namespace {

#define L_HIP(call) HIP_TRY_AS(c, entry, call)
#define L_TRY EMI_TRY

// One call of emi_ipm_solve_ladder_dev / emi_ipm_solve_refine_dev, or one attempt of emi_ipm_solve_restart_dev.  The first block of
// members is the call as it came; rf null: no rung checks the ODE error, and `book` was begun with RefineBook::NEVER
struct LadderRun {
    emi_ctx_t c;
    const char* entry;                  // the entry point, for the messages
    int nrungs;
    const emi_ipm_rung_t* rungs;
    double t0, tf;
    const emi_ipm_refine_t* rf;
    const void *dX0, *dU0;
    int ldm;
    void *dX, *dU, *dLamF, *dLamC;
    RefineBook book;
    // an attempt of a restart run (rb null: none).  The book may begin from a subset; start: where the states of rung 0 come from
    // when dX0 is null, its sets those of the batch of rung 0; drop: EMI_RESTART_DROP_FAILED
    RestartBook* rb = nullptr;
    int attempt = 0;
    const emi_start_t* start = nullptr;
    bool drop = false;
    // the context at entry
    const int B = c->B, ns = c->ns, nc = c->nc, nv = ns + nc, np = emi_api::np_total(c), sets = c->path_sets;
    const hipStream_t s = c->stream;
    IpmLadderWs* w = nullptr;
    int *d_map = nullptr, *d_live = nullptr, *d_pair[2][2] = {}, *d_level = nullptr;
    RefineBook::Moves sent[2];          // the groups of retirees as they went up (a restart run leaves out who is to be solved again)
    // what restore_context has to undo
    bool table_compacted = false, centres_compacted = false;
    const double* master = nullptr;     // the record table in the caller's numbering: the last rung's that brought one, else `table`
    std::vector<double> table;          // ... the context's, read back before its first compaction
    // the rung
    int r = 0, M = 0, Mc = 0, n = 0, cur = 0;
    bool live_up = false;               // the live list of this rung is on the device
    double *cX = nullptr, *cU = nullptr, *cLF = nullptr, *cLC = nullptr;
    emi_ipm_bounds_t bd{};
    std::vector<double> tau, wt, D, tau_c, w_c, herr;
    std::vector<emi_ipm_result_t> res;

    int run() {
        const int st = climb();
        // the context as the caller knows it -- also after an error (whose message stays)
        const std::string msg = c->err;
        const int back = restore_context();
        if (st) { c->err = msg; return st; }
        return back;
    }

    int climb() {
        L_TRY(reserve());
        for (r = 0; r < nrungs && !book.done(); ++r) {
            L_TRY(enter_rung());
            L_TRY(place_iterate());
            L_TRY(gather_bounds());
            L_TRY(solve());
            L_TRY(check_and_retire());
        }
        return EMI_OK;
    }

    int reserve() {
        if (!c->ipm_ladder) c->ipm_ladder = new IpmLadderWs();
        w = c->ipm_ladder;
        int Mmax = 0;
        bool gathers = false;           // per-instance bounds come in the caller's numbering: gathered once somebody has left
        for (int q = 0; q < nrungs; ++q) {
            Mmax = std::max(Mmax, rungs[q].M);
            gathers = gathers || ((rf || rb) && B > 1 && rungs[q].bd.nsets == B);
        }
        L_HIP(hipStreamSynchronize(s));                 // a launch in flight may still use an array that has to move
        for (int k = 0; k < 2 && k < nrungs; ++k) {
            L_HIP(w->X[k].reserve((size_t)B * ns * Mmax)); L_HIP(w->U[k].reserve((size_t)B * nc * Mmax));
            L_HIP(w->LamF[k].reserve((size_t)B * ns * Mmax)); L_HIP(w->LamC[k].reserve((size_t)B * np * Mmax));
        }
        if (gathers) { L_HIP(w->zl.reserve((size_t)B * nv * Mmax)); L_HIP(w->zu.reserve((size_t)B * nv * Mmax)); }
        if (rf) L_HIP(w->err.reserve((size_t)B));
        L_HIP(w->lists.reserve((size_t)7 * B));
        d_map = w->lists.p;
        d_live = d_map + B;
        for (int k = 0; k < 2; ++k) { d_pair[k][0] = d_map + (2 + 2 * k) * B; d_pair[k][1] = d_map + (3 + 2 * k) * B; }
        d_level = d_map + 6 * B;
        herr.resize(B); res.resize(B);
        return EMI_OK;
    }

    // the live list on the device, for whoever of this rung needs the caller's numbering (uploaded once)
    int need_live() {
        if (live_up) return EMI_OK;
        L_HIP(hipMemcpyAsync(d_live, book.caller_map(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
        live_up = true;
        return EMI_OK;
    }

    // the master table as the context's: as it is while the batch is whole or the table shared, else the rows of the live instances
    int set_table() {
        const int* live = book.caller_map();
        const size_t per = (size_t)c->np * EMI_PATH_REC;
        if (!master) {
            table.resize((size_t)sets * per);
            L_TRY(emi_api::download_real(c, table.data(), c->d_path.p, table.size()));
            master = table.data();
        }
        if (sets == 1 || !live) return emi_set_path(c, c->np, sets, master, c->px, c->py);
        std::vector<double> t((size_t)n * per);
        for (int i = 0; i < n; ++i) std::copy(master + live[i] * per, master + (live[i] + 1) * per, t.begin() + i * per);
        table_compacted = true;
        return emi_set_path(c, c->np, n, t.data(), c->px, c->py);
    }

    int enter_rung() {
        const emi_ipm_rung_t& g = rungs[r];
        M = g.M; Mc = r > 0 ? rungs[r - 1].M : 0; n = book.n(); cur = r & 1; live_up = false;
        tau_c.swap(tau); w_c.swap(wt);                  // (the previous rung's, for the prolongation matrix)
        tau.resize(M); wt.resize(M); D.resize((size_t)M * M);
        L_TRY(emi_lgl(M, tau.data(), wt.data(), D.data()));
        L_TRY(emi_set_mesh(c, M, tau.data(), wt.data(), D.data(), t0, tf));
        if (n != c->B) L_TRY(emi_set_batch(c, n));
        if (g.recs && c->np > 0) master = g.recs;
        if (c->np > 0 && (g.recs || (sets > 1 && c->path_sets != n))) L_TRY(set_table());
        // track rows (the entry point has seen to the waypoints): the centres of the live instances on this mesh, ahead of the repair,
        // which reads them.  The set map of the launch does the compaction; a shared waypoint set serves whoever is live
        if (c->np > 0 && c->path_has_track) {
            const bool compact = c->wp_sets == B && B > 1 && book.caller_map();
            if (compact) { L_TRY(need_live()); centres_compacted = true; }
            L_TRY(emi_tracks_from_waypoints_dev(c, compact ? n : 0, compact ? d_live : nullptr));
        }
        return EMI_OK;
    }

    // the start of rung 0.  A whole batch with dX0: two copies.  A batch that begins from a subset: the rows of the live instances
    // through the live list (one emi_shard_move_kernel launch).  Without dX0 the states are emi_start_guess_dev's for the batch as the
    // context now holds it (mesh, table and centres of the live instances), n levels come down
    int place_start() {
        const bool whole = n == B;
        if (whole) {
            if (dX0) L_HIP(hipMemcpyAsync(cX, dX0, (size_t)B * ns * M * sizeof(double), hipMemcpyDeviceToDevice, s));
            if (nc > 0) L_HIP(hipMemcpyAsync(cU, dU0, (size_t)B * nc * M * sizeof(double), hipMemcpyDeviceToDevice, s));
        } else if (dX0 || nc > 0) {
            L_TRY(need_live());
            ShardMoveArgs a{};
            int q = 0;
            if (dX0) { a.src[q] = (const double*)dX0; a.dst[q] = cX; a.rows[q] = ns; ++q; }
            if (nc > 0) { a.src[q] = (const double*)dU0; a.dst[q] = cU; a.rows[q] = nc; ++q; }
            for (int i = 0; i < q; ++i) a.sld[i] = a.dld[i] = M;
            a.sidx = d_live; a.n = n; a.narrays = q; a.len = M;
            L_HIP(launch_shard_move(a, s));
        }
        if (dX0) return EMI_OK;
        L_TRY(emi_start_guess_dev(c, start, cX, d_level));
        L_HIP(hipMemcpyAsync(rb->level.data(), d_level, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
        L_HIP(hipStreamSynchronize(s));
        return EMI_OK;
    }

    // this rung's iterate in one of the two sets (not the previous rung's): the start, or the previous rung's final iterate prolonged,
    // the rows of whoever left that batch skipped by the row map
    int place_iterate() {
        cX = w->X[cur].p; cU = w->U[cur].p; cLF = w->LamF[cur].p; cLC = w->LamC[cur].p;
        if (r == 0) return place_start();
        L_TRY(prolong_matrix());
        const int* map = book.row_map();
        if (map) L_HIP(hipMemcpyAsync(d_map, map, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
        L_HIP(launch_prolong_rows(w->PT.p, w->X[cur ^ 1].p, map ? d_map : nullptr, ns, cX, Mc, M, n * ns, s));
        if (nc > 0) L_HIP(launch_prolong_rows(w->PT.p, w->U[cur ^ 1].p, map ? d_map : nullptr, nc, cU, Mc, M, n * nc, s));
        return EMI_OK;
    }

    // P transposed of the pair of rungs (Mc, M) into w->PT, complete on return (PT is rewritten for the next pair)
    int prolong_matrix() {
        std::vector<double> P((size_t)M * Mc), PT((size_t)M * Mc);
        L_TRY(emi_prolong_matrix(Mc, tau_c.data(), w_c.data(), M, tau.data(), P.data()));
        for (int q = 0; q < M; ++q)
            for (int j = 0; j < Mc; ++j) PT[(size_t)j * M + q] = P[(size_t)q * Mc + j];
        L_HIP(hipStreamSynchronize(s));
        L_HIP(w->PT.reserve(PT.size()));
        L_HIP(hipMemcpyAsync(w->PT.p, PT.data(), PT.size() * sizeof(double), hipMemcpyHostToDevice, s));
        L_HIP(hipStreamSynchronize(s));
        return EMI_OK;
    }

    int gather_bounds() {
        bd = rungs[r].bd;
        if (bd.nsets != B || n == B) return EMI_OK;     // shared, or everybody is still there
        L_TRY(need_live());
        ShardMoveArgs a{};
        a.src[0] = (const double*)bd.zl; a.src[1] = (const double*)bd.zu; a.dst[0] = w->zl.p; a.dst[1] = w->zu.p;
        a.rows[0] = a.rows[1] = nv; a.sld[0] = a.sld[1] = a.dld[0] = a.dld[1] = M;
        a.sidx = d_live; a.n = n; a.narrays = 2; a.len = M;
        L_HIP(launch_shard_move(a, s));
        bd.zl = w->zl.p; bd.zu = w->zu.p; bd.nsets = n;
        return EMI_OK;
    }

    int solve() {
        const emi_ipm_rung_t& g = rungs[r];
        if (g.repair) L_TRY(emi_repair_guess_dev(c, cX));
        L_TRY(emi_ipm_solve_shard_dev(c, cX, cU, &bd, &g.opt, cLF, cLC, res.data()));
        book.record_solve(r, res.data());
        return EMI_OK;
    }

    // a group of retirees from one of the two sets (on Mk nodes) into the caller's arrays; k: which pair of lists carries it
    int move_out(const RefineBook::Moves& all, int k, int set, int Mk) {
        RefineBook::Moves& m = sent[k];
        m = RefineBook::Moves{};
        for (size_t i = 0; i < all.to.size(); ++i) {
            if (rb && !rb->writes(attempt, book.verdict_of(all.to[i]))) continue;
            m.from.push_back(all.from[i]); m.to.push_back(all.to[i]);
        }
        const int cnt = (int)m.from.size();
        if (cnt == 0) return EMI_OK;
        L_HIP(hipMemcpyAsync(d_pair[k][0], m.from.data(), (size_t)cnt * sizeof(int), hipMemcpyHostToDevice, s));
        L_HIP(hipMemcpyAsync(d_pair[k][1], m.to.data(), (size_t)cnt * sizeof(int), hipMemcpyHostToDevice, s));
        const double* const src[SHARD_MOVE_ARRAYS] = {w->X[set].p, w->U[set].p, w->LamF[set].p, w->LamC[set].p};
        void* const dst[SHARD_MOVE_ARRAYS] = {dX, dU, dLamF, dLamC};
        const int rows[SHARD_MOVE_ARRAYS] = {ns, nc, ns, np};
        ShardMoveArgs a{};
        int q = 0;
        for (int i = 0; i < SHARD_MOVE_ARRAYS; ++i) {
            if (rows[i] <= 0) continue;
            a.src[q] = src[i]; a.dst[q] = (double*)dst[i]; a.rows[q] = rows[i]; a.sld[q] = Mk; a.dld[q] = ldm;
            ++q;
        }
        a.sidx = d_pair[k][0]; a.didx = d_pair[k][1]; a.n = cnt; a.narrays = q; a.len = Mk;
        L_HIP(launch_shard_move(a, s));
        return EMI_OK;
    }

    int check_and_retire() {
        const bool last = r + 1 == nrungs;
        if (book.checks(r)) {
            L_TRY(emi_ode_error_dev(c, cX, cU, rf->ul, rf->uu, nullptr, w->err.p));
            L_HIP(hipMemcpyAsync(herr.data(), w->err.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
            L_HIP(hipStreamSynchronize(s));
            book.decide(r, herr.data(), rf->ode_tol, last);
        } else if (drop) {
            book.drop_or_climb(r, last);
        } else if (last) {
            book.return_all(r);
        } else {                                        // a mesh-sequencing rung: everybody climbs
            book.climb_all();
            return EMI_OK;
        }
        L_TRY(move_out(book.here, 0, cur, M));
        L_TRY(move_out(book.older, 1, cur ^ 1, Mc));
        L_HIP(hipStreamSynchronize(s));                 // (the lists are `sent`, rewritten at the next decision)
        return EMI_OK;
    }

    // only what the run changed: the batch size, a compacted table, compacted centres (on the mesh the context is on)
    int restore_context() {
        if (c->B != B) L_TRY(emi_set_batch(c, B));
        if (table_compacted) L_TRY(emi_set_path(c, c->np, sets, master, c->px, c->py));
        if (centres_compacted && c->M > 0) L_TRY(emi_tracks_from_waypoints_dev(c, 0, nullptr));
        return EMI_OK;
    }
};

}  // namespace

int ipm_solve_refine(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t& rf, const void* dX0,
                     const void* dU0, int ldm, void* dX, void* dU, void* dLamF, void* dLamC, emi_ipm_result_t* results, double* err,
                     emi_ipm_refine_result_t* out) {
    if (emi_api::has_param_table(c))
        return emi_api::fail(c, EMI_ERR_UNSUPPORTED, "emi_ipm_solve_refine_dev: the context holds a per-instance parameter table (emi_set_model_params_batch); "
                             "this driver compacts the batch and has no row map for the table");
    LadderRun run{c, "emi_ipm_solve_refine_dev", nrungs, rungs, t0, tf, &rf, dX0, dU0, ldm, dX, dU, dLamF, dLamC};
    run.book.begin(c->B, nrungs, rf.first_check, results, err, out);
    return run.run();
}

// the run that never checks: after the last rung everybody goes to the caller's arrays, which are sized for that rung
int ipm_solve_ladder(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const void* dX0, const void* dU0, void* dX,
                     void* dU, void* dLamF, void* dLamC, emi_ipm_result_t* results) {
    std::vector<double> err((size_t)nrungs * c->B);
    std::vector<emi_ipm_refine_result_t> out(c->B);
    LadderRun run{c, "emi_ipm_solve_ladder_dev", nrungs, rungs, t0, tf, nullptr, dX0, dU0, rungs[nrungs - 1].M, dX, dU, dLamF, dLamC};
    run.book.begin(c->B, nrungs, RefineBook::NEVER, results, err.data(), out.data());
    return run.run();
}

// One LadderRun per attempt on the instances that are still pending.  Every attempt leaves the context as the refine call does (batch
// B, the full table, the centres of all sets), so the next one compacts from the caller's numbering again; a table that a rung
// brought is replaced by the one the context came with before rung 0 is solved again
int ipm_solve_restart(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t* rf,
                      const emi_ipm_restart_t& rs, const void* dX0, const void* dU0, int ldm, void* dX, void* dU, void* dLamF, void* dLamC,
                      emi_ipm_result_t* results, double* err, emi_ipm_restart_result_t* out) {
    const char* entry = "emi_ipm_solve_restart_dev";
    if (emi_api::has_param_table(c))
        return emi_api::fail(c, EMI_ERR_UNSUPPORTED, "%s: the context holds a per-instance parameter table (emi_set_model_params_batch); "
                             "this driver compacts the batch and has no row map for the table", entry);
    const int B = c->B, ns = c->ns, A = (dX0 ? 1 : 0) + rs.nstarts;
    RestartBook rb;
    rb.begin(B, A, nrungs, rf ? rf->first_check : RefineBook::NEVER, rs.retry_mask, results, err, out);
    bool brings_table = false;
    for (int r = 0; r < nrungs; ++r) brings_table = brings_table || rungs[r].recs;
    std::vector<double> table;          // the context's record table at entry
    if (brings_table && A > 1) {
        table.resize((size_t)c->path_sets * c->np * EMI_PATH_REC);
        EMI_TRY(emi_api::download_real(c, table.data(), c->d_path.p, table.size()));
    }
    std::vector<emi_ipm_rung_t> rg(rungs, rungs + nrungs);
    std::vector<double> xa, xb, box;    // the sets of the pending instances of a start with one set per instance
    for (int a = 0; a < A && !rb.done(); ++a) {
        rg[0].opt.max_iter = rs.patience && rs.patience[a] > 0 ? rs.patience[a] : rungs[0].opt.max_iter;
        const bool guess = dX0 && a == 0;
        emi_start_t st{};
        if (!guess) {
            st = rs.starts[a - (dX0 ? 1 : 0)];
            if (st.nsets == B && rb.n() != B) {
                const int n = rb.n();
                xa.resize((size_t)n * ns); xb.resize((size_t)n * ns); box.resize((size_t)n * 4);
                for (int i = 0; i < n; ++i) {
                    const size_t b = (size_t)rb.pending[i];
                    std::copy(st.xa + b * ns, st.xa + (b + 1) * ns, xa.begin() + (size_t)i * ns);
                    std::copy(st.xb + b * ns, st.xb + (b + 1) * ns, xb.begin() + (size_t)i * ns);
                    if (st.box) std::copy(st.box + b * 4, st.box + (b + 1) * 4, box.begin() + (size_t)i * 4);
                }
                st.xa = xa.data(); st.xb = xb.data(); st.box = st.box ? box.data() : nullptr; st.nsets = n;
            }
        }
        if (a > 0 && !table.empty()) EMI_TRY(emi_set_path(c, c->np, c->path_sets, table.data(), c->px, c->py));
        LadderRun run{c, entry, nrungs, rg.data(), t0, tf, rf, guess ? dX0 : nullptr, dU0, ldm, dX, dU, dLamF, dLamC};
        run.rb = &rb; run.attempt = a; run.start = guess ? nullptr : &st; run.drop = (rs.flags & EMI_RESTART_DROP_FAILED) != 0;
        rb.open(a, run.book);
        EMI_TRY(run.run());
        rb.close(a, run.book);
    }
    return EMI_OK;
}

}  // namespace emi
