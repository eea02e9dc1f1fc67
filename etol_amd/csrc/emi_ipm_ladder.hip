// emi_ipm_ladder.hip -- the mesh ladder of a context's whole batch (emi_ipm_solve_ladder_*): prolongation between LGL meshes,
// the repair of a guess that lies inside keep-outs, and the driver that takes the B instances from rung to rung.
//
//   emi_prolong_matrix       host: P[Mf][Mc], row q = the Lagrange basis polynomials of the coarse nodes at tau_f[q] (barycentric
//                            second form, weights (-1)^j sqrt(w_j): interp_lgl of host/eMI355X.cpp as a matrix)
//   emi_prolong_kernel       Vf[r][q] = sum_j PT[j][q] Vc[r][j]: a thread owns one fine node and PROLONG_ROWS rows, reads PT[j][q]
//                            once per j (coalesced along q), the coarse values as wave-uniform loads, and accumulates with fma
//                            in ascending j.  One writer per output; a row's bits depend on nothing but the row and P.
//   emi_repair_guess_kernel  mi355x::repair_guess (host/eMI355X.cpp) with one thread per (instance, interior node): nodes do not
//                            interact, so the sweeps of a node are the host's sweeps of that node.  Contraction off.
//   ipm_solve_ladder         per rung: emi_lgl + emi_set_mesh, emi_set_path where the rung brings a table, prolongation of X and U
//                            from the previous rung's final iterate, the repair where asked for, emi_ipm_solve_shard_dev.  Nothing
//                            of a trajectory's size crosses to the host between rungs.
//   emi_prolong_rows_kernel  emi_prolong_kernel with the source row of an output row taken from a list: the gather that compacts a
//                            batch and the prolongation are one pass.  The same sums: a row has the bits of its source row alone.
//   emi_shard_move_kernel    the instances of a list copied between two sets of up to 4 arrays [instance][rows][ld] whose leading
//                            dimensions differ (compact M against padded ldm): a thread owns one node and walks the rows, so every
//                            access of a wave is a run of consecutive doubles along the node axis.  No arithmetic.
//   emi_track_waypoints_kernel  the centres of the track rows on the context's mesh from waypoint tables kept on the device:
//                            emi_track_centres (emi_host.cpp) with one thread per (result set, track, node), the waypoint set of a
//                            result set taken from a list, so the compaction of a batch is part of the launch.  Contraction off.
//   emi_ipm_refine_decide    host: what becomes of an instance after its solve on a rung (retire / climb, and the verdict)
//   ipm_solve_refine         the ladder with the instances that meet the ODE tolerance retired rung by rung (emi_ode_error_dev per
//                            rung, the rule on the host, the rest compacted into a smaller batch of the same context)
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>
#include <vector>

#include "emi_ctx.hpp"

namespace emi {
namespace {

constexpr int PROLONG_T = 256;      // fine nodes per block
constexpr int PROLONG_ROWS = 4;     // rows per thread
constexpr int REPAIR_T = 256;
constexpr int MOVE_T = 256;         // nodes per block
constexpr int TRACK_T = 256;        // nodes per block

__global__ __launch_bounds__(PROLONG_T) void emi_prolong_kernel(const double* __restrict__ PT, const double* __restrict__ Vc,
                                                                double* __restrict__ Vf, int Mc, int Mf, int R) {
    const int q = blockIdx.x * PROLONG_T + threadIdx.x;
    if (q >= Mf) return;
    for (int r0 = blockIdx.y * PROLONG_ROWS; r0 < R; r0 += gridDim.y * PROLONG_ROWS) {
        const double* v[PROLONG_ROWS];
        double acc[PROLONG_ROWS];
#pragma unroll
        for (int i = 0; i < PROLONG_ROWS; ++i) {
            v[i] = Vc + (size_t)(r0 + i < R ? r0 + i : r0) * Mc;        // a row past the end reads the group's first (not stored)
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

// emi_prolong_kernel with the source row from a list (the existing kernel and its bits stay as they are): the same loads of PT, the
// same fused multiply-adds in ascending j
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

hipError_t launch_prolong(const double* PT, const double* Vc, double* Vf, int Mc, int Mf, int R, hipStream_t s) {
    if (R <= 0) return hipSuccess;
    const int groups = (R + PROLONG_ROWS - 1) / PROLONG_ROWS;
    const dim3 grid((Mf + PROLONG_T - 1) / PROLONG_T, groups < 65535 ? groups : 65535);
    hipLaunchKernelGGL(emi_prolong_kernel, grid, dim3(PROLONG_T), 0, s, PT, Vc, Vf, Mc, Mf, R);
    return hipGetLastError();
}

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

// the arrays of the ladder between its rungs: P transposed for the present pair of rungs, two sets of iterates (the rung being
// solved and the one before it), the multipliers of the rungs below the last
struct IpmLadderWs {
    DeviceArray<double> PT, X[2], U[2], LamF, LamC;
    // the ladder with refinement: compact iterates and multipliers of two consecutive rungs (a fall-back returns the older set), the
    // gathered bounds of the live instances, the estimates, and the lists [6][B]: row map | live | two (source, destination) pairs
    DeviceArray<double> rX[2], rU[2], rLamF[2], rLamC[2], zl, zu, err;
    DeviceArray<int> lists;
};

void ipm_ladder_destroy(IpmLadderWs* w) { delete w; }

// P transposed of the pair of rungs (Mc, M) into w.PT, complete on return (PT is rewritten for the next pair)
static int ladder_prolong_matrix(emi_ctx_t c, IpmLadderWs& w, int Mc, const std::vector<double>& tau_c, const std::vector<double>& w_c, int M,
                          const std::vector<double>& tau) {
    std::vector<double> P((size_t)M * Mc), PT((size_t)M * Mc);
    EMI_TRY(emi_prolong_matrix(Mc, tau_c.data(), w_c.data(), M, tau.data(), P.data()));
    for (int q = 0; q < M; ++q)
        for (int j = 0; j < Mc; ++j) PT[(size_t)j * M + q] = P[(size_t)q * Mc + j];
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, w.PT.reserve(PT.size()));
    HIP_TRY(c, hipMemcpyAsync(w.PT.p, PT.data(), PT.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}

#define L_HIP(call) HIP_TRY_AS(c, "emi_ipm_solve_ladder_dev", call)
#define L_TRY EMI_TRY

int ipm_solve_ladder(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const void* dX0, const void* dU0, void* dX,
                     void* dU, void* dLamF, void* dLamC, emi_ipm_result_t* results) {
    if (!c->ipm_ladder) c->ipm_ladder = new IpmLadderWs();
    IpmLadderWs& w = *c->ipm_ladder;
    const size_t B = (size_t)c->B, ns = (size_t)c->ns, nc = (size_t)c->nc, np = (size_t)emi_api::np_total(c);
    const hipStream_t s = c->stream;
    std::vector<double> tau, wt, D, tau_c, w_c;
    const void *pX = nullptr, *pU = nullptr;        // the previous rung's final iterate
    for (int r = 0; r < nrungs; ++r) {
        const emi_ipm_rung_t& g = rungs[r];
        const int M = g.M, Mc = r > 0 ? rungs[r - 1].M : 0;
        const bool last = r + 1 == nrungs;
        tau.resize(M); wt.resize(M); D.resize((size_t)M * M);
        L_TRY(emi_lgl(M, tau.data(), wt.data(), D.data()));
        L_TRY(emi_set_mesh(c, M, tau.data(), wt.data(), D.data(), t0, tf));
        if (g.recs) L_TRY(emi_set_path(c, c->np, c->path_sets, g.recs, c->px, c->py));
        // track rows (the entry point has seen to the waypoints): their centres on this mesh, ahead of the repair, which reads them
        if (c->np > 0 && c->path_has_track) L_TRY(emi_tracks_from_waypoints_dev(c, 0, nullptr));
        // where this rung's iterate lives: the caller's arrays on the last rung, else one of the two sets (not the previous rung's)
        void *cX = dX, *cU = dU, *cLF = dLamF, *cLC = dLamC;
        if (!last) {
            L_HIP(hipStreamSynchronize(s));             // a launch in flight may still use an array that has to move
            L_HIP(w.X[r & 1].reserve(B * ns * M)); L_HIP(w.U[r & 1].reserve(B * nc * M));
            L_HIP(w.LamF.reserve(B * ns * M)); L_HIP(w.LamC.reserve(B * np * M));
            cX = w.X[r & 1].p; cU = w.U[r & 1].p; cLF = w.LamF.p; cLC = w.LamC.p;
        }
        if (r == 0) {
            L_HIP(hipMemcpyAsync(cX, dX0, B * ns * M * sizeof(double), hipMemcpyDeviceToDevice, s));
            if (nc > 0) L_HIP(hipMemcpyAsync(cU, dU0, B * nc * M * sizeof(double), hipMemcpyDeviceToDevice, s));
        } else {
            L_TRY(ladder_prolong_matrix(c, w, Mc, tau_c, w_c, M, tau));
            L_TRY(emi_prolong_dev(c, Mc, M, w.PT.p, pX, c->B * c->ns, cX));
            if (nc > 0) L_TRY(emi_prolong_dev(c, Mc, M, w.PT.p, pU, c->B * c->nc, cU));
        }
        if (g.repair) L_TRY(emi_repair_guess_dev(c, cX));
        L_TRY(emi_ipm_solve_shard_dev(c, cX, cU, &g.bd, &g.opt, cLF, cLC, results + (size_t)r * B));
        pX = cX; pU = cU;
        tau_c.swap(tau); w_c.swap(wt);
    }
    return EMI_OK;
}


#undef L_HIP
#define L_HIP(call) HIP_TRY_AS(c, "emi_ipm_solve_refine_dev", call)

namespace {

// the rows of the live instances of the master table (shared table: as it is) as the context's table
int refine_set_table(emi_ctx_t c, const std::vector<double>& master, int np, int sets, const std::vector<int>& live) {
    if (np <= 0) return EMI_OK;
    if (sets == 1) return emi_set_path(c, np, 1, master.data(), c->px, c->py);
    const size_t per = (size_t)np * EMI_PATH_REC;
    std::vector<double> t(live.size() * per);
    for (size_t i = 0; i < live.size(); ++i) std::copy(master.begin() + live[i] * per, master.begin() + (live[i] + 1) * per, t.begin() + i * per);
    return emi_set_path(c, np, (int)live.size(), t.data(), c->px, c->py);
}

int refine_rungs(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t& rf, const void* dX0,
                 const void* dU0, int ldm, void* dX, void* dU, void* dLamF, void* dLamC, emi_ipm_result_t* results, double* err,
                 emi_ipm_refine_result_t* out, std::vector<double>& master, int sets, bool& table_changed) {
    IpmLadderWs& w = *c->ipm_ladder;
    const int B = c->B, ns = c->ns, nc = c->nc, nv = ns + nc, np = emi_api::np_total(c);
    const hipStream_t s = c->stream;
    int Mmax = 0;
    for (int r = 0; r < nrungs; ++r) Mmax = std::max(Mmax, rungs[r].M);
    L_HIP(hipStreamSynchronize(s));                 // a launch in flight may still use an array that has to move
    for (int k = 0; k < 2; ++k) {
        L_HIP(w.rX[k].reserve((size_t)B * ns * Mmax)); L_HIP(w.rU[k].reserve((size_t)B * nc * Mmax));
        L_HIP(w.rLamF[k].reserve((size_t)B * ns * Mmax)); L_HIP(w.rLamC[k].reserve((size_t)B * np * Mmax));
    }
    L_HIP(w.zl.reserve((size_t)B * nv * Mmax)); L_HIP(w.zu.reserve((size_t)B * nv * Mmax));
    L_HIP(w.err.reserve((size_t)B)); L_HIP(w.lists.reserve((size_t)6 * B));
    int* const d_map = w.lists.p;
    int* const d_live = d_map + B;
    int* const d_pair[2][2] = {{d_map + 2 * B, d_map + 3 * B}, {d_map + 4 * B, d_map + 5 * B}};

    std::vector<int> live(B), pos(B);               // live: the caller's numbers, ascending; pos: where each sits in the previous rung's batch
    for (int b = 0; b < B; ++b) live[b] = pos[b] = b;
    std::vector<double> tau, wt, D, tau_c, w_c, herr(B);
    std::vector<emi_ipm_result_t> res(B);
    for (int r = 0; r < nrungs && !live.empty(); ++r) {
        const emi_ipm_rung_t& g = rungs[r];
        const int M = g.M, Mc = r > 0 ? rungs[r - 1].M : 0, n = (int)live.size(), cur = r & 1, old = cur ^ 1;
        const bool last = r + 1 == nrungs;
        tau.resize(M); wt.resize(M); D.resize((size_t)M * M);
        L_TRY(emi_lgl(M, tau.data(), wt.data(), D.data()));
        L_TRY(emi_set_mesh(c, M, tau.data(), wt.data(), D.data(), t0, tf));
        if (n != c->B) L_TRY(emi_set_batch(c, n));
        if (g.recs && c->np > 0) master.assign(g.recs, g.recs + (size_t)c->np * sets * EMI_PATH_REC);
        if (c->np > 0 && (g.recs || (sets > 1 && c->path_sets != n))) {
            L_TRY(refine_set_table(c, master, c->np, sets, live));
            table_changed = true;
        }
        // the live list on the device, for whoever of this rung needs the caller's numbering (uploaded once)
        bool live_up = false;
        const auto need_live = [&]() -> int {
            if (live_up) return EMI_OK;
            L_HIP(hipMemcpyAsync(d_live, live.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
            live_up = true;
            return EMI_OK;
        };
        // track rows: the centres of the live instances on this mesh, the compaction done by the set map in the launch (a shared
        // waypoint set serves whoever is live), ahead of the repair, which reads them
        if (c->np > 0 && c->path_has_track) {
            const bool per_instance = c->wp_sets == B && B > 1;
            if (per_instance) L_TRY(need_live());
            L_TRY(emi_tracks_from_waypoints_dev(c, per_instance ? n : 0, per_instance ? d_live : nullptr));
        }
        double *cX = w.rX[cur].p, *cU = w.rU[cur].p, *cLF = w.rLamF[cur].p, *cLC = w.rLamC[cur].p;
        if (r == 0) {
            L_HIP(hipMemcpyAsync(cX, dX0, (size_t)B * ns * M * sizeof(double), hipMemcpyDeviceToDevice, s));
            if (nc > 0) L_HIP(hipMemcpyAsync(cU, dU0, (size_t)B * nc * M * sizeof(double), hipMemcpyDeviceToDevice, s));
        } else {
            L_TRY(ladder_prolong_matrix(c, w, Mc, tau_c, w_c, M, tau));
            L_HIP(hipMemcpyAsync(d_map, pos.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
            L_HIP(launch_prolong_rows(w.PT.p, w.rX[old].p, d_map, ns, cX, Mc, M, n * ns, s));
            if (nc > 0) L_HIP(launch_prolong_rows(w.PT.p, w.rU[old].p, d_map, nc, cU, Mc, M, n * nc, s));
        }
        emi_ipm_bounds_t bd = g.bd;
        if (bd.nsets == B && n < B) {               // per-instance bounds come in the caller's numbering
            L_TRY(need_live());
            ShardMoveArgs a{};
            a.src[0] = (const double*)g.bd.zl; a.src[1] = (const double*)g.bd.zu; a.dst[0] = w.zl.p; a.dst[1] = w.zu.p;
            a.rows[0] = a.rows[1] = nv; a.sld[0] = a.sld[1] = a.dld[0] = a.dld[1] = M;
            a.sidx = d_live; a.n = n; a.narrays = 2; a.len = M;
            L_HIP(launch_shard_move(a, s));
            bd.zl = w.zl.p; bd.zu = w.zu.p; bd.nsets = n;
        }
        if (g.repair) L_TRY(emi_repair_guess_dev(c, cX));
        L_TRY(emi_ipm_solve_shard_dev(c, cX, cU, &bd, &g.opt, cLF, cLC, res.data()));
        for (int i = 0; i < n; ++i) {
            results[(size_t)r * B + live[i]] = res[i];
            out[live[i]].rungs_solved = r + 1;
        }
        tau_c.swap(tau); w_c.swap(wt);
        if (r < rf.first_check) {                   // a mesh-sequencing rung: everybody climbs
            for (int i = 0; i < n; ++i) pos[i] = i;
            continue;
        }
        L_TRY(emi_ode_error_dev(c, cX, cU, rf.ul, rf.uu, nullptr, w.err.p));
        L_HIP(hipMemcpyAsync(herr.data(), w.err.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
        L_HIP(hipStreamSynchronize(s));
        // the rule; list 0: retirees that return this rung's iterate, list 1: those that fall back to the previous rung's
        std::vector<int> from[2], to[2], next, next_pos;
        for (int i = 0; i < n; ++i) {
            const int b = live[i];
            const bool has_good = r > rf.first_check;           // whoever climbed from a checked rung was solved there
            err[(size_t)r * B + b] = herr[i];
            int verdict = 0;
            if (!emi_ipm_refine_decide(res[i].status, herr[i], rf.ode_tol, has_good, last, &verdict)) {
                next.push_back(b); next_pos.push_back(i);
                continue;
            }
            const int k = verdict == EMI_REFINE_FELL_BACK ? 1 : 0;
            from[k].push_back(k ? pos[i] : i); to[k].push_back(b);
            out[b].verdict = verdict;
            out[b].rung = r - k;
            out[b].err = err[(size_t)(r - k) * B + b];
        }
        for (int k = 0; k < 2; ++k) {
            const int m = (int)from[k].size();
            if (m == 0) continue;
            const int set = k ? old : cur, Mk = k ? Mc : M;
            L_HIP(hipMemcpyAsync(d_pair[k][0], from[k].data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, s));
            L_HIP(hipMemcpyAsync(d_pair[k][1], to[k].data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, s));
            ShardMoveArgs a{};
            int q = 0;
            const auto add = [&](const double* src, void* dst, int rows) {
                if (rows <= 0) return;
                a.src[q] = src; a.dst[q] = (double*)dst; a.rows[q] = rows; a.sld[q] = Mk; a.dld[q] = ldm;
                ++q;
            };
            add(w.rX[set].p, dX, ns); add(w.rU[set].p, dU, nc); add(w.rLamF[set].p, dLamF, ns); add(w.rLamC[set].p, dLamC, np);
            a.sidx = d_pair[k][0]; a.didx = d_pair[k][1]; a.n = m; a.narrays = q; a.len = Mk;
            L_HIP(launch_shard_move(a, s));
        }
        L_HIP(hipStreamSynchronize(s));             // (the lists are locals)
        live.swap(next); pos.swap(next_pos);
    }
    return EMI_OK;
}

}  // namespace

int ipm_solve_refine(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t& rf, const void* dX0,
                     const void* dU0, int ldm, void* dX, void* dU, void* dLamF, void* dLamC, emi_ipm_result_t* results, double* err,
                     emi_ipm_refine_result_t* out) {
    if (!c->ipm_ladder) c->ipm_ladder = new IpmLadderWs();
    const int B = c->B, sets = c->path_sets;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t i = 0; i < (size_t)nrungs * B; ++i) {
        results[i] = emi_ipm_result_t{};
        results[i].status = -1;
        err[i] = nan;
    }
    for (int b = 0; b < B; ++b) out[b] = emi_ipm_refine_result_t{-1, EMI_REFINE_FAILED, 0, nan};
    // the master copy of the record table, in the caller's numbering
    std::vector<double> master((size_t)c->np * sets * EMI_PATH_REC);
    if (c->np > 0) L_TRY(emi_api::download_real(c, master.data(), c->d_path.p, master.size()));
    bool table_changed = false;
    const int st = refine_rungs(c, nrungs, rungs, t0, tf, rf, dX0, dU0, ldm, dX, dU, dLamF, dLamC, results, err, out, master, sets, table_changed);
    // the context as the caller knows it: batch B, the full table, the centres of every set -- also after an error (whose message stays)
    const std::string msg = c->err;
    int back = EMI_OK;
    if (c->B != B) back = emi_set_batch(c, B);
    if (!back && table_changed) back = emi_set_path(c, c->np, sets, master.data(), c->px, c->py);
    // ... and, where the table has track rows, the centres of all sets on the mesh the context is on
    if (!back && c->np > 0 && c->path_has_track && c->wp_ntracks > 0 && c->M > 0) back = emi_tracks_from_waypoints_dev(c, 0, nullptr);
    if (st) { c->err = msg; return st; }
    return back;
}

}  // namespace emi

extern "C" int emi_prolong_matrix(int Mc, const double* tau_c, const double* w_c, int Mf, const double* tau_f, double* P) {
#pragma clang fp contract(off)
    if (Mc < 2 || Mf < 2 || !tau_c || !w_c || !tau_f || !P) return EMI_ERR_ARG;
    for (int q = 0; q < Mf; ++q) {
        double* row = P + (size_t)q * Mc;
        int hit = -1;
        double den = 0.0;
        for (int j = 0; j < Mc; ++j) {
            const double dlt = tau_f[q] - tau_c[j];
            if (dlt == 0.0) { hit = j; break; }
            row[j] = ((j & 1) ? -1.0 : 1.0) * std::sqrt(w_c[j]) / dlt;
            den += row[j];
        }
        for (int j = 0; j < Mc; ++j) row[j] = hit >= 0 ? (j == hit ? 1.0 : 0.0) : row[j] / den;
    }
    return EMI_OK;
}

extern "C" int emi_ipm_refine_decide(int status, double err, double ode_tol, int has_good, int is_last, int* verdict) {
    const bool ok = status == EMI_IPM_CONVERGED || status == EMI_IPM_ACCEPTABLE;
    const bool met = std::isfinite(err) && err <= ode_tol;
    const int v = ok ? (met ? EMI_REFINE_MET : EMI_REFINE_NOT_MET) : (has_good ? EMI_REFINE_FELL_BACK : EMI_REFINE_FAILED);
    if (verdict) *verdict = v;
    return !(ok && !met && !is_last);
}
