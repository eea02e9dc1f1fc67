// emi_api_ode.hip -- the relative local ODE error of the C ABI (kernels: emi_ode_error.hip and the model's residual kernel in
// emi_node_kernels.hpp): the product alone (emi_interp_dev), and the estimate of the context's batch on its collocation mesh,
// device and host forms; the total calls take a context with delays too.  The operator builders emi_ode_error_operator and
// emi_ode_error_delay_operator are host code (emi_host.cpp).
#include "emi_ctx.hpp"

using namespace emi_api;

namespace {

// the stacked operator [E | E' | D] (rows padded to the even ldk), the point times and the interval scales of the mesh in force
int ode_operator(emi_ctx_t c) {
    if (!c->ode_dirty) return EMI_OK;
    const int M = c->M, nq = M - 1, np = 5 * nq, ldk = M + (M & 1);
    const double h = (c->tf - c->t0) / 2.0;
    std::vector<double> E((size_t)np * M), Ed((size_t)np * M), tq((size_t)np + nq);
    if (emi_ode_error_operator(M, c->h_tau.data(), c->h_w.data(), E.data(), Ed.data(), tq.data()))
        return fail(c, EMI_ERR_STATE, "emi_ode_error: no operator for this mesh");
    for (int p = 0; p < np; ++p) tq[p] = c->t0 + h * (tq[p] + 1.0);
    for (int k = 0; k < nq; ++k) tq[(size_t)np + k] = 0.5 * (c->h_tau[k + 1] - c->h_tau[k]) * h;
    HIP_TRY(c, c->d_ode_op.reserve((size_t)(2 * np + M) * ldk));
    HIP_TRY(c, c->d_ode_tq.reserve(tq.size()));
    const size_t row = (size_t)M * 8, drow = (size_t)ldk * 8;
    if (ldk != M) HIP_TRY(c, hipMemsetAsync(c->d_ode_op.p, 0, (size_t)2 * np * drow, c->stream));      // the padding column
    HIP_TRY(c, hipMemcpy2DAsync(c->d_ode_op.p, drow, E.data(), row, row, np, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpy2DAsync(c->d_ode_op.p + (size_t)np * ldk, drow, Ed.data(), row, row, np, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_ode_tq.p, tq.data(), tq.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, emi::launch_ode_copy_D((const double*)c->d_D.p, c->d_ode_op.p + (size_t)2 * np * ldk, M, ldk, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // E, Ed and tq are locals
    c->ode_dirty = false;
    return EMI_OK;
}

// The stacked operators of a context with delays, built once per (mesh, delays): the state rows' [E | E' | D | Edel(dt) ..
// Edel((xh-1) dt)] and the free controls' [E | Edel(dt) .. Edel(uh dt)].  The leading blocks are copies of ode_operator's array,
// so the products' leading columns are the plain call's; the delayed blocks come from the host (emi_ode_error_delay_operator).
int ode_delay_operator(emi_ctx_t c) {
    EMI_TRY(ode_operator(c));
    if (!c->odel_dirty) return EMI_OK;
    const int M = c->M, np = 5 * (M - 1), ldk = M + (M & 1), nxb = std::max(c->xh - 1, 0), nd = std::max(nxb, c->uh);
    const size_t blk = (size_t)np * ldk, head = (size_t)(2 * np + M) * ldk;
    std::vector<double> Ed((size_t)np * M), H(blk * nd, 0.0);          // H: the delayed blocks with padded rows
    for (int d = 0; d < nd; ++d) {
        if (emi_ode_error_delay_operator(M, c->h_tau.data(), c->h_w.data(), c->t0, c->tf, (d + 1) * c->delay_dt, Ed.data()))
            return fail(c, EMI_ERR_STATE, "emi_ode_error_total: no delayed operator for this mesh");
        for (int p = 0; p < np; ++p) memcpy(H.data() + d * blk + (size_t)p * ldk, Ed.data() + (size_t)p * M, (size_t)M * 8);
    }
    HIP_TRY(c, c->d_odel_ops.reserve(head + blk * nxb));
    HIP_TRY(c, c->d_odel_opc.reserve(blk * (1 + c->uh)));
    HIP_TRY(c, hipMemcpyAsync(c->d_odel_ops.p, c->d_ode_op.p, head * 8, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_odel_opc.p, c->d_ode_op.p, blk * 8, hipMemcpyDeviceToDevice, c->stream));
    if (nxb > 0) HIP_TRY(c, hipMemcpyAsync(c->d_odel_ops.p + head, H.data(), blk * nxb * 8, hipMemcpyHostToDevice, c->stream));
    if (c->uh > 0) HIP_TRY(c, hipMemcpyAsync(c->d_odel_opc.p + blk, H.data(), blk * c->uh * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // H is a local
    c->odel_dirty = false;
    return EMI_OK;
}

// what every form refuses; track and record tables play no part (f does not read them).  total: the caller takes delays
int ode_ready(emi_ctx_t c, const char* who, bool total = false) {
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: f64 contexts only", who);
    if (c->M <= 0 || c->model < 0 || c->B <= 0) return fail(c, EMI_ERR_STATE, "%s: mesh, model and batch must be set", who);
    if (c->nch > 0 && !total)
        return fail(c, EMI_ERR_UNSUPPORTED, "%s: contexts with delays (emi_set_delays) are not taken: f reads the delayed values "
                    "(emi_ode_error_total_dev / _host take them)", who);
    if (c->points_only) return fail(c, EMI_ERR_STATE, "%s: the mesh has no differentiation matrix (points-only mesh)", who);
    if (c->B > 65535) return fail(c, EMI_ERR_UNSUPPORTED, "%s: up to 65535 instances", who);
    return EMI_OK;
}

// the estimate of a context WITH delays: dU holds the ncf free controls, ul / uu their bounds
int ode_error_delayed(emi_ctx_t c, const void* dX, const void* dU, const double* ul, const double* uu, void* dEta, void* dErr) {
    HIP_TRY(c, hipSetDevice(c->device));
    EMI_TRY(ode_delay_operator(c));
    const int M = c->M, B = c->B, ns = c->ns, ncf = c->nc - c->nch, nq = M - 1, np = 5 * nq, ldk = M + (M & 1);
    const int nxb = std::max(c->xh - 1, 0), lds = (2 + nxb) * np + M, ldc = (1 + c->uh) * np;
    const double h = (c->tf - c->t0) / 2.0;
    const size_t nZs = (size_t)B * ns * lds, nZc = (size_t)B * ncf * ldc, nEta = (size_t)B * ns * nq;
    HIP_TRY(c, c->d_ode_ws.reserve(nZs + nZc + nEta));
    double *Zs = c->d_ode_ws.p, *Zc = Zs + nZs, *eta = dEta ? (double*)dEta : Zc + nZc;
    const bool clip = ul != nullptr;
    if (clip) {
        HIP_TRY(c, c->d_ode_ub.reserve((size_t)2 * ncf));
        HIP_TRY(c, hipMemcpyAsync(c->d_ode_ub.p, ul, (size_t)ncf * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->d_ode_ub.p + ncf, uu, (size_t)ncf * 8, hipMemcpyHostToDevice, c->stream));
    }
    // state rows against [E | E' | D | Edel ..]: x~, h x~', D x and the delayed states from one launch; free controls against [E | Edel ..]
    const emi::InterpOpArgs ps{(const double*)dX, c->d_odel_ops.p, Zs, B * ns, M, lds, ldk, lds};
    HIP_TRY(c, emi::launch_interp_op(ps, c->stream));
    const emi::InterpOpArgs pc{(const double*)dU, c->d_odel_opc.p, Zc, B * ncf, M, ldc, ldk, ldc};
    HIP_TRY(c, emi::launch_interp_op(pc, c->stream));
    emi::OdeResidDelayArgs<double> r;
    r.Zs = Zs; r.Zc = Zc; r.tq = c->d_ode_tq.p; r.scale = c->d_ode_tq.p + np;
    r.ul = clip ? c->d_ode_ub.p : nullptr; r.uu = clip ? c->d_ode_ub.p + ncf : nullptr;
    r.eta = eta; r.M = M; r.B = B; r.lds = lds; r.ldc = ldc; r.ncf = ncf; r.ns = ns; r.xh = c->xh; r.uh = c->uh; r.h = h;
    for (int i = 0; i < EMI_MAX_PARAMS; ++i) r.P.p[i] = c->params[i];
    if (c->rtc) HIP_TRY(c, emi::rtc_launch_ode_resid_delay(c->rtc, r, c->stream));
    else HIP_TRY(c, emi::launch_ode_resid_delay(c->model, r, c->stream));
    const emi::OdeFinishArgs f{(const double*)dX, Zs, eta, (double*)dErr, B, M, ns, lds, 2 * np, h};
    HIP_TRY(c, emi::launch_ode_finish(f, c->stream));
    return EMI_OK;
}

}  // namespace

extern "C" {

int emi_interp_dev(emi_ctx_t c, int K, int N, int ldk, const void* dOP, const void* dV, int R, int ldo, void* dOut) {
    if (!c) return EMI_ERR_ARG;
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "emi_interp_dev: f64 contexts only");
    if (K < 2 || N < 1 || R < 0 || ldk < K || ldk % 2 != 0 || ldo < N || !dOP || ((size_t)dOP & 15) != 0 || (R > 0 && (!dV || !dOut)))
        return fail(c, EMI_ERR_ARG, "emi_interp_dev: bad argument (K >= 2, N >= 1, R >= 0, ldk even and >= K, ldo >= N, dOP on 16 bytes)");
    if (R == 0) return EMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const emi::InterpOpArgs a{(const double*)dV, (const double*)dOP, (double*)dOut, R, K, N, ldk, ldo};
    HIP_TRY(c, emi::launch_interp_op(a, c->stream));
    return EMI_OK;
}

int emi_ode_error_dev(emi_ctx_t c, const void* dX, const void* dU, const double* ul, const double* uu, void* dEta, void* dErr) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ode_ready(c, "emi_ode_error_dev"));
    if (!dX || (c->nc > 0 && !dU) || !dErr || (ul == nullptr) != (uu == nullptr)) return fail(c, EMI_ERR_ARG, "emi_ode_error_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    EMI_TRY(ode_operator(c));
    const int M = c->M, B = c->B, ns = c->ns, nc = c->nc, nq = M - 1, np = 5 * nq, ldk = M + (M & 1), lds = 2 * np + M;
    const double h = (c->tf - c->t0) / 2.0;
    const size_t nZs = (size_t)B * ns * lds, nZc = (size_t)B * nc * np, nEta = (size_t)B * ns * nq;
    HIP_TRY(c, c->d_ode_ws.reserve(nZs + nZc + nEta));
    double *Zs = c->d_ode_ws.p, *Zc = Zs + nZs, *eta = dEta ? (double*)dEta : Zc + nZc;
    const bool clip = ul && nc > 0;
    if (clip) {
        HIP_TRY(c, c->d_ode_ub.reserve((size_t)2 * nc));
        // pageable host memory: the copies are staged before the calls return, the caller's arrays are free again
        HIP_TRY(c, hipMemcpyAsync(c->d_ode_ub.p, ul, (size_t)nc * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->d_ode_ub.p + nc, uu, (size_t)nc * 8, hipMemcpyHostToDevice, c->stream));
    }
    // state rows against [E | E' | D]: x~, h x~' and D x from one launch; control rows against E alone
    const emi::InterpOpArgs ps{(const double*)dX, c->d_ode_op.p, Zs, B * ns, M, lds, ldk, lds};
    HIP_TRY(c, emi::launch_interp_op(ps, c->stream));
    if (nc > 0) {
        const emi::InterpOpArgs pc{(const double*)dU, c->d_ode_op.p, Zc, B * nc, M, np, ldk, np};
        HIP_TRY(c, emi::launch_interp_op(pc, c->stream));
    }
    emi::OdeResidArgs<double> r;
    r.Zs = Zs; r.Zc = Zc; r.tq = c->d_ode_tq.p; r.scale = c->d_ode_tq.p + np;
    r.ul = clip ? c->d_ode_ub.p : nullptr; r.uu = clip ? c->d_ode_ub.p + nc : nullptr;
    r.eta = eta; r.M = M; r.B = B; r.lds = lds; r.ldc = np; r.h = h;
    for (int i = 0; i < EMI_MAX_PARAMS; ++i) r.P.p[i] = c->params[i];
    const double* tab = param_rows<double>(c, 0);      // per-instance parameter table: the tabled residual kernel
    if (tab && c->rtc) HIP_TRY(c, emi::rtc_launch_ode_resid_tab(c->rtc, r, tab, c->stream));
    else if (tab) HIP_TRY(c, emi::launch_ode_resid_tab(c->model, r, tab, c->stream));
    else if (c->rtc) HIP_TRY(c, emi::rtc_launch_ode_resid(c->rtc, r, c->stream));
    else HIP_TRY(c, emi::launch_ode_resid(c->model, r, c->stream));
    const emi::OdeFinishArgs f{(const double*)dX, Zs, eta, (double*)dErr, B, M, ns, lds, 2 * np, h};
    HIP_TRY(c, emi::launch_ode_finish(f, c->stream));
    return EMI_OK;
}

int emi_ode_error_host(emi_ctx_t c, const double* X, const double* U, const double* ul, const double* uu, double* Eta, double* Err) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ode_ready(c, "emi_ode_error_host"));
    if (!X || (c->nc > 0 && !U) || !Err) return fail(c, EMI_ERR_ARG, "emi_ode_error_host: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HostStager s(c);
    const size_t B = (size_t)c->B, M = (size_t)c->M;
    const void *dX = s.place(X, B * c->ns * M * 8, true, false), *dU = s.place(U, B * c->nc * M * 8, true, false);
    void *dEta = s.place(Eta, B * c->ns * (M - 1) * 8, false, true), *dErr = s.place(Err, B * 8, false, true);
    HOST_STAGED_TRY(s, emi_ode_error_dev(c, dX, dU, ul, uu, dEta, dErr));
    return s.finish();
}

int emi_ode_error_total_dev(emi_ctx_t c, const void* dX, const void* dU, const double* ul, const double* uu, void* dEta, void* dErr) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ode_ready(c, "emi_ode_error_total_dev", true));
    if (c->nch == 0) return emi_ode_error_dev(c, dX, dU, ul, uu, dEta, dErr);      // no delays: the plain call, launch for launch
    if (!dX || !dU || !dErr || (ul == nullptr) != (uu == nullptr)) return fail(c, EMI_ERR_ARG, "emi_ode_error_total_dev: null argument");
    return ode_error_delayed(c, dX, dU, ul, uu, dEta, dErr);
}

int emi_ode_error_total_host(emi_ctx_t c, const double* X, const double* U, const double* ul, const double* uu, double* Eta, double* Err) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ode_ready(c, "emi_ode_error_total_host", true));
    if (c->nch == 0) return emi_ode_error_host(c, X, U, ul, uu, Eta, Err);
    if (!X || !U || !Err || (ul == nullptr) != (uu == nullptr)) return fail(c, EMI_ERR_ARG, "emi_ode_error_total_host: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HostStager s(c);
    const size_t B = (size_t)c->B, M = (size_t)c->M;
    const void *dX = s.place(X, B * c->ns * M * 8, true, false), *dU = s.place(U, B * (c->nc - c->nch) * M * 8, true, false);
    void *dEta = s.place(Eta, B * c->ns * (M - 1) * 8, false, true), *dErr = s.place(Err, B * 8, false, true);
    HOST_STAGED_TRY(s, ode_error_delayed(c, dX, dU, ul, uu, dEta, dErr));
    return s.finish();
}

}  // extern "C"
