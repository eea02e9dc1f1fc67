// emi_api_adjoint.hip -- the adjoint pass of the C ABI: Lagrangian gradient and KKT certificate (kernels: emi_adjoint.hip), plain
// and for contexts with delays (the *_total_* forms), device and host forms.
#include "emi_ctx.hpp"

using namespace emi_api;

extern "C" {

// a null context on a box without a device is "no device", not a bad argument: there is no host path to fall back to
static int adj_null_ctx() {
    int n = 0;
    return (hipGetDeviceCount(&n) != hipSuccess || n <= 0) ? EMI_ERR_NO_DEVICE : EMI_ERR_ARG;
}

// total: the caller is one of the emi_*_total_* entry points, which fold the delayed values' adjoints onto their sources
static int adj_ready(emi_ctx_t c, const char* who, bool total = false) {
    int st = ready(c);
    if (st) return st;
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: fp32 contexts have no adjoint pass (the certificate is an fp64 figure)", who);
    if (c->nch > 0 && !total)
        return fail(c, EMI_ERR_UNSUPPORTED, "%s: contexts with delays (emi_set_delays) take emi_lagr_grad_total_* / emi_kkt_certificate_total_*, "
                    "which fold the adjoints of the delayed values onto their sources", who);
    if (c->points_only) return fail(c, EMI_ERR_STATE, "%s: the mesh has no differentiation matrix (points-only mesh)", who);
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->adj_dirty) {
        const int M = c->M, ldt = M + (M & 1);
        if ((st = ensure(c, c->d_adjDT, (size_t)M * ldt * 8))) return st;
        HIP_TRY(c, emi::launch_adjoint_transpose((const double*)c->d_D.p, (double*)c->d_adjDT.p, M, ldt, ldt, 1, false, c->stream));
        c->adj_dirty = false;
    }
    if (c->nch > 0 && (c->adjw_dirty || c->delay_dirty)) {      // (an adjoint call may be the first use of W on this mesh)
        const int M = c->M, ldt = M + (M & 1), nd = std::max(c->xh - 1, c->uh);
        if ((st = ensure_delay_matrices(c))) return st;
        if ((st = ensure(c, c->d_adjWT, (size_t)M * nd * ldt * 8))) return st;
        HIP_TRY(c, emi::launch_adjoint_transpose((const double*)c->d_W.p, (double*)c->d_adjWT.p, M, ldt, nd * ldt, nd, true, c->stream));
        c->adjw_dirty = false;
    }
    if (c->adj_pvars != c->pvars || (!c->pvars.empty() && !c->d_adj_pvars.p)) {
        if ((st = upload_bytes(c, c->d_adj_pvars, c->pvars.data(), c->pvars.size() * sizeof(int)))) return st;
        c->adj_pvars = c->pvars;
    }
    return EMI_OK;
}

// G[B][ns+nc][M] on the node variables of the model (the extended ones of a context with delays); the context is adj_ready
static int lagr_grad_launch(emi_ctx_t c, const void* dVALS, const void* dLamF, const void* dLamC, double sigma, void* dG) {
    int st;
    emi::AdjointArgs a;
    a.VALS = (const double*)dVALS; a.lamF = (const double*)dLamF; a.lamC = np_total(c) > 0 ? (const double*)dLamC : nullptr;
    a.DT = (const double*)c->d_adjDT.p; a.pvars = (const int*)c->d_adj_pvars.p; a.G = (double*)dG;
    a.B = c->B; a.M = c->M; a.ldt = c->M + (c->M & 1); a.ns = c->ns; a.nc = c->nc;
    a.np_table = c->np; a.np_traced = c->np_model; a.pw = c->np_model > 0 ? (int)c->pvars.size() : 0;
    a.px = c->px; a.py = c->py; a.nvals = nvals_of(c); a.sigma = sigma; a.add_op = 1;
    if (!emi::adjoint_side_by_side(c->B, c->ns, c->M)) {
        HIP_TRY(c, emi::launch_adjoint_op(a, c->stream));
        HIP_TRY(c, emi::launch_adjoint_nodes(a, c->stream));
        return EMI_OK;
    }
    // Large batches: the product (matrix pipe) on the second stream BESIDE the node kernel (HBM) -- they share nothing until the last
    // addition.  The product writes its own [B][ns][M] block; a third, short kernel adds it onto the state rows: the same last
    // addition as in the back-to-back form, so both forms give the same bits.
    if ((st = need_stream2(c))) return st;
    if ((st = ensure(c, c->d_adj_op, (size_t)c->B * c->ns * c->M * 8))) return st;
    emi::AdjointArgs op = a;
    op.G = (double*)c->d_adj_op.p;
    op.nc = 0;                                       // rows (instance * ns + state) of the block
    a.add_op = 0;
    HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));          // the inputs (and the previous call's last addition) are done
    HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    HIP_TRY(c, emi::launch_adjoint_op(op, c->stream2));
    HIP_TRY(c, hipEventRecord(c->ev_join, c->stream2));
    HIP_TRY(c, emi::launch_adjoint_nodes(a, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    HIP_TRY(c, emi::launch_adjoint_add((const double*)c->d_adj_op.p, (double*)dG, c->B, c->ns, c->ns + c->nc, c->M, c->stream));
    return EMI_OK;
}

int emi_lagr_grad_dev(emi_ctx_t c, const void* dVALS, const void* dLamF, const void* dLamC, double sigma, void* dG) {
    if (!c) return adj_null_ctx();
    int st = adj_ready(c, "emi_lagr_grad");
    if (st) return st;
    if (!dVALS || !dLamF || !dG || (np_total(c) > 0 && !dLamC)) return fail(c, EMI_ERR_ARG, "emi_lagr_grad: null device pointer");
    return lagr_grad_launch(c, dVALS, dLamF, dLamC, sigma, dG);
}

// The gradient with respect to the trajectory of a context with delays.  Gx on the extended variables as above (workspace), then
// per class of sources one product on the matrix pipe: rows (instance, source), K = the node ranges of the delay indices one after
// the other against the transposed stack of W, last addition Gx[source] + product, stored into the caller's G[B][ns+ncf][M].
// One stream, back to back; every entry has one writer and a fixed summation order.
int emi_lagr_grad_total_dev(emi_ctx_t c, const void* dVALS, const void* dLamF, const void* dLamC, double sigma, void* dG, void* dGdel) {
    if (!c) return adj_null_ctx();
    int st = adj_ready(c, "emi_lagr_grad_total", true);
    if (st) return st;
    if (!dVALS || !dLamF || !dG || (np_total(c) > 0 && !dLamC)) return fail(c, EMI_ERR_ARG, "emi_lagr_grad_total: null device pointer");
    if (c->nch == 0) return lagr_grad_launch(c, dVALS, dLamF, dLamC, sigma, dG);
    const int M = c->M, B = c->B, ns = c->ns, nv = c->ns + c->nc, ncf = c->nc - c->nch, nf = ns + ncf, ldt = M + (M & 1);
    const int nd = std::max(c->xh - 1, c->uh), nxs = std::max(c->xh - 1, 0);
    if ((st = ensure(c, c->d_adj_Gx, (size_t)B * nv * M * 8))) return st;
    const double* Gx = (const double*)c->d_adj_Gx.p;
    if ((st = lagr_grad_launch(c, dVALS, dLamF, dLamC, sigma, c->d_adj_Gx.p))) return st;
    const size_t row = (size_t)M * 8;
    // rows [row0, row0 + n) of every instance of Gx -> rows [dst0, ..) of a [B][dst_rows][M] array
    auto copy_rows = [&](void* dst, int dst_rows, int dst0, int row0, int n) {
        return hipMemcpy2DAsync((double*)dst + (size_t)dst0 * M, (size_t)dst_rows * row, Gx + (size_t)row0 * M, (size_t)nv * row, (size_t)n * row, B,
                                hipMemcpyDeviceToDevice, c->stream);
    };
    auto fold = [&](int src0, int nsrc, int slot0, int nseg) {
        emi::AdjointOpArgs o;
        o.A = Gx; o.Bop = (const double*)c->d_adjWT.p; o.add = Gx; o.out = (double*)dG;
        o.R = B * nsrc; o.rpi = nsrc; o.M = M; o.ldt = ldt; o.nseg = nseg; o.ldb = nd * ldt;
        o.a_inst = nv; o.a_row0 = slot0; o.a_seg = nsrc; o.out_inst = nf; o.out_row0 = src0; o.add_inst = nv; o.add_row0 = src0;
        return emi::launch_adjoint_product(o, c->adj_fold_tile, c->stream);
    };
    if (nxs > 0) HIP_TRY(c, fold(0, ns, nf, nxs));              // states: copies x(t - i dt), i = 1 .. xh - 1, in slots nf + (i - 1) ns + state
    else HIP_TRY(c, copy_rows(dG, nf, 0, 0, ns));
    if (c->uh > 0) HIP_TRY(c, fold(ns, ncf, nf + nxs * ns, c->uh));   // controls: u(t - i dt), i = 1 .. uh, behind the states' copies
    else HIP_TRY(c, copy_rows(dG, nf, ns, ns, ncf));
    if (dGdel) HIP_TRY(c, copy_rows(dGdel, c->nch, 0, nf, c->nch));
    return EMI_OK;
}

// total: emi_lagr_grad_total_host (G on the free variables, Gdel the adjoints of the delayed values); a context the plain form
// accepts has no delayed values, so the sizes below are the same figures for both
static int lagr_grad_host(emi_ctx_t c, bool total, const double* VALS, const double* LamF, const double* LamC, double sigma, double* G,
                          double* Gdel) {
    if (!c) return adj_null_ctx();
    const char* who = total ? "emi_lagr_grad_total_host" : "emi_lagr_grad_host";
    int st = adj_ready(c, who, total);
    if (st) return st;
    if (!VALS || !LamF || !G || (np_total(c) > 0 && !LamC)) return fail(c, EMI_ERR_ARG, "%s: null pointer", who);
    const size_t M = c->M, B = c->B, nf = c->ns + c->nc - c->nch;
    const size_t nV = B * nvals_of(c) * M, nF = B * c->ns * M, nC = B * np_total(c) * M, nG = B * nf * M, nGd = B * c->nch * M;
    c->keep.written(c->s_VALS.p);           // the caller's VALS replace what an evaluation left in the staging buffer
    if ((st = upload_real(c, c->s_VALS, VALS, nV))) return st;
    c->keep.written(c->s_VALS.p);
    if ((st = upload_real(c, c->s_LF, LamF, nF))) return st;
    if (nC && (st = upload_real(c, c->s_LC, LamC, nC))) return st;
    if ((st = ensure(c, c->s_G, nG * 8))) return st;
    const bool del = total && Gdel && nGd > 0;
    if (del && (st = ensure(c, c->s_Gdel, nGd * 8))) return st;
    if ((st = total ? emi_lagr_grad_total_dev(c, c->s_VALS.p, c->s_LF.p, c->s_LC.p, sigma, c->s_G.p, del ? c->s_Gdel.p : nullptr)
                    : emi_lagr_grad_dev(c, c->s_VALS.p, c->s_LF.p, c->s_LC.p, sigma, c->s_G.p)))
        return st;
    if (del && (st = download_real(c, Gdel, c->s_Gdel.p, nGd))) return st;
    return download_real(c, G, c->s_G.p, nG);
}

int emi_lagr_grad_total_host(emi_ctx_t c, const double* VALS, const double* LamF, const double* LamC, double sigma, double* G, double* Gdel) {
    return lagr_grad_host(c, true, VALS, LamF, LamC, sigma, G, Gdel);
}

int emi_lagr_grad_host(emi_ctx_t c, const double* VALS, const double* LamF, const double* LamC, double sigma, double* G) {
    return lagr_grad_host(c, false, VALS, LamF, LamC, sigma, G, nullptr);
}

// the certificate on the free variables: G, U, zl, zu hold nf = ns + nc - n_delayed variables (total: the folded gradient)
static int kkt_certificate_launch(emi_ctx_t c, bool total, const void* dX, const void* dU, const void* dRES, const void* dVALS,
                                  const void* dLamF, const void* dLamC, double sigma, const void* dZl, const void* dZu, int nsets,
                                  const double* cl, const double* cu, void* dCert, void* dG, void* dGdel) {
    if (!c) return adj_null_ctx();
    int st = adj_ready(c, total ? "emi_kkt_certificate_total" : "emi_kkt_certificate", total);
    if (st) return st;
    const int np = np_total(c), ncf = c->nc - c->nch;
    if (!dX || !dU || !dRES || !dVALS || !dLamF || !dZl || !dZu || !dCert || (np > 0 && (!dLamC || !cl || !cu)))
        return fail(c, EMI_ERR_ARG, "emi_kkt_certificate: null pointer");
    if (nsets != 1 && nsets != c->B) return fail(c, EMI_ERR_ARG, "emi_kkt_certificate: %d bound sets, batch is %d", nsets, c->B);
    if (!dG) {
        if ((st = ensure(c, c->d_adj_G, (size_t)c->B * (c->ns + ncf) * c->M * 8))) return st;
        dG = c->d_adj_G.p;
    }
    if (np > 0) {
        if ((st = ensure(c, c->d_adj_c, (size_t)2 * np * 8))) return st;
        // pageable host memory: the copies are staged before the calls return, the caller's arrays are free again
        HIP_TRY(c, hipMemcpyAsync(c->d_adj_c.p, cl, (size_t)np * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync((double*)c->d_adj_c.p + np, cu, (size_t)np * 8, hipMemcpyHostToDevice, c->stream));
    }
    if ((st = total ? emi_lagr_grad_total_dev(c, dVALS, dLamF, dLamC, sigma, dG, dGdel) : emi_lagr_grad_dev(c, dVALS, dLamF, dLamC, sigma, dG)))
        return st;
    emi::CertArgs a;
    a.X = (const double*)dX; a.U = (const double*)dU; a.RES = (const double*)dRES; a.VALS = (const double*)dVALS;
    a.lamF = (const double*)dLamF; a.lamC = np > 0 ? (const double*)dLamC : nullptr; a.G = (const double*)dG;
    a.zl = (const double*)dZl; a.zu = (const double*)dZu;
    a.cl = (const double*)c->d_adj_c.p; a.cu = np > 0 ? (const double*)c->d_adj_c.p + np : nullptr;
    a.cert = (double*)dCert;
    a.B = c->B; a.M = c->M; a.ns = c->ns; a.nc = ncf; a.np = np; a.nres = nres_of(c); a.nvals = nvals_of(c); a.nsets = nsets;
    a.ncg = c->ns + c->nc;                             // gmax: a scale figure, over the cost gradient on all node variables
    a.sigma = sigma;
    HIP_TRY(c, emi::launch_kkt_certificate(a, c->stream));
    return EMI_OK;
}

int emi_kkt_certificate_dev(emi_ctx_t c, const void* dX, const void* dU, const void* dRES, const void* dVALS, const void* dLamF,
                            const void* dLamC, double sigma, const void* dZl, const void* dZu, int nsets, const double* cl,
                            const double* cu, void* dCert, void* dG) {
    return kkt_certificate_launch(c, false, dX, dU, dRES, dVALS, dLamF, dLamC, sigma, dZl, dZu, nsets, cl, cu, dCert, dG, nullptr);
}

int emi_kkt_certificate_total_dev(emi_ctx_t c, const void* dX, const void* dU, const void* dRES, const void* dVALS, const void* dLamF,
                                  const void* dLamC, double sigma, const void* dZl, const void* dZu, int nsets, const double* cl,
                                  const double* cu, void* dCert, void* dG, void* dGdel) {
    return kkt_certificate_launch(c, true, dX, dU, dRES, dVALS, dLamF, dLamC, sigma, dZl, dZu, nsets, cl, cu, dCert, dG, dGdel);
}

static int kkt_certificate_host(emi_ctx_t c, bool total, const double* X, const double* U, const double* LamF, const double* LamC,
                                double sigma, const double* zl, const double* zu, int nsets, const double* cl, const double* cu,
                                double* cert, double* G, double* Gdel) {
    if (!c) return adj_null_ctx();
    int st = adj_ready(c, total ? "emi_kkt_certificate_total_host" : "emi_kkt_certificate_host", total);
    if (st) return st;
    const int np = np_total(c);
    if (!X || !U || !LamF || !zl || !zu || !cert || (np > 0 && (!LamC || !cl || !cu)))
        return fail(c, EMI_ERR_ARG, "emi_kkt_certificate_host: null pointer");
    if (nsets != 1 && nsets != c->B) return fail(c, EMI_ERR_ARG, "emi_kkt_certificate_host: %d bound sets, batch is %d", nsets, c->B);
    const size_t M = c->M, B = c->B, ncf = c->nc - c->nch, nv = c->ns + ncf;      // the free variables: what X, U, zl, zu and G hold
    const size_t nX = B * c->ns * M, nU = B * ncf * M, nR = B * nres_of(c) * M, nV = B * nvals_of(c) * M, nC = B * np * M, nG = B * nv * M;
    const size_t nGd = B * c->nch * M;
    const bool del = total && Gdel && nGd > 0;
    if (del && (st = ensure(c, c->s_Gdel, nGd * 8))) return st;
    if ((st = upload_real(c, c->s_X, X, nX))) return st;
    if ((st = upload_real(c, c->s_U, U, nU))) return st;
    if ((st = upload_real(c, c->s_LF, LamF, nX))) return st;
    if (nC && (st = upload_real(c, c->s_LC, LamC, nC))) return st;
    if ((st = upload_real(c, c->s_zl, zl, (size_t)nsets * nv * M))) return st;
    if ((st = upload_real(c, c->s_zu, zu, (size_t)nsets * nv * M))) return st;
    if ((st = ensure(c, c->s_RES, nR * 8))) return st;
    if ((st = ensure_vals_staging(c, nV * 8))) return st;
    if ((st = ensure(c, c->s_COST, B * 8))) return st;
    if ((st = ensure(c, c->s_G, nG * 8))) return st;
    if ((st = ensure(c, c->s_cert, B * 6 * 8))) return st;
    if ((st = emi_eval_dev(c, c->s_X.p, c->s_U.p, c->s_RES.p, c->s_VALS.p, c->s_COST.p, EMI_EVAL_ALL))) return st;
    if ((st = kkt_certificate_launch(c, total, c->s_X.p, c->s_U.p, c->s_RES.p, c->s_VALS.p, c->s_LF.p, c->s_LC.p, sigma, c->s_zl.p, c->s_zu.p,
                                     nsets, cl, cu, c->s_cert.p, c->s_G.p, del ? c->s_Gdel.p : nullptr))) return st;
    if ((st = download_real(c, cert, c->s_cert.p, B * 6))) return st;
    if (G && (st = download_real(c, G, c->s_G.p, nG))) return st;
    if (del && (st = download_real(c, Gdel, c->s_Gdel.p, nGd))) return st;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}

int emi_kkt_certificate_host(emi_ctx_t c, const double* X, const double* U, const double* LamF, const double* LamC, double sigma,
                             const double* zl, const double* zu, int nsets, const double* cl, const double* cu, double* cert,
                             double* G) {
    return kkt_certificate_host(c, false, X, U, LamF, LamC, sigma, zl, zu, nsets, cl, cu, cert, G, nullptr);
}

int emi_kkt_certificate_total_host(emi_ctx_t c, const double* X, const double* U, const double* LamF, const double* LamC, double sigma,
                                   const double* zl, const double* zu, int nsets, const double* cl, const double* cu, double* cert,
                                   double* G, double* Gdel) {
    return kkt_certificate_host(c, true, X, U, LamF, LamC, sigma, zl, zu, nsets, cl, cu, cert, G, Gdel);
}

}  // extern "C"
