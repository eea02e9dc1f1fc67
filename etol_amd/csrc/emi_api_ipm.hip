// emi_api_ipm.hip -- the interior-point part of the C ABI: the array arithmetic of an iteration over [instance][node] (emi_ipm.hip)
// with its _host forms, the lock-step solve of a context's whole batch (driver: emi_ipm_solve.hip) and the mesh ladder over it
// (kernels and driver: emi_ipm_ladder.hip), with and without refinement.
#include "emi_ctx.hpp"
#include "emi_restart_book.hpp"

using namespace emi_api;

namespace {

int ipm_check(emi_ctx_t c, const char* what) {
    if (c->M <= 0 || c->model < 0 || c->B <= 0) return fail(c, EMI_ERR_STATE, "%s: mesh, model and batch must be set", what);
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: f64 contexts only", what);
    if (c->nch > 0) return fail(c, EMI_ERR_UNSUPPORTED, "%s: contexts with delays are not taken", what);
    if (c->ns + c->nc > 16) return fail(c, EMI_ERR_UNSUPPORTED, "%s: up to 16 variables per node (this model has %d)", what, c->ns + c->nc);
    return EMI_OK;
}

// the path-row lists by row and by variable on the device (built once per list)
int ipm_lists(emi_ctx_t c, const char* what, emi::IpmArgs& a) {
    const int nv = c->ns + c->nc, np = np_total(c);
    std::vector<int> ptr, var, ent;
    EMI_TRY(path_row_list(c, what, ptr, var, ent));
    std::vector<int> key = {nv, np, nvals_of(c)};
    key.insert(key.end(), ptr.begin(), ptr.end());
    key.insert(key.end(), var.begin(), var.end());
    key.insert(key.end(), ent.begin(), ent.end());
    const int n = (int)var.size();
    if (key != c->ipm_key) {
        std::vector<int> all(ptr);                                  // rptr [np + 1]
        all.insert(all.end(), var.begin(), var.end());              // rvar [n]
        all.insert(all.end(), ent.begin(), ent.end());              // rent [n]
        std::vector<int> vptr(nv + 1, 0), vrow, vent;
        for (int v = 0; v < nv; ++v) {
            for (int j = 0; j < np; ++j)
                for (int t = ptr[j]; t < ptr[j + 1]; ++t)
                    if (var[t] == v) { vrow.push_back(j); vent.push_back(ent[t]); }
            vptr[v + 1] = (int)vrow.size();
        }
        all.insert(all.end(), vptr.begin(), vptr.end());
        all.insert(all.end(), vrow.begin(), vrow.end());
        all.insert(all.end(), vent.begin(), vent.end());
        HIP_TRY(c, hipStreamSynchronize(c->stream));        // a launch in flight may still read the old lists
        HIP_TRY(c, c->ipm_lists.reserve(all.size()));
        HIP_TRY(c, hipMemcpyAsync(c->ipm_lists.p, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));        // (the source is a local)
        c->ipm_key = key;
        c->ipm_npairs = n;
    }
    const int* p = c->ipm_lists.p;
    a.rptr = p; a.rvar = p + np + 1; a.rent = a.rvar + n;
    a.vptr = a.rent + n; a.vrow = a.vptr + nv + 1; a.vent = a.vrow + n;
    return EMI_OK;
}

// sizes, bounds and per-instance scalars of a call; the row bounds go to the device when they differ from what is there
int ipm_common(emi_ctx_t c, const char* what, const emi_ipm_bounds_t* bd, const void* dPar, emi::IpmArgs& a) {
    const int np = np_total(c);
    a.B = c->B; a.M = c->M; a.ns = c->ns; a.nc = c->nc; a.np = np; a.nvals = nvals_of(c);
    a.par = (const double*)dPar;
    if (!bd) return EMI_OK;
    if (!bd->zl || !bd->zu || (bd->nsets != 1 && bd->nsets != c->B) || (np > 0 && (!bd->cl || !bd->cu)))
        return fail(c, EMI_ERR_ARG, "%s: bad bounds (zl, zu [nsets][nv][M] with nsets 1 or the batch; cl, cu [np])", what);
    a.zl = (const double*)bd->zl; a.zu = (const double*)bd->zu; a.nsets = bd->nsets;
    if (np > 0) {
        std::vector<double> h((size_t)5 * np);
        for (int j = 0; j < np; ++j) {
            const double cs = bd->cscale ? bd->cscale[j] : 1.0;
            if (!(cs > 0.0)) return fail(c, EMI_ERR_ARG, "%s: cscale[%d] must be positive", what, j);
            h[j] = bd->cl[j]; h[np + j] = bd->cu[j];
            h[2 * np + j] = bd->cl[j] > -1e19 ? cs * bd->cl[j] : bd->cl[j];
            h[3 * np + j] = bd->cu[j] < 1e19 ? cs * bd->cu[j] : bd->cu[j];
            h[4 * np + j] = cs;
        }
        if (h != c->ipm_crow_h || !c->ipm_crow.p) {
            // new bounds (once per problem, not per iteration): the launches that read the old values are drained before the buffer
            // may move, and the copy is complete before its source is touched again
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, c->ipm_crow.reserve(h.size()));
            c->ipm_crow_h = h;
            HIP_TRY(c, hipMemcpyAsync(c->ipm_crow.p, c->ipm_crow_h.data(), h.size() * 8, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        a.crow = c->ipm_crow.p;
    }
    return EMI_OK;
}

int ipm_partials(emi_ctx_t c, emi::IpmArgs& a) {
    HIP_TRY(c, c->ipm_part.reserve((size_t)c->B * emi::ipm_chunks(c->M) * emi::IPM_MAX_PARTIALS));
    a.part = c->ipm_part.p;
    return EMI_OK;
}

bool ipm_has_point(const emi_ipm_point_t* p, int nc, int np) { return p && p->X && (nc == 0 || p->U) && (np == 0 || (p->S && p->E1 && p->E2)); }
bool ipm_has_duals(const emi_ipm_duals_t* d, int np) {
    return d && d->LamF && d->ZL && d->ZU && (np == 0 || (d->Y && d->VL && d->VU && d->W1 && d->W2));
}
bool ipm_has_step(const emi_ipm_step_t* s, int np) {
    return s && s->DZLam && s->DZL && s->DZU && (np == 0 || (s->DS && s->DY && s->DE1 && s->DE2 && s->DVL && s->DVU && s->DW1 && s->DW2));
}
bool ipm_has_elim(const emi_ipm_elim_t* e, int np) { return e && e->Sigma && (np == 0 || (e->SigT && e->SigS && e->RhatS && e->Rt)); }
void ipm_set_point(emi::IpmArgs& a, const emi_ipm_point_t* p) { a.X = (double*)p->X; a.U = (double*)p->U; a.S = (double*)p->S; a.E1 = (double*)p->E1; a.E2 = (double*)p->E2; }
void ipm_set_trial(emi::IpmArgs& a, const emi_ipm_point_t* p) { a.tX = (double*)p->X; a.tU = (double*)p->U; a.tS = (double*)p->S; a.tE1 = (double*)p->E1; a.tE2 = (double*)p->E2; }
void ipm_set_duals(emi::IpmArgs& a, const emi_ipm_duals_t* d) {
    a.LF = (double*)d->LamF; a.Y = (double*)d->Y; a.ZL = (double*)d->ZL; a.ZU = (double*)d->ZU;
    a.VL = (double*)d->VL; a.VU = (double*)d->VU; a.W1 = (double*)d->W1; a.W2 = (double*)d->W2;
}
void ipm_set_step(emi::IpmArgs& a, const emi_ipm_step_t* s) {
    a.DZ = (double*)s->DZLam; a.DS = (double*)s->DS; a.DY = (double*)s->DY; a.DE1 = (double*)s->DE1; a.DE2 = (double*)s->DE2;
    a.DZL = (double*)s->DZL; a.DZU = (double*)s->DZU; a.DVL = (double*)s->DVL; a.DVU = (double*)s->DVU; a.DW1 = (double*)s->DW1; a.DW2 = (double*)s->DW2;
}
void ipm_set_elim(emi::IpmArgs& a, const emi_ipm_elim_t* e) {
    a.Sigma = (double*)e->Sigma; a.SigT = (double*)e->SigT; a.SigS = (double*)e->SigS; a.RhatS = (double*)e->RhatS; a.Rt = (double*)e->Rt;
}

struct IpmSizes {
    size_t X, U, row, var, kkt, res, vals, bnd, inst;
    IpmSizes(emi_ctx_t c, int nsets) {
        const size_t B = (size_t)c->B, M = (size_t)c->M, nv = (size_t)(c->ns + c->nc), np = (size_t)np_total(c);
        X = B * c->ns * M * 8; U = B * c->nc * M * 8; row = B * np * M * 8; var = B * nv * M * 8; kkt = B * (nv + c->ns) * M * 8;
        res = B * (c->ns + np) * M * 8; vals = B * (size_t)nvals_of(c) * M * 8; bnd = (size_t)std::max(nsets, 0) * nv * M * 8; inst = B * 8;
    }
};
emi_ipm_point_t stage_point(HostStager& s, const IpmSizes& z, const emi_ipm_point_t* p, bool in, bool out) {
    emi_ipm_point_t d{};
    if (!p) return d;
    d.X = s.place(p->X, z.X, in, out); d.U = s.place(p->U, z.U, in, out);
    d.S = s.place(p->S, z.row, in, out); d.E1 = s.place(p->E1, z.row, in, out); d.E2 = s.place(p->E2, z.row, in, out);
    return d;
}
emi_ipm_duals_t stage_duals(HostStager& s, const IpmSizes& z, const emi_ipm_duals_t* p, bool in, bool out) {
    emi_ipm_duals_t d{};
    if (!p) return d;
    d.LamF = s.place(p->LamF, z.X, in, out); d.Y = s.place(p->Y, z.row, in, out);
    d.ZL = s.place(p->ZL, z.var, in, out); d.ZU = s.place(p->ZU, z.var, in, out);
    d.VL = s.place(p->VL, z.row, in, out); d.VU = s.place(p->VU, z.row, in, out);
    d.W1 = s.place(p->W1, z.row, in, out); d.W2 = s.place(p->W2, z.row, in, out);
    return d;
}
// dz_in / dz_out: the solved step goes in and comes back with the fixed variables zeroed; the rest as `in` / `out` say
emi_ipm_step_t stage_step(HostStager& s, const IpmSizes& z, const emi_ipm_step_t* p, bool dz_in, bool dz_out, bool in, bool out) {
    emi_ipm_step_t d{};
    if (!p) return d;
    d.DZLam = s.place(p->DZLam, z.kkt, dz_in, dz_out);
    d.DS = s.place(p->DS, z.row, in, out); d.DY = s.place(p->DY, z.row, in, out);
    d.DE1 = s.place(p->DE1, z.row, in, out); d.DE2 = s.place(p->DE2, z.row, in, out);
    d.DZL = s.place(p->DZL, z.var, in, out); d.DZU = s.place(p->DZU, z.var, in, out);
    d.DVL = s.place(p->DVL, z.row, in, out); d.DVU = s.place(p->DVU, z.row, in, out);
    d.DW1 = s.place(p->DW1, z.row, in, out); d.DW2 = s.place(p->DW2, z.row, in, out);
    return d;
}
emi_ipm_elim_t stage_elim(HostStager& s, const IpmSizes& z, const emi_ipm_elim_t* p, bool in, bool out) {
    emi_ipm_elim_t d{};
    if (!p) return d;
    d.Sigma = s.place(p->Sigma, z.var, in, out); d.SigT = s.place(p->SigT, z.row, in, out); d.SigS = s.place(p->SigS, z.row, in, out);
    d.RhatS = s.place(p->RhatS, z.row, in, out); d.Rt = s.place(p->Rt, z.row, in, out);
    return d;
}
emi_ipm_bounds_t stage_bounds(HostStager& s, const IpmSizes& z, const emi_ipm_bounds_t* p) {
    emi_ipm_bounds_t d{};
    if (!p) return d;
    d = *p;
    d.zl = s.place(p->zl, z.bnd, true, false); d.zu = s.place(p->zu, z.bnd, true, false);
    return d;
}

}  // namespace

#define IPM_HOST_BEGIN(what, nsets)                  \
    if (!c) return EMI_ERR_ARG;                      \
    EMI_TRY(ipm_check(c, what));                     \
    HIP_TRY(c, hipSetDevice(c->device));             \
    HostStager s(c);                                 \
    const IpmSizes z(c, nsets)
#define IPM_HOST_END(call) HOST_STAGED_TRY(s, call) return s.finish()

int emi_api::ctx_ipm_launch(emi_ctx_t c, int what, const emi_ipm_bounds_t* bd, const void* dPar, emi::IpmArgs& a) {
    EMI_TRY(ipm_common(c, "emi_ipm_solve_shard_dev", bd, dPar, a));
    HIP_TRY(c, emi::launch_ipm(what, a, c->stream));
    return EMI_OK;
}

extern "C" {

int emi_ipm_reduce_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dRES, const void* dVALS, const void* dG,
                       const emi_ipm_bounds_t* bd, const void* dPar, const void* dDefRes, const void* dRowRes, const emi_ipm_elim_t* out,
                       void* dRhs) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_reduce_dev"));
    const int np = np_total(c);
    if (!ipm_has_point(pt, c->nc, np) || !ipm_has_duals(du, np) || !dRES || !dVALS || !dG || !bd || !dPar || !ipm_has_elim(out, np) || !dRhs)
        return fail(c, EMI_ERR_ARG, "emi_ipm_reduce_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_reduce_dev", bd, dPar, a));
    EMI_TRY(ipm_lists(c, "emi_ipm_reduce_dev", a));
    ipm_set_point(a, pt); ipm_set_duals(a, du); ipm_set_elim(a, out);
    a.RES = (const double*)dRES; a.VALS = (const double*)dVALS; a.G = (const double*)dG;
    a.DefRes = (const double*)dDefRes; a.RowRes = (const double*)dRowRes; a.Rhs = (double*)dRhs;
    HIP_TRY(c, emi::launch_ipm(emi::IPM_REDUCE, a, c->stream));
    return EMI_OK;
}

int emi_ipm_expand_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dVALS, const emi_ipm_bounds_t* bd,
                       const void* dPar, const emi_ipm_elim_t* el, const void* dRs, const emi_ipm_step_t* st, void* dScal) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_expand_dev"));
    const int np = np_total(c);
    if (!ipm_has_point(pt, c->nc, np) || !ipm_has_duals(du, np) || !dVALS || !bd || !dPar || !ipm_has_elim(el, np) || !ipm_has_step(st, np) || !dScal)
        return fail(c, EMI_ERR_ARG, "emi_ipm_expand_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_expand_dev", bd, dPar, a));
    EMI_TRY(ipm_lists(c, "emi_ipm_expand_dev", a));
    EMI_TRY(ipm_partials(c, a));
    ipm_set_point(a, pt); ipm_set_duals(a, du); ipm_set_elim(a, el); ipm_set_step(a, st);
    a.VALS = (const double*)dVALS; a.rs = (const double*)dRs; a.out = (double*)dScal;
    HIP_TRY(c, emi::launch_ipm(emi::IPM_EXPAND, a, c->stream));
    return EMI_OK;
}

int emi_ipm_trial_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_step_t* st, const void* dAlpha, const emi_ipm_point_t* trial) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_trial_dev"));
    const int np = np_total(c);
    if (!ipm_has_point(pt, c->nc, np) || !ipm_has_point(trial, c->nc, np) || !st || !st->DZLam || (np > 0 && (!st->DS || !st->DE1 || !st->DE2)) || !dAlpha)
        return fail(c, EMI_ERR_ARG, "emi_ipm_trial_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_trial_dev", nullptr, nullptr, a));
    ipm_set_point(a, pt); ipm_set_trial(a, trial); ipm_set_step(a, st);
    a.apr = (const double*)dAlpha;
    HIP_TRY(c, emi::launch_ipm(emi::IPM_TRIAL, a, c->stream));
    return EMI_OK;
}

int emi_ipm_merit_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const void* dRES, const void* dCOST, const emi_ipm_bounds_t* bd, const void* dPar,
                      const void* dRs, int reset, void* dOut) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_merit_dev"));
    if (!ipm_has_point(pt, c->nc, np_total(c)) || !dRES || !dCOST || !bd || !dPar || !dOut) return fail(c, EMI_ERR_ARG, "emi_ipm_merit_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_merit_dev", bd, dPar, a));
    EMI_TRY(ipm_partials(c, a));
    ipm_set_point(a, pt);
    a.RES = (const double*)dRES; a.COST = (const double*)dCOST; a.rs = (const double*)dRs; a.reset = reset ? 1 : 0; a.out = (double*)dOut;
    HIP_TRY(c, emi::launch_ipm(emi::IPM_MERIT, a, c->stream));
    return EMI_OK;
}

int emi_ipm_accept_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_point_t* trial, const emi_ipm_duals_t* du, const emi_ipm_step_t* st,
                       const emi_ipm_bounds_t* bd, const void* dPar, const void* dApr, const void* dAdu, const void* dMask) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_accept_dev"));
    const int np = np_total(c);
    if (!ipm_has_point(pt, c->nc, np) || !ipm_has_point(trial, c->nc, np) || !ipm_has_duals(du, np) || !ipm_has_step(st, np) || !bd || !dPar || !dApr || !dAdu)
        return fail(c, EMI_ERR_ARG, "emi_ipm_accept_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_accept_dev", bd, dPar, a));
    ipm_set_point(a, pt); ipm_set_trial(a, trial); ipm_set_duals(a, du); ipm_set_step(a, st);
    a.apr = (const double*)dApr; a.adu = (const double*)dAdu; a.mask = (const unsigned char*)dMask;
    HIP_TRY(c, emi::launch_ipm(emi::IPM_ACCEPT, a, c->stream));
    return EMI_OK;
}

int emi_ipm_error_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dRES, const void* dG,
                      const emi_ipm_bounds_t* bd, const void* dPar, void* dOut) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_error_dev"));
    const int np = np_total(c);
    if (!ipm_has_point(pt, c->nc, np) || !ipm_has_duals(du, np) || !dRES || !dG || !bd || !dPar || !dOut) return fail(c, EMI_ERR_ARG, "emi_ipm_error_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_error_dev", bd, dPar, a));
    EMI_TRY(ipm_partials(c, a));
    ipm_set_point(a, pt); ipm_set_duals(a, du);
    a.RES = (const double*)dRES; a.G = (const double*)dG; a.out = (double*)dOut;
    HIP_TRY(c, emi::launch_ipm(emi::IPM_ERROR, a, c->stream));
    return EMI_OK;
}

int emi_ipm_start_dev(emi_ctx_t c, int phase, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dRES, const emi_ipm_bounds_t* bd,
                      const void* dPar, double bound_push, double bound_frac, void* dFixed, const void* dMask) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_start_dev"));
    const int np = np_total(c);
    bool ok = pt && du && bd && phase >= 0 && phase <= 2;
    if (ok && phase == 0) ok = pt->X && (c->nc == 0 || pt->U) && du->LamF && dFixed && bound_push > 0 && bound_frac > 0;
    if (ok && phase == 1) ok = ipm_has_point(pt, c->nc, np) && ipm_has_duals(du, np) && dRES && dPar && bound_push > 0 && bound_frac > 0;
    if (ok && phase == 2) ok = dPar && (np == 0 || (du->Y && du->W1 && du->W2));
    if (!ok) return fail(c, EMI_ERR_ARG, "emi_ipm_start_dev: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_start_dev", bd, dPar, a));
    ipm_set_point(a, pt); ipm_set_duals(a, du);
    a.RES = (const double*)dRES; a.fixedb = (unsigned char*)dFixed; a.mask = (const unsigned char*)dMask; a.push = bound_push; a.frac = bound_frac;
    HIP_TRY(c, emi::launch_ipm(phase == 0 ? emi::IPM_START_PUSH : phase == 1 ? emi::IPM_START_ROWS : emi::IPM_RESET_W, a, c->stream));
    return EMI_OK;
}

int emi_ipm_error_parts_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dRES, const void* dG,
                            const emi_ipm_bounds_t* bd, const void* dPar, void* dOut) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_error_parts_dev"));
    const int np = np_total(c);
    if (!ipm_has_point(pt, c->nc, np) || !ipm_has_duals(du, np) || !dRES || !dG || !bd || !dPar || !dOut)
        return fail(c, EMI_ERR_ARG, "emi_ipm_error_parts_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_error_parts_dev", bd, dPar, a));
    EMI_TRY(ipm_partials(c, a));
    ipm_set_point(a, pt); ipm_set_duals(a, du);
    a.RES = (const double*)dRES; a.G = (const double*)dG; a.out = (double*)dOut;
    HIP_TRY(c, emi::launch_ipm(emi::IPM_ERROR_PARTS, a, c->stream));
    return EMI_OK;
}

int emi_ipm_keep_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const emi_ipm_point_t* kpt, const emi_ipm_duals_t* kdu,
                     const void* dMask, int restore) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_keep_dev"));
    const int np = np_total(c);
    if (!ipm_has_point(pt, c->nc, np) || !ipm_has_duals(du, np) || !ipm_has_point(kpt, c->nc, np) || !ipm_has_duals(kdu, np))
        return fail(c, EMI_ERR_ARG, "emi_ipm_keep_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmKeepArgs a{};
    const emi_ipm_point_t* P[2] = {pt, kpt};
    const emi_ipm_duals_t* D[2] = {du, kdu};
    for (int side = 0; side < 2; ++side) {
        void* const v[13] = {P[side]->X, P[side]->U, P[side]->S, P[side]->E1, P[side]->E2, D[side]->LamF, D[side]->Y, D[side]->ZL, D[side]->ZU,
                             D[side]->VL, D[side]->VU, D[side]->W1, D[side]->W2};
        for (int i = 0; i < 13; ++i) (side ? a.kept : a.live)[i] = (double*)v[i];
    }
    a.mask = (const unsigned char*)dMask;
    a.B = c->B; a.M = c->M; a.ns = c->ns; a.nc = c->nc; a.np = np; a.restore = restore ? 1 : 0;
    HIP_TRY(c, emi::launch_ipm_keep(a, c->stream));
    return EMI_OK;
}

// ---- the _host forms: every array copied in, the _dev form run, what it writes copied out, synchronised -------------------------------
int emi_ipm_reduce_host(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const double* RES, const double* VALS, const double* G,
                        const emi_ipm_bounds_t* bd, const double* par, const double* DefRes, const double* RowRes, const emi_ipm_elim_t* out,
                        double* Rhs) {
    IPM_HOST_BEGIN("emi_ipm_reduce_host", bd ? bd->nsets : 0);
    const emi_ipm_point_t dp = stage_point(s, z, pt, true, false);
    const emi_ipm_duals_t dd = stage_duals(s, z, du, true, false);
    const emi_ipm_bounds_t db = stage_bounds(s, z, bd);
    const emi_ipm_elim_t de = stage_elim(s, z, out, false, true);
    const void *dR = s.place(RES, z.res, true, false), *dV = s.place(VALS, z.vals, true, false), *dG = s.place(G, z.var, true, false);
    const void *dP = s.place(par, z.inst * 4, true, false), *dDef = s.place(DefRes, z.X, true, false), *dRow = s.place(RowRes, z.row, true, false);
    void* dRhs = s.place(Rhs, z.kkt, false, true);
    IPM_HOST_END(emi_ipm_reduce_dev(c, pt ? &dp : nullptr, du ? &dd : nullptr, dR, dV, dG, bd ? &db : nullptr, dP, dDef, dRow, out ? &de : nullptr, dRhs));
}

int emi_ipm_expand_host(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const double* VALS, const emi_ipm_bounds_t* bd,
                        const double* par, const emi_ipm_elim_t* el, const double* rs, const emi_ipm_step_t* st, double* scal) {
    IPM_HOST_BEGIN("emi_ipm_expand_host", bd ? bd->nsets : 0);
    const emi_ipm_point_t dp = stage_point(s, z, pt, true, false);
    const emi_ipm_duals_t dd = stage_duals(s, z, du, true, false);
    const emi_ipm_bounds_t db = stage_bounds(s, z, bd);
    const emi_ipm_elim_t de = stage_elim(s, z, el, true, false);
    const emi_ipm_step_t ds = stage_step(s, z, st, true, true, false, true);
    const void *dV = s.place(VALS, z.vals, true, false), *dP = s.place(par, z.inst * 4, true, false), *dRs = s.place(rs, z.X, true, false);
    void* dS = s.place(scal, z.inst * 4, false, true);
    IPM_HOST_END(emi_ipm_expand_dev(c, pt ? &dp : nullptr, du ? &dd : nullptr, dV, bd ? &db : nullptr, dP, el ? &de : nullptr, dRs, st ? &ds : nullptr, dS));
}

int emi_ipm_trial_host(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_step_t* st, const double* alpha, const emi_ipm_point_t* trial) {
    IPM_HOST_BEGIN("emi_ipm_trial_host", 0);
    const emi_ipm_point_t dp = stage_point(s, z, pt, true, false), dt = stage_point(s, z, trial, false, true);
    const emi_ipm_step_t ds = stage_step(s, z, st, true, false, true, false);
    const void* dA = s.place(alpha, z.inst, true, false);
    IPM_HOST_END(emi_ipm_trial_dev(c, pt ? &dp : nullptr, st ? &ds : nullptr, dA, trial ? &dt : nullptr));
}

int emi_ipm_merit_host(emi_ctx_t c, const emi_ipm_point_t* pt, const double* RES, const double* COST, const emi_ipm_bounds_t* bd, const double* par,
                       const double* rs, int reset, double* out) {
    IPM_HOST_BEGIN("emi_ipm_merit_host", bd ? bd->nsets : 0);
    emi_ipm_point_t dp = stage_point(s, z, pt, true, false);
    if (pt && reset) s.outs.push_back({pt->S, dp.S, pt->S ? z.row : 0});        // the slack reset updates S in place
    const emi_ipm_bounds_t db = stage_bounds(s, z, bd);
    const void *dR = s.place(RES, z.res, true, false), *dC = s.place(COST, z.inst, true, false), *dP = s.place(par, z.inst * 4, true, false);
    const void* dRs = s.place(rs, z.X, true, false);
    void* dO = s.place(out, z.inst * 2, false, true);
    IPM_HOST_END(emi_ipm_merit_dev(c, pt ? &dp : nullptr, dR, dC, bd ? &db : nullptr, dP, dRs, reset, dO));
}

int emi_ipm_accept_host(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_point_t* trial, const emi_ipm_duals_t* du, const emi_ipm_step_t* st,
                        const emi_ipm_bounds_t* bd, const double* par, const double* a_pr, const double* a_du, const unsigned char* mask) {
    IPM_HOST_BEGIN("emi_ipm_accept_host", bd ? bd->nsets : 0);
    const emi_ipm_point_t dp = stage_point(s, z, pt, true, true), dt = stage_point(s, z, trial, true, false);
    const emi_ipm_duals_t dd = stage_duals(s, z, du, true, true);
    const emi_ipm_step_t ds = stage_step(s, z, st, true, false, true, false);
    const emi_ipm_bounds_t db = stage_bounds(s, z, bd);
    const void *dP = s.place(par, z.inst * 4, true, false), *dA = s.place(a_pr, z.inst, true, false), *dD = s.place(a_du, z.inst, true, false);
    const void* dM = s.place(mask, (size_t)c->B, true, false);
    IPM_HOST_END(emi_ipm_accept_dev(c, pt ? &dp : nullptr, trial ? &dt : nullptr, du ? &dd : nullptr, st ? &ds : nullptr, bd ? &db : nullptr, dP, dA, dD, dM));
}

int emi_ipm_error_host(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const double* RES, const double* G,
                       const emi_ipm_bounds_t* bd, const double* par, double* out) {
    IPM_HOST_BEGIN("emi_ipm_error_host", bd ? bd->nsets : 0);
    const emi_ipm_point_t dp = stage_point(s, z, pt, true, false);
    const emi_ipm_duals_t dd = stage_duals(s, z, du, true, false);
    const emi_ipm_bounds_t db = stage_bounds(s, z, bd);
    const void *dR = s.place(RES, z.res, true, false), *dG = s.place(G, z.var, true, false), *dP = s.place(par, z.inst * 4, true, false);
    void* dO = s.place(out, z.inst * 3, false, true);
    IPM_HOST_END(emi_ipm_error_dev(c, pt ? &dp : nullptr, du ? &dd : nullptr, dR, dG, bd ? &db : nullptr, dP, dO));
}

int emi_ipm_error_parts_host(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const double* RES, const double* G,
                             const emi_ipm_bounds_t* bd, const double* par, double* out) {
    IPM_HOST_BEGIN("emi_ipm_error_parts_host", bd ? bd->nsets : 0);
    const emi_ipm_point_t dp = stage_point(s, z, pt, true, false);
    const emi_ipm_duals_t dd = stage_duals(s, z, du, true, false);
    const emi_ipm_bounds_t db = stage_bounds(s, z, bd);
    const void *dR = s.place(RES, z.res, true, false), *dG = s.place(G, z.var, true, false), *dP = s.place(par, z.inst * 4, true, false);
    void* dO = s.place(out, z.inst * 8, false, true);
    IPM_HOST_END(emi_ipm_error_parts_dev(c, pt ? &dp : nullptr, du ? &dd : nullptr, dR, dG, bd ? &db : nullptr, dP, dO));
}

int emi_ipm_keep_host(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const emi_ipm_point_t* kpt, const emi_ipm_duals_t* kdu,
                      const unsigned char* mask, int restore) {
    IPM_HOST_BEGIN("emi_ipm_keep_host", 0);
    // (both sides go in and come out: an instance the mask leaves out keeps its bits on the side that is written)
    const emi_ipm_point_t dp = stage_point(s, z, pt, true, true), dk = stage_point(s, z, kpt, true, true);
    const emi_ipm_duals_t dd = stage_duals(s, z, du, true, true), de = stage_duals(s, z, kdu, true, true);
    const void* dM = s.place(mask, (size_t)c->B, true, false);
    IPM_HOST_END(emi_ipm_keep_dev(c, pt ? &dp : nullptr, du ? &dd : nullptr, kpt ? &dk : nullptr, kdu ? &de : nullptr, dM, restore));
}

// ---- lock-step interior-point solve of the whole batch (the driver: emi_ipm_solve.hip) -------------------------------------------
int emi_ipm_solve_shard_dev(emi_ctx_t c, void* dX, void* dU, const emi_ipm_bounds_t* bd, const emi_ipm_options_t* opt, void* dLamF,
                            void* dLamC, emi_ipm_result_t* results) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_solve_shard_dev"));
    EMI_TRY(shard_check(c, "emi_ipm_solve_shard_dev"));
    EMI_TRY(ready(c));
    const int np = np_total(c);
    if (!dX || (c->nc > 0 && !dU) || !bd || !opt || !dLamF || (np > 0 && !dLamC) || !results)
        return fail(c, EMI_ERR_ARG, "emi_ipm_solve_shard_dev: null argument");
    if (opt->rules & ~EMI_IPM_RULE_RESIDUAL) return fail(c, EMI_ERR_ARG, "emi_ipm_solve_shard_dev: unknown bit in rules (%d)", opt->rules);
    HIP_TRY(c, hipSetDevice(c->device));
    return emi::ipm_solve_shard(c, dX, dU, bd, *opt, dLamF, dLamC, results);
}

int emi_ipm_solve_shard_host(emi_ctx_t c, double* X, double* U, const emi_ipm_bounds_t* bd, const emi_ipm_options_t* opt, double* LamF,
                             double* LamC, emi_ipm_result_t* results) {
    IPM_HOST_BEGIN("emi_ipm_solve_shard_host", bd ? bd->nsets : 0);
    void *dX = s.place(X, z.X, true, true), *dU = s.place(U, z.U, true, true);
    void *dLF = s.place(LamF, z.X, false, true), *dLC = s.place(LamC, z.row, false, true);
    const emi_ipm_bounds_t db = stage_bounds(s, z, bd);
    IPM_HOST_END(emi_ipm_solve_shard_dev(c, dX, dU, bd ? &db : nullptr, opt, dLF, dLC, results));
}

// ---- the mesh ladder over the lock-step solve (kernels and driver: emi_ipm_ladder.hip) ---------------------------------------------
namespace {

// emi_prolong_dev (no row map) and emi_prolong_rows_dev: one kernel
int prolong(emi_ctx_t c, const char* what, int Mc, int Mf, const void* dPT, const void* dVc, int R, const void* dRowMap, void* dVf) {
    if (!c) return EMI_ERR_ARG;
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: f64 contexts only", what);
    if (Mc < 2 || Mf < 2 || R < 0 || !dPT || (R > 0 && (!dVc || !dVf))) return fail(c, EMI_ERR_ARG, "%s: bad argument", what);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, emi::launch_prolong_rows((const double*)dPT, (const double*)dVc, (const int*)dRowMap, 1, (double*)dVf, Mc, Mf, R, c->stream));
    return EMI_OK;
}

}  // namespace

int emi_prolong_dev(emi_ctx_t c, int Mc, int Mf, const void* dPT, const void* dVc, int R, void* dVf) {
    return prolong(c, "emi_prolong_dev", Mc, Mf, dPT, dVc, R, nullptr, dVf);
}

int emi_repair_guess_dev(emi_ctx_t c, void* dX) {
    if (!c) return EMI_ERR_ARG;
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "emi_repair_guess_dev: f64 contexts only");
    EMI_TRY(ready(c));
    if (!dX) return fail(c, EMI_ERR_ARG, "emi_repair_guess_dev: null argument");
    if (c->B > 65535) return fail(c, EMI_ERR_UNSUPPORTED, "emi_repair_guess_dev: up to 65535 instances");
    if (c->np > 0 && c->path_has_track && c->ntracks <= 0)
        return fail(c, EMI_ERR_STATE, "emi_repair_guess_dev: the table has rows of kind EMI_PATH_TRACK: emi_set_tracks must follow emi_set_mesh");
    HIP_TRY(c, hipSetDevice(c->device));
    const emi::RepairArgs a{(double*)dX, (const double*)c->d_path.p, (const double*)c->d_trkx.p, (const double*)c->d_trky.p, c->B, c->ns, c->M,
                            c->np, c->path_sets, c->px, c->py, c->ntracks, c->track_sets};
    HIP_TRY(c, emi::launch_repair_guess(a, c->stream));
    return EMI_OK;
}

namespace {

// what the ladder refuses before it touches the context (the mesh need not be set: the call sets it)
int ladder_check(emi_ctx_t c, const char* what, int nrungs, const emi_ipm_rung_t* rungs) {
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: f64 contexts only", what);
    if (c->model < 0 || c->B <= 0) return fail(c, EMI_ERR_STATE, "%s: model and batch must be set", what);
    if (c->nch > 0) return fail(c, EMI_ERR_UNSUPPORTED, "%s: contexts with delays are not taken", what);
    if (c->ns + c->nc > 16) return fail(c, EMI_ERR_UNSUPPORTED, "%s: up to 16 variables per node (this model has %d)", what, c->ns + c->nc);
    if (c->kkt_method != 1) return fail(c, EMI_ERR_UNSUPPORTED, "%s: the context is set to the LU method (\"kkt_method\" 0)", what);
    if (nrungs < 1 || !rungs) return fail(c, EMI_ERR_ARG, "%s: no rungs", what);
    bool track = c->np > 0 && c->path_has_track;
    for (int r = 0; r < nrungs; ++r) {
        if (rungs[r].M < 2) return fail(c, EMI_ERR_ARG, "%s: rung %d has %d nodes", what, r, rungs[r].M);
        if (!rungs[r].bd.zl || !rungs[r].bd.zu) return fail(c, EMI_ERR_ARG, "%s: rung %d has no bounds", what, r);
        if (rungs[r].opt.rules & ~EMI_IPM_RULE_RESIDUAL) return fail(c, EMI_ERR_ARG, "%s: rung %d has an unknown bit in rules", what, r);
        if (!rungs[r].recs) continue;
        if (c->np <= 0) return fail(c, EMI_ERR_ARG, "%s: rung %d brings a record table and the context has none", what, r);
        for (size_t i = 0; i < (size_t)c->np * c->path_sets; ++i) track = track || (int)rungs[r].recs[i * EMI_PATH_REC] == EMI_PATH_TRACK;
    }
    if (!track) return EMI_OK;
    // track rows: their centres are per mesh, and only waypoint tables on the device (emi_set_track_waypoints) let the call supply
    // them rung by rung
    if (c->wp_ntracks <= 0)
        return fail(c, EMI_ERR_UNSUPPORTED, "%s: rows of kind EMI_PATH_TRACK have their centres per mesh, which this call cannot supply", what);
    if (c->wp_sets != 1 && c->wp_sets != c->B)
        return fail(c, EMI_ERR_ARG, "%s: the waypoint table has %d sets (1 or the batch, %d)", what, c->wp_sets, c->B);
    const size_t nrec = (size_t)c->np * c->path_sets;
    const auto track_rows_ok = [&](const double* recs, const std::string& whose) {
        for (size_t i = 0; i < nrec; ++i) {
            const double* q = recs + i * EMI_PATH_REC;
            if ((int)q[0] == EMI_PATH_TRACK && !(q[1] >= 0 && q[1] < c->wp_ntracks))
                return fail(c, EMI_ERR_ARG, "%s: record %zu of %s names track %d and the waypoint table has %d", what, i, whose.c_str(), (int)q[1],
                            c->wp_ntracks);
        }
        return (int)EMI_OK;
    };
    if (c->path_has_track) {
        std::vector<double> table(nrec * EMI_PATH_REC);
        HIP_TRY(c, hipSetDevice(c->device));
        EMI_TRY(download_real(c, table.data(), c->d_path.p, table.size()));
        EMI_TRY(track_rows_ok(table.data(), "the context's table"));
    }
    for (int r = 0; r < nrungs; ++r)
        if (rungs[r].recs) EMI_TRY(track_rows_ok(rungs[r].recs, "the table of rung " + std::to_string(r)));
    return EMI_OK;
}

// what the _dev forms of the ladder, with and without refinement, ask of their arrays and of the horizon
int ladder_args_check(emi_ctx_t c, const char* what, double t0, double tf, const void* dX0, const void* dU0, const void* dX, const void* dU,
                      const void* dLamF, const void* dLamC, const void* results) {
    if (!dX0 || !dX || (c->nc > 0 && (!dU0 || !dU)) || !dLamF || (np_total(c) > 0 && !dLamC) || !results)
        return fail(c, EMI_ERR_ARG, "%s: null argument", what);
    if (!(tf > t0)) return fail(c, EMI_ERR_ARG, "%s: tf must exceed t0", what);
    return EMI_OK;
}

// the two _host forms, after their checks: the starts, every rung's zl and zu and the outputs [B][rows][ld] staged, the _dev form run.
// rf NULL: the ladder, whose outputs only come out; with refinement they go in too (the columns beyond an instance's mesh are the caller's)
// rs given: the restart run over either, whose outputs go in and come out as with refinement (X0 may be NULL there)
int ladder_host(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t* rf, const emi_ipm_restart_t* rs,
                const double* X0, const double* U0, int ld, double* X, double* U, double* LamF, double* LamC, emi_ipm_result_t* results,
                double* err, emi_ipm_refine_result_t* out, emi_ipm_restart_result_t* rout) {
    HIP_TRY(c, hipSetDevice(c->device));
    HostStager s(c);
    const size_t B = (size_t)c->B, nv = (size_t)(c->ns + c->nc), M0 = (size_t)rungs[0].M, L = (size_t)ld;
    const bool in = rf != nullptr || rs != nullptr;
    const void *dX0 = s.place(X0, B * c->ns * M0 * 8, true, false), *dU0 = s.place(U0, B * c->nc * M0 * 8, true, false);
    void *dX = s.place(X, B * c->ns * L * 8, in, true), *dU = s.place(U, B * c->nc * L * 8, in, true);
    void *dLF = s.place(LamF, B * c->ns * L * 8, in, true), *dLC = s.place(LamC, B * (size_t)np_total(c) * L * 8, in, true);
    std::vector<emi_ipm_rung_t> dr(rungs, rungs + nrungs);
    for (emi_ipm_rung_t& g : dr) {
        const size_t bytes = (size_t)std::max(g.bd.nsets, 0) * nv * (size_t)g.M * 8;
        g.bd.zl = s.place(g.bd.zl, bytes, true, false);
        g.bd.zu = s.place(g.bd.zu, bytes, true, false);
    }
    IPM_HOST_END(rs   ? emi_ipm_solve_restart_dev(c, nrungs, dr.data(), t0, tf, rf, rs, dX0, dU0, ld, dX, dU, dLF, dLC, results, err, rout)
                 : rf ? emi_ipm_solve_refine_dev(c, nrungs, dr.data(), t0, tf, rf, dX0, dU0, ld, dX, dU, dLF, dLC, results, err, out)
                      : emi_ipm_solve_ladder_dev(c, nrungs, dr.data(), t0, tf, dX0, dU0, dX, dU, dLF, dLC, results));
}

}  // namespace

int emi_ipm_solve_ladder_dev(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const void* dX0, const void* dU0,
                             void* dX, void* dU, void* dLamF, void* dLamC, emi_ipm_result_t* results) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ladder_check(c, "emi_ipm_solve_ladder_dev", nrungs, rungs));
    EMI_TRY(ladder_args_check(c, "emi_ipm_solve_ladder_dev", t0, tf, dX0, dU0, dX, dU, dLamF, dLamC, results));
    HIP_TRY(c, hipSetDevice(c->device));
    return emi::ipm_solve_ladder(c, nrungs, rungs, t0, tf, dX0, dU0, dX, dU, dLamF, dLamC, results);
}

int emi_ipm_solve_ladder_host(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const double* X0, const double* U0,
                              double* X, double* U, double* LamF, double* LamC, emi_ipm_result_t* results) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ladder_check(c, "emi_ipm_solve_ladder_host", nrungs, rungs));
    return ladder_host(c, nrungs, rungs, t0, tf, nullptr, nullptr, X0, U0, rungs[nrungs - 1].M, X, U, LamF, LamC, results, nullptr, nullptr, nullptr);
}

// ---- the ladder with refinement: instances that meet the ODE tolerance leave the batch (kernels and driver: emi_ipm_ladder.hip) -------
int emi_prolong_rows_dev(emi_ctx_t c, int Mc, int Mf, const void* dPT, const void* dVc, int R, const void* dRowMap, void* dVf) {
    return prolong(c, "emi_prolong_rows_dev", Mc, Mf, dPT, dVc, R, dRowMap, dVf);
}

int emi_shard_move_dev(emi_ctx_t c, int n, const void* dSrcIdx, const void* dDstIdx, int narrays, const int* rows, const void* const* src,
                       const int* src_ld, void* const* dst, const int* dst_ld, int len) {
    if (!c) return EMI_ERR_ARG;
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "emi_shard_move_dev: f64 contexts only");
    if (n < 0 || len < 0 || narrays < 1 || narrays > emi::SHARD_MOVE_ARRAYS || !rows || !src || !src_ld || !dst || !dst_ld)
        return fail(c, EMI_ERR_ARG, "emi_shard_move_dev: bad argument (n >= 0, len >= 0, 1 .. %d arrays)", emi::SHARD_MOVE_ARRAYS);
    emi::ShardMoveArgs a{};
    for (int q = 0; q < narrays; ++q) {
        if (rows[q] < 0 || src_ld[q] < len || dst_ld[q] < len || (rows[q] > 0 && n > 0 && len > 0 && (!src[q] || !dst[q])))
            return fail(c, EMI_ERR_ARG, "emi_shard_move_dev: array %d: rows >= 0, leading dimensions >= len, no NULL array", q);
        a.src[q] = (const double*)src[q]; a.dst[q] = (double*)dst[q]; a.rows[q] = rows[q]; a.sld[q] = src_ld[q]; a.dld[q] = dst_ld[q];
    }
    a.sidx = (const int*)dSrcIdx; a.didx = (const int*)dDstIdx; a.n = n; a.narrays = narrays; a.len = len;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, emi::launch_shard_move(a, c->stream));
    return EMI_OK;
}

namespace {

// what a call whose instances leave the batch asks of the caller's padded arrays and of the rungs' bounds
int compaction_check(emi_ctx_t c, const char* what, int nrungs, const emi_ipm_rung_t* rungs, int ldm) {
    if (c->B > 65535) return fail(c, EMI_ERR_UNSUPPORTED, "%s: up to 65535 instances", what);
    for (int r = 0; r < nrungs; ++r) {
        if (rungs[r].M > ldm) return fail(c, EMI_ERR_ARG, "%s: ldm %d is below rung %d's %d nodes", what, ldm, r, rungs[r].M);
        if (rungs[r].bd.nsets != 1 && rungs[r].bd.nsets != c->B)
            return fail(c, EMI_ERR_ARG, "%s: rung %d's bounds have %d sets (1 or the batch, %d)", what, r, rungs[r].bd.nsets, c->B);
    }
    return EMI_OK;
}

// what the refinement refuses beyond the ladder's list
int refine_check(emi_ctx_t c, const char* what, int nrungs, const emi_ipm_rung_t* rungs, const emi_ipm_refine_t* rf, int ldm, const void* err,
                 const void* out) {
    EMI_TRY(ladder_check(c, what, nrungs, rungs));
    if (!rf || !err || !out) return fail(c, EMI_ERR_ARG, "%s: null argument", what);
    if (!(rf->ode_tol >= 0.0)) return fail(c, EMI_ERR_ARG, "%s: ode_tol must be >= 0", what);
    if (rf->first_check < 0 || rf->first_check >= nrungs) return fail(c, EMI_ERR_ARG, "%s: first_check %d outside the %d rungs", what, rf->first_check, nrungs);
    if ((rf->ul == nullptr) != (rf->uu == nullptr)) return fail(c, EMI_ERR_ARG, "%s: ul and uu come as a pair", what);
    return compaction_check(c, what, nrungs, rungs, ldm);
}

// what the restart run refuses beyond the list of the refinement (rf NULL: of the ladder)
int restart_check(emi_ctx_t c, const char* what, int nrungs, const emi_ipm_rung_t* rungs, const emi_ipm_refine_t* rf, const emi_ipm_restart_t* rs,
                  bool has_x0, int ldm, const void* err, const void* out) {
    if (rf) EMI_TRY(refine_check(c, what, nrungs, rungs, rf, ldm, err, out));
    else {
        EMI_TRY(ladder_check(c, what, nrungs, rungs));
        if (!err || !out) return fail(c, EMI_ERR_ARG, "%s: null argument", what);
        EMI_TRY(compaction_check(c, what, nrungs, rungs, ldm));
    }
    if (!rs) return fail(c, EMI_ERR_ARG, "%s: rs is NULL", what);
    if (rs->nstarts < 0 || (rs->nstarts > 0 && !rs->starts)) return fail(c, EMI_ERR_ARG, "%s: %d starts and no array of them", what, rs->nstarts);
    const long long A = (long long)rs->nstarts + (has_x0 ? 1 : 0);
    if (A < 1 || A > emi::RestartBook::MAX_ATTEMPTS)
        return fail(c, EMI_ERR_ARG, "%s: %lld attempts (a guess and the starts: 1 .. %d)", what, A, emi::RestartBook::MAX_ATTEMPTS);
    for (int i = 0; i < rs->nstarts; ++i)
        if (rs->starts[i].nsets != 1 && rs->starts[i].nsets != c->B)
            return fail(c, EMI_ERR_ARG, "%s: start %d has %d sets of end states (1 or the batch, %d)", what, i, rs->starts[i].nsets, c->B);
    for (int a = 0; rs->patience && a < A; ++a)
        if (rs->patience[a] < 0) return fail(c, EMI_ERR_ARG, "%s: patience[%d] is negative", what, a);
    if (rs->retry_mask & ~((1 << (EMI_REFINE_FAILED + 1)) - 1)) return fail(c, EMI_ERR_ARG, "%s: retry_mask %d has bits beyond the four verdicts", what, rs->retry_mask);
    if (rs->flags & ~EMI_RESTART_DROP_FAILED) return fail(c, EMI_ERR_ARG, "%s: unknown flag in %d", what, rs->flags);
    return EMI_OK;
}

}  // namespace

int emi_ipm_solve_refine_dev(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t* rf,
                             const void* dX0, const void* dU0, int ldm, void* dX, void* dU, void* dLamF, void* dLamC,
                             emi_ipm_result_t* results, double* err, emi_ipm_refine_result_t* out) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(refine_check(c, "emi_ipm_solve_refine_dev", nrungs, rungs, rf, ldm, err, out));
    EMI_TRY(ladder_args_check(c, "emi_ipm_solve_refine_dev", t0, tf, dX0, dU0, dX, dU, dLamF, dLamC, results));
    HIP_TRY(c, hipSetDevice(c->device));
    return emi::ipm_solve_refine(c, nrungs, rungs, t0, tf, *rf, dX0, dU0, ldm, dX, dU, dLamF, dLamC, results, err, out);
}

int emi_ipm_solve_refine_host(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t* rf,
                              const double* X0, const double* U0, int ldm, double* X, double* U, double* LamF, double* LamC,
                              emi_ipm_result_t* results, double* err, emi_ipm_refine_result_t* out) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(refine_check(c, "emi_ipm_solve_refine_host", nrungs, rungs, rf, ldm, err, out));
    return ladder_host(c, nrungs, rungs, t0, tf, rf, nullptr, X0, U0, ldm, X, U, LamF, LamC, results, err, out, nullptr);
}

// ---- ladder restarts: the instances an attempt did not solve are solved again from the next start (driver: emi_ipm_ladder.hip) ------
int emi_ipm_solve_restart_dev(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t* rf,
                              const emi_ipm_restart_t* rs, const void* dX0, const void* dU0, int ldm, void* dX, void* dU, void* dLamF,
                              void* dLamC, emi_ipm_result_t* results, double* err, emi_ipm_restart_result_t* out) {
    const char* what = "emi_ipm_solve_restart_dev";
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(restart_check(c, what, nrungs, rungs, rf, rs, dX0 != nullptr, ldm, err, out));
    if (!dX || (c->nc > 0 && (!dU0 || !dU)) || !dLamF || (np_total(c) > 0 && !dLamC) || !results) return fail(c, EMI_ERR_ARG, "%s: null argument", what);
    if (!(tf > t0)) return fail(c, EMI_ERR_ARG, "%s: tf must exceed t0", what);
    HIP_TRY(c, hipSetDevice(c->device));
    return emi::ipm_solve_restart(c, nrungs, rungs, t0, tf, rf, *rs, dX0, dU0, ldm, dX, dU, dLamF, dLamC, results, err, out);
}

int emi_ipm_solve_restart_host(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t* rf,
                               const emi_ipm_restart_t* rs, const double* X0, const double* U0, int ldm, double* X, double* U,
                               double* LamF, double* LamC, emi_ipm_result_t* results, double* err, emi_ipm_restart_result_t* out) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(restart_check(c, "emi_ipm_solve_restart_host", nrungs, rungs, rf, rs, X0 != nullptr, ldm, err, out));
    return ladder_host(c, nrungs, rungs, t0, tf, rf, rs, X0, U0, ldm, X, U, LamF, LamC, results, err, nullptr, out);
}

}  // extern "C"
