// emi_api_kkt.hip -- the Newton step of the C ABI (emi_kkt.hip, emi_kkt_blocks.hip): factor / low-rank correction / solve of one
// context, of n contexts as a batch, the node blocks (assembly, screen and eigen-fix over [instance][node]), and the steps of a
// context's whole batch from device arrays (the shard calls).
#include "emi_ctx.hpp"

using namespace emi_api;

namespace {

// the per-entry term lists of the assembly kernel on the device: for every packed entry of the block, the products
// SigT[row] VALS[ea] VALS[eb] that the host loop adds to it, in that loop's order (rows ascending, pairs (a, b <= a) in list order)
int blocks_terms(emi_ctx_t c, const char* what) {
    const int nv = c->ns + c->nc, nh = nv * (nv + 1) / 2, np = np_total(c), nvals = nvals_of(c);
    std::vector<int> ptr, var, ent;
    EMI_TRY(path_row_list(c, what, ptr, var, ent));
    std::vector<int> key = {nv, np, nvals, (int)c->blk_rows_set};
    key.insert(key.end(), ptr.begin(), ptr.end());
    key.insert(key.end(), var.begin(), var.end());
    key.insert(key.end(), ent.begin(), ent.end());
    if (key == c->blk_key) return EMI_OK;
    std::vector<std::vector<int>> per(nh);      // (row, ea, eb) triples of every entry
    for (int j = 0; j < np; ++j)
        for (int a = ptr[j]; a < ptr[j + 1]; ++a)
            for (int b = ptr[j]; b <= a; ++b) {
                const int hi = std::max(var[a], var[b]), lo = std::min(var[a], var[b]);
                std::vector<int>& t = per[hi * (hi + 1) / 2 + lo];
                t.push_back(j); t.push_back(ent[a]); t.push_back(ent[b]);
            }
    std::vector<int> tp(nh + 1, 0), tr, ta, tb;
    for (int e = 0; e < nh; ++e) {
        for (size_t i = 0; i < per[e].size(); i += 3) { tr.push_back(per[e][i]); ta.push_back(per[e][i + 1]); tb.push_back(per[e][i + 2]); }
        tp[e + 1] = (int)tr.size();
    }
    const size_t nt = std::max<size_t>(tr.size(), 1);
    tr.resize(nt); ta.resize(nt); tb.resize(nt);
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // a launch in flight may still read the old lists
    HIP_TRY(c, c->blk_term_ptr.reserve(tp.size()));
    HIP_TRY(c, c->blk_term_row.reserve(nt));
    HIP_TRY(c, c->blk_term_ea.reserve(nt));
    HIP_TRY(c, c->blk_term_eb.reserve(nt));
    HIP_TRY(c, hipMemcpyAsync(c->blk_term_ptr.p, tp.data(), tp.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->blk_term_row.p, tr.data(), nt * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->blk_term_ea.p, ta.data(), nt * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->blk_term_eb.p, tb.data(), nt * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // (the sources are locals)
    c->blk_key = key;
    return EMI_OK;
}

int blocks_check(emi_ctx_t c, const char* what) {
    if (c->M <= 0 || c->model < 0 || c->B <= 0) return fail(c, EMI_ERR_STATE, "%s: mesh, model and batch must be set", what);
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: f64 contexts only", what);
    if (c->ns + c->nc > 16) return fail(c, EMI_ERR_UNSUPPORTED, "%s: node blocks of up to 16 variables (this model has %d)", what, c->ns + c->nc);
    return EMI_OK;
}

// the unmasked instances of the batch; need > 0: every one of them must hold a factorisation for the context's mesh and model
// (1: any, 2: of the Schur path)
int shard_members(emi_ctx_t c, const char* what, const unsigned char* mask, int need, std::vector<int>& inst) {
    const int nv = c->ns + c->nc;
    for (int b = 0; b < c->B; ++b) {
        if (mask && !mask[b]) continue;
        if (need) {
            const int held = b < (int)c->kkt_shard.size() ? emi::kkt_holds(c->kkt_shard[b], c->M, c->ns, nv) : 0;
            if (held == 0)
                return fail(c, EMI_ERR_STATE, "%s: instance %d holds no factorisation for this mesh and model (emi_kkt_factor_shard_dev)", what, b);
            if (need == 2 && held != 1)
                return fail(c, EMI_ERR_UNSUPPORTED, "%s: instance %d holds no factorisation of the Schur path (the LU fallback is refined by "
                                                    "the caller: emi_kkt_solve_shard_dev)", what, b);
        }
        inst.push_back(b);
    }
    return EMI_OK;
}

}  // namespace

// the (variable, VALS entry) pairs of every path row: the caller's list (emi_kkt_blocks_rows) or the record table's default
int emi_api::path_row_list(emi_ctx_t c, const char* what, std::vector<int>& ptr, std::vector<int>& var, std::vector<int>& ent) {
    const int nv = c->ns + c->nc, np = np_total(c), nvals = nvals_of(c);
    if (c->blk_rows_set) {
        if ((int)c->blk_row_ptr.size() != np + 1)
            return fail(c, EMI_ERR_STATE, "%s: the row list (emi_kkt_blocks_rows) has %d rows, the context %d", what, (int)c->blk_row_ptr.size() - 1, np);
        ptr = c->blk_row_ptr; var = c->blk_var; ent = c->blk_entry;
        for (size_t a = 0; a < var.size(); ++a)         // (the model may have changed since the list was given)
            if (var[a] >= nv || ent[a] >= nvals) return fail(c, EMI_ERR_STATE, "%s: the row list does not fit the context's layout any more", what);
    } else {
        if (c->np_model > 0)
            return fail(c, EMI_ERR_STATE, "%s: the context has traced path rows and no row list (emi_kkt_blocks_rows)", what);
        ptr.push_back(0);
        for (int j = 0; j < c->np; ++j) {
            var.push_back(c->px); ent.push_back(c->ns * nv + 2 * j);
            var.push_back(c->py); ent.push_back(c->ns * nv + 2 * j + 1);
            ptr.push_back((int)var.size());
        }
    }
    return EMI_OK;
}

int emi_api::shard_check(emi_ctx_t c, const char* what) {
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: f64 contexts only", what);
    if (c->M <= 0 || c->model < 0 || c->B <= 0) return fail(c, EMI_ERR_STATE, "%s: mesh, model and batch must be set", what);
    if (c->points_only) return fail(c, EMI_ERR_STATE, "%s: the mesh has no differentiation matrix", what);
    if (c->nch > 0) return fail(c, EMI_ERR_UNSUPPORTED, "%s: contexts without delays only", what);
    if (c->ns + c->nc > 16) return fail(c, EMI_ERR_UNSUPPORTED, "%s: node blocks of up to 16 variables (this model has %d)", what, c->ns + c->nc);
    if (c->kkt_method != 1)
        return fail(c, EMI_ERR_UNSUPPORTED, "%s: the context is set to the LU method (\"kkt_method\" 0): emi_kkt_factor_dev per instance", what);
    return EMI_OK;
}

extern "C" {

// emi_kkt_factor / emi_kkt_factor_dev: the blocks in host or in device memory, everything else the same
static int kkt_factor_from(emi_ctx_t c, const char* what, const void* Qblk, const void* Jblk, const void* fixed, double dc, int* info,
                           bool blocks_on_device) {
    if (!c) return EMI_ERR_ARG;
    if (c->M <= 0 || c->model < 0) return fail(c, EMI_ERR_STATE, "%s: mesh and model must be set", what);
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: f64 contexts only", what);
    if (c->points_only) return fail(c, EMI_ERR_STATE, "%s: the mesh has no differentiation matrix", what);
    if (!Qblk || !Jblk || !fixed || !info || !(dc >= 0.0)) return fail(c, EMI_ERR_ARG, "%s: bad argument", what);
    HIP_TRY(c, hipSetDevice(c->device));
    std::string err;
    const int st = emi::kkt_factor(&c->kkt, c->stream, (const double*)c->d_D.p, c->M, c->ns, c->ns + c->nc, (const double*)Qblk,
                                   (const double*)Jblk, (const unsigned char*)fixed, dc, c->kkt_method, info, &err, blocks_on_device);
    if (st) c->err = err;
    return st;
}

int emi_kkt_factor(emi_ctx_t c, const double* Qblk, const double* Jblk, const unsigned char* fixed, double dc,
                   int* info) {
    return kkt_factor_from(c, "emi_kkt_factor", Qblk, Jblk, fixed, dc, info, false);
}

int emi_kkt_factor_dev(emi_ctx_t c, const void* dQblk, const void* dJblk, const void* dFixed, double dc, int* info) {
    return kkt_factor_from(c, "emi_kkt_factor_dev", dQblk, dJblk, dFixed, dc, info, true);
}

// ---- node blocks of the Newton step: assembly, screen and eigen-fix over [instance][node] (emi_kkt_blocks.hip) -----------------
int emi_kkt_blocks_rows(emi_ctx_t c, int np, const int* row_ptr, const int* var, const int* entry) {
    if (!c) return EMI_ERR_ARG;
    if (c->model < 0) return fail(c, EMI_ERR_STATE, "emi_kkt_blocks_rows: the model must be set");
    if (np < 0 || !row_ptr || row_ptr[0] != 0) return fail(c, EMI_ERR_ARG, "emi_kkt_blocks_rows: bad argument");
    const int nv = c->ns + c->nc, nvals = nvals_of(c);
    for (int j = 0; j < np; ++j)
        if (row_ptr[j + 1] < row_ptr[j]) return fail(c, EMI_ERR_ARG, "emi_kkt_blocks_rows: row_ptr decreases at row %d", j);
    const int n = row_ptr[np];
    if (n > 0 && (!var || !entry)) return fail(c, EMI_ERR_ARG, "emi_kkt_blocks_rows: bad argument");
    for (int a = 0; a < n; ++a)
        if (var[a] < 0 || var[a] >= nv || entry[a] < 0 || entry[a] >= nvals)
            return fail(c, EMI_ERR_ARG, "emi_kkt_blocks_rows: pair %d (variable %d, VALS entry %d) is out of range (%d variables, %d entries)",
                        a, var[a], entry[a], nv, nvals);
    c->blk_row_ptr.assign(row_ptr, row_ptr + np + 1);
    c->blk_var.assign(var, var + n);
    c->blk_entry.assign(entry, entry + n);
    c->blk_rows_set = true;
    c->blk_key.clear();
    return EMI_OK;
}

int emi_kkt_blocks_dev(emi_ctx_t c, const void* dH, const void* dVALS, const void* dSigma, const void* dSigT, const void* dFixed,
                       double dw_shift, void* dQexact, void* dQ, int max_mods, void* dCount, void* dNode, void* dDelta, void* dVec,
                       void* dWorst) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(blocks_check(c, "emi_kkt_blocks_dev"));
    const int nv = c->ns + c->nc, np = np_total(c);
    if (!dH || !dVALS || !dSigma || !dFixed || !dQ || !dCount || !dWorst || max_mods < 0 || (np > 0 && !dSigT) ||
        (max_mods > 0 && (!dNode || !dDelta || !dVec)) || !(dw_shift >= 0.0))
        return fail(c, EMI_ERR_ARG, "emi_kkt_blocks_dev: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    EMI_TRY(blocks_terms(c, "emi_kkt_blocks_dev"));
    const size_t BM = (size_t)c->B * c->M;
    HIP_TRY(c, c->blk_flag.reserve(BM));
    HIP_TRY(c, c->blk_list.reserve(BM));
    HIP_TRY(c, c->blk_cnt.reserve(BM));
    HIP_TRY(c, c->blk_nflag.reserve((size_t)c->B));
    HIP_TRY(c, c->blk_tworst.reserve(BM));
    HIP_TRY(c, c->blk_tdelta.reserve(BM * nv));
    // (room for EVERY block failing with all nv eigenvalues negative: how many fail is known on the device only, and a host
    //  round trip to size it is what this call avoids.  B M nv^2 doubles: 34 MB at 64 x 1024 nodes x 8, 2 GiB at 1024 x 1024 x 16)
    HIP_TRY(c, c->blk_tvec.reserve(BM * nv * nv));
    emi::BlocksArgs a{};
    a.H = (const double*)dH; a.VALS = (const double*)dVALS; a.Sigma = (const double*)dSigma; a.SigT = (const double*)dSigT;
    a.fixed = (const unsigned char*)dFixed; a.dw_shift = dw_shift; a.Qexact = (double*)dQexact; a.Q = (double*)dQ;
    a.max_mods = max_mods; a.count = (int*)dCount; a.node = (int*)dNode; a.delta = (double*)dDelta; a.vec = (double*)dVec;
    a.worst = (double*)dWorst;
    a.B = c->B; a.M = c->M; a.nv = nv; a.np = np; a.nvals = nvals_of(c); a.generic = c->blk_generic;
    a.term_ptr = c->blk_term_ptr.p; a.term_row = c->blk_term_row.p; a.term_ea = c->blk_term_ea.p; a.term_eb = c->blk_term_eb.p;
    a.flag = c->blk_flag.p; a.list = c->blk_list.p; a.nflag = c->blk_nflag.p; a.cnt = c->blk_cnt.p;
    a.tdelta = c->blk_tdelta.p; a.tvec = c->blk_tvec.p; a.tworst = c->blk_tworst.p;
    HIP_TRY(c, emi::launch_kkt_blocks(a, c->stream));
    return EMI_OK;
}

int emi_kkt_blocks_host(emi_ctx_t c, const double* H, const double* VALS, const double* Sigma, const double* SigT,
                        const unsigned char* fixed, double dw_shift, double* Qexact, double* Q, int max_mods, int* count, int* node,
                        double* delta, double* vec, double* worst) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(blocks_check(c, "emi_kkt_blocks_host"));
    const size_t B = (size_t)c->B, M = (size_t)c->M, nv = (size_t)(c->ns + c->nc), nh = nv * (nv + 1) / 2, np = (size_t)np_total(c);
    if (!H || !VALS || !Sigma || !fixed || !Q || !count || !worst || max_mods < 0 || (np > 0 && !SigT) ||
        (max_mods > 0 && (!node || !delta || !vec)))
        return fail(c, EMI_ERR_ARG, "emi_kkt_blocks_host: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t mm = (size_t)max_mods, blk = B * nh * M * 8, list = std::max<size_t>(B * mm, 1);
    HostStager s(c);
    const void *dH = s.place(H, blk, true, false), *dV = s.place(VALS, B * nvals_of(c) * M * 8, true, false), *dFx = s.place(fixed, B * nv * M, true, false);
    const void *dSg = s.place(Sigma, B * nv * M * 8, true, false), *dSt = np ? s.place(SigT, B * np * M * 8, true, false) : nullptr;
    void *dQx = s.place(Qexact, blk, false, true), *dQ = s.place(Q, blk, false, true);
    void *dCnt = s.place(count, B * sizeof(int), false, true), *dWorst = s.place(worst, B * 8, false, true);
    // (the lists come back below, not with the rest: the caller's memory beyond an instance's count stays as it is)
    void *dNode = s.place(node, list * sizeof(int), false, false), *dDelta = s.place(delta, list * 8, false, false);
    void* dVec = s.place(vec, list * nv * 8, false, false);
    HOST_STAGED_TRY(s, emi_kkt_blocks_dev(c, dH, dV, dSg, dSt, dFx, dw_shift, dQx, dQ, max_mods, dCnt, dNode, dDelta, dVec, dWorst));
    EMI_TRY(s.finish());
    // only what the kernels wrote: the first min(count, max_mods) entries of every instance
    for (size_t b = 0; b < B && mm > 0; ++b) {
        const size_t n = std::min<size_t>((size_t)std::max(count[b], 0), mm);
        if (n == 0) continue;
        HIP_TRY(c, hipMemcpyAsync(node + b * mm, (const int*)dNode + b * mm, n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(delta + b * mm, (const double*)dDelta + b * mm, n * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(vec + b * mm * nv, (const double*)dVec + b * mm * nv, n * nv * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}

int emi_kkt_lowrank(emi_ctx_t c, int r, const int* node, const double* vec, const double* delta, int* exact) {
    if (!c || r < 0 || !exact || (r > 0 && (!node || !vec || !delta))) return fail(c, EMI_ERR_ARG, "emi_kkt_lowrank: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    for (int a = 0; a < r; ++a)
        if (node[a] < 0 || node[a] >= c->M || !(delta[a] > 0.0))
            return fail(c, EMI_ERR_ARG, "emi_kkt_lowrank: column %d has node %d / delta %g", a, node[a], delta[a]);
    std::string err;
    const int st = emi::kkt_lowrank(c->kkt, c->stream, (c->ns + c->nc) * c->M, r, node, vec, delta, exact, &err);
    if (st) c->err = err;
    return st;
}

// ---- batched Newton steps: n contexts (one scenario each) on the same mesh and model ---------------------------------------
static int batch_compatible(int n, const emi_ctx_t* ctxs, const char* what, bool factorising) {
    if (n < 1 || !ctxs || !ctxs[0]) return EMI_ERR_ARG;
    emi_ctx_t c0 = ctxs[0];
    for (int b = 0; b < n; ++b) {
        emi_ctx_t c = ctxs[b];
        if (!c) return EMI_ERR_ARG;
        if (c->M <= 0 || c->model < 0 || c->f32 || c->points_only)
            return fail(c0, EMI_ERR_STATE, "%s: context %d is not an f64 context with a collocation mesh and a model", what, b);
        if (factorising && c->kkt_method != 1)
            return fail(c0, EMI_ERR_UNSUPPORTED, "%s: context %d is set to the LU method (\"kkt_method\" 0): emi_kkt_factor", what, b);
        if (c->device != c0->device || c->M != c0->M || c->ns != c0->ns || c->nc != c0->nc)
            return fail(c0, EMI_ERR_ARG, "%s: context %d differs from context 0 in device, mesh size or model dimensions", what, b);
        for (int a = 0; a < b; ++a)
            if (ctxs[a] == c) return fail(c0, EMI_ERR_ARG, "%s: context %d appears twice", what, b);
    }
    return EMI_OK;
}

int emi_kkt_factor_batch(int n, const emi_ctx_t* ctxs, const double* const* Qblk, const double* const* Jblk,
                         const unsigned char* const* fixed, const double* dc, int* info) {
    int st = batch_compatible(n, ctxs, "emi_kkt_factor_batch", true);
    if (st) return st;
    emi_ctx_t c0 = ctxs[0];
    if (!Qblk || !Jblk || !fixed || !dc || !info) return fail(c0, EMI_ERR_ARG, "emi_kkt_factor_batch: null argument");
    for (int b = 0; b < n; ++b)
        if (!Qblk[b] || !Jblk[b] || !fixed[b] || !(dc[b] >= 0.0)) return fail(c0, EMI_ERR_ARG, "emi_kkt_factor_batch: bad argument for scenario %d", b);
    HIP_TRY(c0, hipSetDevice(c0->device));
    std::vector<emi::KktWorkspace**> pws(n);
    std::vector<const double*> dD(n);
    for (int b = 0; b < n; ++b) {
        HIP_TRY(c0, hipStreamSynchronize(ctxs[b]->stream));     // whatever the scenario's own stream still holds (its last evaluation)
        pws[b] = &ctxs[b]->kkt;
        dD[b] = (const double*)ctxs[b]->d_D.p;
    }
    std::string err;
    st = emi::kkt_factor_batch(n, pws.data(), c0->stream, dD.data(), c0->M, c0->ns, c0->ns + c0->nc, Qblk, Jblk, fixed, dc, info, &err);
    if (st) { c0->err = err; return st; }
    // scenarios the batch could not take (a node block not positive definite, the ladder exhausted, more than 16 variables per node):
    // the single path with its LU
    for (int b = 0; b < n; ++b)
        if (info[b] < 0) {
            const int s1 = emi_kkt_factor(ctxs[b], Qblk[b], Jblk[b], fixed[b], dc[b], &info[b]);
            if (s1) { c0->err = ctxs[b]->err; return s1; }
        }
    return EMI_OK;
}

int emi_kkt_solve_batch(int n, const emi_ctx_t* ctxs, double* const* rhs) {
    int st = batch_compatible(n, ctxs, "emi_kkt_solve_batch", false);
    if (st) return st;
    emi_ctx_t c0 = ctxs[0];
    if (!rhs) return fail(c0, EMI_ERR_ARG, "emi_kkt_solve_batch: null argument");
    HIP_TRY(c0, hipSetDevice(c0->device));
    // scenarios whose factorisation is the LU fallback (or none) go through the single entry point; the rest as one batch
    std::vector<emi::KktWorkspace*> ws;
    std::vector<double*> rb;
    for (int b = 0; b < n; ++b) {
        if (!rhs[b]) return fail(c0, EMI_ERR_ARG, "emi_kkt_solve_batch: null right-hand side %d", b);
        HIP_TRY(c0, hipStreamSynchronize(ctxs[b]->stream));
        if (emi::kkt_is_schur(ctxs[b]->kkt)) { ws.push_back(ctxs[b]->kkt); rb.push_back(rhs[b]); }
        else if ((st = emi_kkt_solve(ctxs[b], rhs[b], 1))) { c0->err = ctxs[b]->err; return st; }
    }
    if (ws.empty()) return EMI_OK;
    std::string err;
    st = emi::kkt_solve_batch((int)ws.size(), ws.data(), c0->stream, (c0->ns + c0->nc) * c0->M, rb.data(), &err);
    if (st) c0->err = err;
    return st;
}

int emi_kkt_solve_refined_batch(int n, const emi_ctx_t* ctxs, double* const* rhs, const double* dc_nominal, int max_steps, double* rel,
                                int* nsolve, int* reverted, int* status) {
    int st = batch_compatible(n, ctxs, "emi_kkt_solve_refined_batch", false);
    if (st) return st;
    emi_ctx_t c0 = ctxs[0];
    if (!rhs || !dc_nominal || !rel || !nsolve || !reverted || !status || max_steps < 0)
        return fail(c0, EMI_ERR_ARG, "emi_kkt_solve_refined_batch: bad argument");
    HIP_TRY(c0, hipSetDevice(c0->device));
    std::vector<emi::KktWorkspace*> ws(n);
    for (int b = 0; b < n; ++b) {
        if (!rhs[b] || !(dc_nominal[b] >= 0.0)) return fail(c0, EMI_ERR_ARG, "emi_kkt_solve_refined_batch: bad argument for scenario %d", b);
        if (!emi::kkt_is_schur(ctxs[b]->kkt))
            return fail(c0, EMI_ERR_UNSUPPORTED, "emi_kkt_solve_refined_batch: scenario %d holds no factorisation of the Schur path (the LU fallback "
                                                 "is refined by the caller: emi_kkt_solve)", b);
        HIP_TRY(c0, hipStreamSynchronize(ctxs[b]->stream));
        ws[b] = ctxs[b]->kkt;
    }
    std::string err;
    st = emi::kkt_solve_refined_batch(n, ws.data(), c0->stream, rhs, dc_nominal, max_steps, rel, nsolve, reverted, status, &err);
    if (st) c0->err = err;
    return st;
}

int emi_kkt_solve_refined(emi_ctx_t c, double* rhs, double dc_nominal, int max_steps, double* rel, int* nsolve, int* reverted, int* status) {
    if (!c) return EMI_ERR_ARG;
    double* r1 = rhs;
    return emi_kkt_solve_refined_batch(1, &c, &r1, &dc_nominal, max_steps, rel, nsolve, reverted, status);
}

int emi_kkt_is_schur(emi_ctx_t c) { return c && emi::kkt_is_schur(c->kkt) ? 1 : 0; }

int emi_kkt_last_regularisation(emi_ctx_t c, double* dc, double* dw) {
    if (!c || (!dc && !dw)) return EMI_ERR_ARG;
    if (!c->kkt) return fail(c, EMI_ERR_STATE, "emi_kkt_last_regularisation: no factorisation");
    emi::kkt_last_regularisation(c->kkt, dc, dw);
    return EMI_OK;
}

// emi_kkt_solve / emi_kkt_solve_dev: the right-hand sides in host or in device memory, everything else the same
static int kkt_solve_from(emi_ctx_t c, void* rhs, int nrhs, bool on_device) {
    if (!c || !rhs || nrhs < 1) return EMI_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    std::string err;
    const int st = emi::kkt_solve(c->kkt, c->stream, (c->ns + c->nc) * c->M, (double*)rhs, nrhs, &err, on_device);
    if (st) c->err = err;
    return st;
}

int emi_kkt_solve(emi_ctx_t c, double* rhs, int nrhs) { return kkt_solve_from(c, rhs, nrhs, false); }

int emi_kkt_solve_dev(emi_ctx_t c, void* dRhs, int nrhs) { return kkt_solve_from(c, dRhs, nrhs, true); }

// ---- the Newton steps of a context's whole batch, device arrays in and out (the workspaces of c->kkt_shard) ------------------
int emi_kkt_factor_shard_dev(emi_ctx_t c, const void* dQ, const void* dVALS, const void* dFixed, const double* dc, const unsigned char* mask,
                             int* info) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(shard_check(c, "emi_kkt_factor_shard_dev"));
    if (!dQ || !dVALS || !dFixed || !dc || !info) return fail(c, EMI_ERR_ARG, "emi_kkt_factor_shard_dev: null argument");
    std::vector<int> inst;
    EMI_TRY(shard_members(c, "emi_kkt_factor_shard_dev", mask, 0, inst));
    for (int b : inst)
        if (!(dc[b] >= 0.0)) return fail(c, EMI_ERR_ARG, "emi_kkt_factor_shard_dev: dc[%d] = %g", b, dc[b]);
    if (inst.empty()) return EMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((int)c->kkt_shard.size() < c->B) c->kkt_shard.resize((size_t)c->B, nullptr);
    const int n = (int)inst.size(), M = c->M, ns = c->ns, nv = c->ns + c->nc, nh = nv * (nv + 1) / 2;
    const size_t vals_stride = (size_t)nvals_of(c) * M;
    std::vector<emi::KktWorkspace**> pws(n);
    std::vector<const double*> dD(n, (const double*)c->d_D.p);
    std::vector<double> dcs(n);
    std::vector<int> inf(n, -1);
    for (int a = 0; a < n; ++a) { pws[a] = &c->kkt_shard[inst[a]]; dcs[a] = dc[inst[a]]; }
    const emi::KktShardSrc src{(const double*)dQ, (const double*)dVALS, (const unsigned char*)dFixed, vals_stride, inst.data()};
    std::string err;
    int st = emi::kkt_factor_batch(n, pws.data(), c->stream, dD.data(), M, ns, nv, nullptr, nullptr, nullptr, dcs.data(), inf.data(), &err, &src);
    if (st) { c->err = err; return st; }
    // instances the batch could not take (a node block not positive definite, the ladder exhausted): the single path with its LU,
    // on the instance's own workspace and slices
    for (int a = 0; a < n; ++a) {
        const int b = inst[a];
        if (inf[a] < 0) {
            st = emi::kkt_factor(&c->kkt_shard[b], c->stream, (const double*)c->d_D.p, M, ns, nv, (const double*)dQ + (size_t)b * nh * M,
                                 (const double*)dVALS + (size_t)b * vals_stride, (const unsigned char*)dFixed + (size_t)b * nv * M, dc[b], 1,
                                 &inf[a], &err, true);
            if (st) { c->err = err; return st; }
        }
        info[b] = inf[a];
    }
    return EMI_OK;
}

int emi_kkt_lowrank_shard_dev(emi_ctx_t c, int max_mods, const void* dCount, const void* dNode, const void* dDelta, const void* dVec,
                              const unsigned char* mask, int* exact) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(shard_check(c, "emi_kkt_lowrank_shard_dev"));
    if (max_mods < 0 || !exact || (max_mods > 0 && (!dCount || !dNode || !dDelta || !dVec)))
        return fail(c, EMI_ERR_ARG, "emi_kkt_lowrank_shard_dev: bad argument");
    std::vector<int> inst;
    EMI_TRY(shard_members(c, "emi_kkt_lowrank_shard_dev", mask, 1, inst));
    if (inst.empty()) return EMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const int n = (int)inst.size();
    std::vector<int> all((size_t)c->B, 0), cnt(n, 0), ex(n, 0);
    if (max_mods > 0) {             // the counts: the one download of this call
        HIP_TRY(c, hipMemcpyAsync(all.data(), dCount, (size_t)c->B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    std::vector<emi::KktWorkspace*> ws(n);
    for (int a = 0; a < n; ++a) {
        ws[a] = c->kkt_shard[inst[a]];
        // max_mods == 0 clears: no list is read, every instance is taken as unmodified (exact, no correction), as emi_kkt_lowrank with r = 0
        cnt[a] = max_mods > 0 ? std::max(all[inst[a]], 0) : 0;
    }
    std::string err;
    const int st = emi::kkt_lowrank_shard(n, ws.data(), c->stream, max_mods, inst.data(), cnt.data(), (const int*)dNode, (const double*)dDelta,
                                          (const double*)dVec, ex.data(), &err);
    if (st) { c->err = err; return st; }
    for (int a = 0; a < n; ++a) exact[inst[a]] = ex[a];
    return EMI_OK;
}

int emi_kkt_solve_shard_dev(emi_ctx_t c, void* dRhs, const unsigned char* mask) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(shard_check(c, "emi_kkt_solve_shard_dev"));
    if (!dRhs) return fail(c, EMI_ERR_ARG, "emi_kkt_solve_shard_dev: null argument");
    std::vector<int> inst;
    EMI_TRY(shard_members(c, "emi_kkt_solve_shard_dev", mask, 1, inst));
    HIP_TRY(c, hipSetDevice(c->device));
    const int nv = c->ns + c->nc, nz = nv * c->M;
    const size_t N = (size_t)(nv + c->ns) * c->M;
    // instances that hold the LU fallback go through the single solve; the rest as one batch
    std::vector<emi::KktWorkspace*> ws;
    std::vector<double*> rb;
    std::string err;
    for (int b : inst) {
        emi::KktWorkspace* w = c->kkt_shard[b];
        double* x = (double*)dRhs + (size_t)b * N;
        if (emi::kkt_is_schur(w)) { ws.push_back(w); rb.push_back(x); }
        else if (int st = emi::kkt_solve(w, c->stream, nz, x, 1, &err, true)) { c->err = err; return st; }
    }
    if (ws.empty()) return EMI_OK;
    const int st = emi::kkt_solve_batch((int)ws.size(), ws.data(), c->stream, nz, rb.data(), &err, true);
    if (st) c->err = err;
    return st;
}

int emi_kkt_solve_refined_shard_dev(emi_ctx_t c, void* dRhs, const unsigned char* mask, const double* dc_nominal, int max_steps, double* rel,
                                    int* nsolve, int* reverted, int* status) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(shard_check(c, "emi_kkt_solve_refined_shard_dev"));
    if (!dRhs || !dc_nominal || !rel || !nsolve || !reverted || !status || max_steps < 0)
        return fail(c, EMI_ERR_ARG, "emi_kkt_solve_refined_shard_dev: bad argument");
    std::vector<int> inst;
    EMI_TRY(shard_members(c, "emi_kkt_solve_refined_shard_dev", mask, 2, inst));
    for (int b : inst)
        if (!(dc_nominal[b] >= 0.0)) return fail(c, EMI_ERR_ARG, "emi_kkt_solve_refined_shard_dev: dc_nominal[%d] = %g", b, dc_nominal[b]);
    if (inst.empty()) return EMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const int n = (int)inst.size();
    const size_t N = (size_t)(2 * c->ns + c->nc) * c->M;
    std::vector<emi::KktWorkspace*> ws(n);
    std::vector<double*> rb(n);
    std::vector<double> dcn(n), r(n);
    std::vector<int> nsv(n), rev(n), sta(n);
    for (int a = 0; a < n; ++a) { ws[a] = c->kkt_shard[inst[a]]; rb[a] = (double*)dRhs + (size_t)inst[a] * N; dcn[a] = dc_nominal[inst[a]]; }
    std::string err;
    const int st = emi::kkt_solve_refined_batch(n, ws.data(), c->stream, rb.data(), dcn.data(), max_steps, r.data(), nsv.data(), rev.data(),
                                                sta.data(), &err, true);
    if (st) { c->err = err; return st; }
    for (int a = 0; a < n; ++a) { rel[inst[a]] = r[a]; nsolve[inst[a]] = nsv[a]; reverted[inst[a]] = rev[a]; status[inst[a]] = sta[a]; }
    return EMI_OK;
}

}  // extern "C"
