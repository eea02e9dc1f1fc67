// emi_api.hip -- device side of the C ABI declared in include/emi355x.h: the context itself.  Create / destroy / stream /
// synchronise, the setters (mesh, model, batch, delays, path, tracks), the layout, device memory for the caller, the options,
// the timer and the profile; and the helpers of emi_ctx.hpp that every part shares.  The evaluation pass is in emi_api_pass.hip,
// the adjoint pass in emi_api_adjoint.hip, the Newton step in emi_api_kkt.hip, the interior-point calls in emi_api_ipm.hip.
#include "emi_ctx.hpp"

using namespace emi_api;

int emi_api::fail(emi_ctx_t c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

int emi_api::upload_bytes(emi_ctx_t c, DevBuf& b, const void* src, size_t bytes) {
    EMI_TRY(ensure(c, b, bytes));
    if (bytes == 0) return EMI_OK;
    HIP_TRY(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}

int emi_api::upload_real(emi_ctx_t c, DevBuf& b, const double* src, size_t n) {
    if (!c->f32) return upload_bytes(c, b, src, n * 8);
    std::vector<float> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = (float)src[i];
    return upload_bytes(c, b, tmp.data(), n * 4);
}

int emi_api::download_real(emi_ctx_t c, double* dst, const void* dsrc, size_t n) {
    if (!dst || n == 0) return EMI_OK;
    std::vector<float> tmp(c->f32 ? n : 0);
    HIP_TRY(c, hipMemcpyAsync(c->f32 ? (void*)tmp.data() : (void*)dst, dsrc, n * (c->f32 ? 4 : 8), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < tmp.size(); ++i) dst[i] = tmp[i];
    return EMI_OK;
}

int emi_api::ensure_vals_staging(emi_ctx_t c, size_t bytes) {
    if (c->s_VALS.bytes() < bytes) c->keep.written(c->s_VALS.p);
    return ensure(c, c->s_VALS, bytes);
}

void* emi_api::HostStager::place(const void* host, size_t bytes, bool in, bool out) {
    if (!host || status) return nullptr;
    if (slot == c->host_stage.size()) c->host_stage.emplace_back();
    DevBuf& b = c->host_stage[slot++];
    if (b.reserve(std::max<size_t>(bytes, 8)) != hipSuccess) { status = fail(c, EMI_ERR_HIP, "staging of a host-form call: out of device memory"); return nullptr; }
    if (in && bytes && hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        status = fail(c, EMI_ERR_HIP, "staging of a host-form call: copy failed");
        return nullptr;
    }
    if (out) outs.push_back({const_cast<void*>(host), b.p, bytes});
    return b.p;
}

int emi_api::HostStager::finish() {
    for (const Out& o : outs)
        if (o.bytes) HIP_TRY(c, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}

bool emi_api::even_odd_halves(int M, const double* D, std::vector<double>& De, std::vector<double>& Do) {
    if (M % 2 != 0) return false;
    const int N = M - 1, Hh = M / 2;
    for (int i = 0; i < M; ++i)
        for (int j = 0; j < M; ++j)
            if (D[(size_t)i * M + j] != -D[(size_t)(N - i) * M + (N - j)]) return false;
    De.assign((size_t)Hh * Hh, 0.0);
    Do.assign((size_t)Hh * Hh, 0.0);
    for (int i = 0; i < Hh; ++i)
        for (int j = 0; j < Hh; ++j) {
            const double p = D[(size_t)i * M + j], q = D[(size_t)i * M + (N - j)];
            De[(size_t)i * Hh + j] = 0.5 * (p + q);
            Do[(size_t)i * Hh + j] = 0.5 * (p - q);
        }
    return true;
}

namespace {

// ---- emi_set_option: the plain options, one row each (what the name means is said at the member it sets) -------------------
struct OptionRow {
    const char* name;
    int emi_ctx_s::*member;
    bool (*accepts)(int);       // the range or set of values taken ...
    int (*stored)(int);         // ... what an accepted value is stored as ...
    const char* message;        // ... and what emi_last_error says about any other
};
template <int LO, int HI> bool within(int v) { return v >= LO && v <= HI; }
template <int... VS> bool one_of(int v) { return ((v == VS) || ...); }
bool any_value(int) { return true; }
bool at_least_0(int v) { return v >= 0; }
bool whole_tiles(int v) { return v >= 0 && v % 16 == 0; }
int as_given(int v) { return v; }
int as_flag(int v) { return v != 0; }
int ring_wgs(int v) { return v == 1 ? 1 : 2; }
int block_order(int v) { return v < 0 ? -1 : (v >= 100 ? v : (v != 0)); }

const OptionRow OPTIONS[] = {
    {"overlap", &emi_ctx_s::allow_fused, any_value, as_flag, nullptr},
    {"fused", &emi_ctx_s::allow_fused, any_value, as_flag, nullptr},
    {"sym_ct", &emi_ctx_s::sym_ct, within<0, 8>, as_given,
     "sym_ct must be 0..8 (0/4 = chosen from the batch, 3 = LDS-DMA ring, 5..8 = state-split ring with SW = NS/2/1/3)"},
    {"small_rows", &emi_ctx_s::small_rows, at_least_0, as_given, "small_rows must be >= 0 (0 disables the skinny defect kernel)"},
    {"sym_order", &emi_ctx_s::sym_order, any_value, as_flag, nullptr},
    {"f32_ring", &emi_ctx_s::f32_ring, any_value, as_flag, nullptr},
    {"f32_ring_wgs", &emi_ctx_s::f32_ring_wgs, any_value, ring_wgs, nullptr},
    {"f32_one_launch", &emi_ctx_s::f32_one_launch, any_value, as_flag, nullptr},
    {"slice", &emi_ctx_s::slice, whole_tiles, as_given, "slice must be 0 (never) or a multiple of 16 instances"},
    {"pass_order", &emi_ctx_s::pass_order, any_value, block_order, nullptr},
    {"sym_ablate", &emi_ctx_s::sym_ablate, any_value, as_given, nullptr},   // diagnostics only
    {"adj_fold_tile", &emi_ctx_s::adj_fold_tile, within<0, 2>, as_given, "adj_fold_tile must be 0 (by size), 1 (48 x 64) or 2 (96 x 128)"},
    {"cost_in_kernel", &emi_ctx_s::cost_in_kernel, any_value, as_flag, nullptr},
    {"sym_nst", &emi_ctx_s::sym_nst, one_of<3, 4>, as_given, "sym_nst must be 3 or 4"},
    {"sym_hs", &emi_ctx_s::sym_hs, within<0, 2>, as_given, "sym_hs must be 0 (by batch size), 1 or 2"},
    {"sym_ctc", &emi_ctx_s::sym_ctc, within<0, 2>, as_given, "sym_ctc must be 0 (by batch size), 1 or 2"},
    {"sym_bk", &emi_ctx_s::sym_bk, one_of<0, 8, 16>, as_given, "sym_bk must be 0 (by batch size), 8 or 16"},
    {"sym_dop", &emi_ctx_s::sym_dop, within<0, 2>, as_given, "sym_dop must be 0 (by batch size), 1 (De / Do through the operand ring) or 2 (straight from L2)"},
    {"sym_res", &emi_ctx_s::sym_res, one_of<0, 2, 3>, as_given,
     "sym_res must be 0 (by batch size), 2 or 3 resident workgroups per CU (3: granted to the De / Do from L2 forms only)"},
    {"sym_cpart", &emi_ctx_s::sym_cpart, one_of<-1, 0, 1, 2, 4, 8>, as_given, "sym_cpart must be -1 (plain order), 0 (by mesh size), 1, 2, 4 or 8"},
    {"sym_gblk", &emi_ctx_s::sym_gblk, within<0, 64>, as_given, "sym_gblk must be 0 (off) .. 64 instance groups per super-block"},
    {"sym_cx", &emi_ctx_s::sym_cx, within<0, 64>, as_given, "sym_cx must be 0 (default) .. 64 column tiles per block"},
    {"sym_combine", &emi_ctx_s::sym_combine, any_value, as_flag, nullptr},
    {"sym_ksplit", &emi_ctx_s::sym_ksplit, one_of<0, 1, 2, 4, 8>, as_given, "sym_ksplit must be 0 (by batch size), 1, 2, 4 or 8"},
    {"node_store", &emi_ctx_s::node_store, within<-1, 3>, as_given,
     "node_store must be -1 (by size), 0 (plain), 1 (write-through sc1), 2 (non-temporal) or 3 (nt sc1; the one-launch pass only)"},
    {"overlap_mode", &emi_ctx_s::overlap_mode, within<0, 3>, as_given,
     "overlap_mode must be 0 (by batch size), 1 (one stream), 2 (two streams) or 3 (one launch)"},
};

}  // namespace

extern "C" {

int emi_device_count(int* count) {
    if (!count) return EMI_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return EMI_OK;
}

static int create_impl(int device_id, bool f32, emi_ctx_t* out) {
    if (!out) return EMI_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return EMI_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= n) return EMI_ERR_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return EMI_ERR_HIP;
    // gfx950 only: the code object holds no other ISA
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return EMI_ERR_NO_DEVICE;
    if (hipSetDevice(device_id) != hipSuccess) return EMI_ERR_HIP;
    emi_ctx_t c = new emi_ctx_s();
    c->device = device_id;
    c->f32 = f32;
    c->own_stream = true;
    // (stream2 is created when a two-stream form first asks for it, need_stream2: every stream takes a share of one of the runtime's few
    // hardware queues, and a Monte-Carlo run has a context per host thread)
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreate(&c->t_start) != hipSuccess || hipEventCreate(&c->t_stop) != hipSuccess) {
        delete c;               // (the destructor releases what was created before the failure)
        return EMI_ERR_HIP;
    }
    *out = c;
    return EMI_OK;
}

int emi_create(int device_id, emi_ctx_t* out) { return create_impl(device_id, false, out); }
int emi_create_f32(int device_id, emi_ctx_t* out) { return create_impl(device_id, true, out); }

int emi_destroy(emi_ctx_t c) {
    if (!c) return EMI_ERR_ARG;
    delete c;
    return EMI_OK;
}

const char* emi_last_error(emi_ctx_t c) { return c ? c->err.c_str() : "null context"; }

int emi_set_stream(emi_ctx_t c, void* s) {
    if (!c) return EMI_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (s == nullptr) {
        if (!c->own_stream) {
            HIP_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
            c->own_stream = true;
        }
        return EMI_OK;
    }
    if (c->own_stream) { HIP_TRY(c, hipStreamDestroy(c->stream)); c->own_stream = false; }
    c->stream = (hipStream_t)s;
    return EMI_OK;
}

int emi_get_stream(emi_ctx_t c, void** s) {
    if (!c || !s) return EMI_ERR_ARG;
    *s = (void*)c->stream;
    return EMI_OK;
}

int emi_synchronize(emi_ctx_t c) {
    if (!c) return EMI_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}

// the differentiation matrix of a collocation mesh on the device: D itself (fp32 contexts: a copy whose rows sum to zero), and for
// an exactly centro-antisymmetric D on an even number of nodes its even/odd halves De / Do (c->symmetric says whether they are valid)
static int upload_operator(emi_ctx_t c, int M, const double* D) {
    if (c->f32) {
        // f32 copy of D whose rows sum to EXACTLY zero in f32 arithmetic terms: off-diagonals rounded,
        // diagonal = -(f64 sum of the rounded off-diagonals), rounded.  The shifted-difference form of
        // the f32 defect kernel (emi_defect_f32.hip) relies on it.
        std::vector<float> Df((size_t)M * M);
        for (int i = 0; i < M; ++i) {
            double rs = 0.0;
            for (int j = 0; j < M; ++j) {
                if (j == i) continue;
                Df[(size_t)i * M + j] = (float)D[(size_t)i * M + j];
                rs += (double)Df[(size_t)i * M + j];
            }
            Df[(size_t)i * M + i] = (float)(-rs);
        }
        return upload_bytes(c, c->d_D, Df.data(), Df.size() * 4);
    }
    EMI_TRY(upload_real(c, c->d_D, D, (size_t)M * M));
    // even/odd split of D for the fused kernel: valid only for an exactly centro-antisymmetric D
    std::vector<double> De, Do;
    if (!even_odd_halves(M, D, De, Do)) return EMI_OK;
    EMI_TRY(upload_real(c, c->d_De, De.data(), De.size()));
    EMI_TRY(upload_real(c, c->d_Do, Do.data(), Do.size()));
    c->symmetric = true;
    if (M % 128 == 0) {         // what the one-launch pass takes: the same panels once more, in the order its MFMA waves consume them
        std::vector<double> frag(De.size() + Do.size());
        emi::operator_fragments(M, De.data(), Do.data(), frag.data());
        EMI_TRY(upload_real(c, c->d_Dfrag, frag.data(), frag.size()));
        c->has_dfrag = true;
    }
    return EMI_OK;
}

int emi_set_mesh(emi_ctx_t c, int M, const double* tau, const double* w, const double* D, double t0,
                 double tf) {
    if (!c || M < 2 || !tau || !w) return fail(c, EMI_ERR_ARG, "emi_set_mesh: bad argument");
    if (!(tf > t0)) return fail(c, EMI_ERR_ARG, "emi_set_mesh: tf must exceed t0");
    c->keep.bump();             // h, D_kk and the weights enter the invariant rows of VALS
    HIP_TRY(c, hipSetDevice(c->device));
    // D == NULL is a points-only mesh: the node functions are evaluated at arbitrary abscissae (the ODE-error estimate between
    // the collocation nodes); there is no differentiation matrix, so EMI_EVAL_DEFECT and the KKT entry points refuse
    const double h = (tf - t0) / 2.0;
    std::vector<double> nt(M), dd(M, 0.0);
    for (int k = 0; k < M; ++k) {
        nt[k] = t0 + h * (tau[k] + 1.0);
        if (D) dd[k] = D[(size_t)k * M + k];
    }
    EMI_TRY(upload_real(c, c->d_w, w, M));
    EMI_TRY(upload_real(c, c->d_t, nt.data(), M));
    EMI_TRY(upload_real(c, c->d_Ddiag, dd.data(), M));
    c->symmetric = false;
    c->has_dfrag = false;
    if (D) EMI_TRY(upload_operator(c, M, D));
    c->points_only = !D;
    c->h_tau.assign(tau, tau + M);
    c->h_w.assign(w, w + M);
    c->M = M;
    c->t0 = t0;
    c->tf = tf;
    c->adj_dirty = true;
    c->ode_dirty = true;
    c->delay_dirty = true;      // W(delay) is built for one mesh: [nd][M][M] on these nodes and this horizon
    c->odel_dirty = true;       // ... and so are the delayed blocks of the ODE-error operator
    c->adjw_dirty = true;
    emi::kkt_mesh_changed(c->kkt);
    for (emi::KktWorkspace* w : c->kkt_shard) emi::kkt_mesh_changed(w);
    // tables sized by M are stale now
    c->ntracks = 0;
    c->track_sets = 0;
    c->wp_nt_dirty = true;      // (the waypoint tables themselves are not per mesh and stay)
    // the per-block cost partials are sized B * node_chunks(M): keep them valid for the batch already set
    if (c->B > 0) EMI_TRY(ensure(c, c->d_cost_part, (size_t)c->B * emi::node_chunks(M) * (c->f32 ? 4 : 8)));
    return EMI_OK;
}

// A new model is in force: its dimensions, the traced rows it computes itself (run-time compiled models) and its parameters.
// What was declared for the previous model goes: delayed values (emi_set_delays again) and the path rows, which name states
// (px, py) that this model may not have.
static void model_in_force(emi_ctx_t c, int model, int ns, int nc, int npath, const int* path_vars, int n_path_vars,
                           const double* params, int nparams, int maximize) {
    c->keep.bump();             // the model, its parameters and the cost sign
    c->model = model;
    c->ns = ns;
    c->nc = nc;
    c->xh = c->uh = c->nch = 0;
    c->np_model = npath;
    c->pvars.assign(path_vars, path_vars + n_path_vars);
    c->maximize = maximize ? 1 : 0;
    memset(c->params, 0, sizeof c->params);
    for (int i = 0; i < nparams; ++i) c->params[i] = params[i];
    c->nparams = nparams;
    c->ptab_sets = 0;           // a per-instance table was the previous model's
    c->h_ptab.clear();
    c->np = 0;
    c->path_sets = 0;
    c->path_has_track = false;
}

int emi_set_model(emi_ctx_t c, int model, const double* params, int nparams, int maximize) {
    if (!c) return EMI_ERR_ARG;
    int ns, nc, np_expected;
    if (emi_model_dims(model, &ns, &nc, &np_expected)) return fail(c, EMI_ERR_ARG, "unknown model %d", model);
    if (nparams != np_expected || (nparams > 0 && !params))
        return fail(c, EMI_ERR_ARG, "model %d takes %d parameters, got %d", model, np_expected, nparams);
    if (c->rtc) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        emi::rtc_destroy(c->rtc);
        c->rtc = nullptr;
    }
    model_in_force(c, model, ns, nc, 0, nullptr, 0, params, nparams, maximize);
    return EMI_OK;
}

int emi_set_model_source(emi_ctx_t c, const char* struct_name, const char* source, int ns, int nc, int npath,
                         const int* path_vars, int n_path_vars, const double* params, int nparams, int maximize) {
    if (!c) return EMI_ERR_ARG;
    if (npath < 0 || npath > 64) return fail(c, EMI_ERR_ARG, "emi_set_model_source: npath must be in [0, 64]");
    if (npath > 0 && (!path_vars || n_path_vars < 1 || n_path_vars > ns + nc))
        return fail(c, EMI_ERR_ARG, "emi_set_model_source: %d traced rows need the list of variables they depend on", npath);
    for (int q = 0; q < (npath > 0 ? n_path_vars : 0); ++q)
        if (path_vars[q] < 0 || path_vars[q] >= ns + nc || (q > 0 && path_vars[q] <= path_vars[q - 1]))
            return fail(c, EMI_ERR_ARG, "emi_set_model_source: path_vars must be ascending node-variable indices below %d", ns + nc);
    if (nparams < 0 || nparams > EMI_MAX_PARAMS || (nparams > 0 && !params))
        return fail(c, EMI_ERR_ARG, "emi_set_model_source: at most %d parameters", EMI_MAX_PARAMS);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    emi::RtcModel* m = nullptr;
    std::string log;
    const int st = emi::rtc_build(c->f32, struct_name, source, ns, nc, npath, npath > 0 ? n_path_vars : 0, &m, &log);
    if (st) {
        c->err = log;
        return st;
    }
    emi::rtc_destroy(c->rtc);
    c->rtc = m;
    model_in_force(c, EMI_MODEL_SOURCE, ns, nc, npath, path_vars, npath > 0 ? n_path_vars : 0, params, nparams, maximize);
    return EMI_OK;
}

int emi_check_model_source(const char* struct_name, const char* source, int ns, int nc, int npath, int n_path_vars, int f32,
                           char* log, size_t log_len) {
    std::string l;
    const int st = emi::rtc_check(f32 != 0, struct_name, source, ns, nc, npath, npath > 0 ? n_path_vars : 0, &l);
    if (log && log_len) {
        strncpy(log, l.c_str(), log_len - 1);
        log[log_len - 1] = '\0';
    }
    return st;
}

int emi_set_batch(emi_ctx_t c, int B) {
    if (!c || B < 1) return fail(c, EMI_ERR_ARG, "emi_set_batch: B must be >= 1");
    if (c->M <= 0) return fail(c, EMI_ERR_STATE, "emi_set_mesh must precede emi_set_batch");
    c->keep.bump();
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t rb = c->f32 ? 4 : 8;
    int st = ensure(c, c->d_cost_part, (size_t)B * emi::node_chunks(c->M) * rb);
    if (st) return st;
    if (B != c->B) {            // a per-instance parameter table is one row per instance of the batch it was set for
        c->ptab_sets = 0;
        c->h_ptab.clear();
    }
    c->B = B;
    return EMI_OK;
}

int emi_set_model_params_batch(emi_ctx_t c, const double* params, int nsets, int nparams) {
    if (!c) return EMI_ERR_ARG;
    if (c->model < 0) return fail(c, EMI_ERR_STATE, "emi_set_model / emi_set_model_source must precede emi_set_model_params_batch");
    if (c->B <= 0) return fail(c, EMI_ERR_STATE, "emi_set_batch must precede emi_set_model_params_batch");
    if (nsets == 0) {           // back to the shared set of emi_set_model*
        if (c->ptab_sets > 0) c->keep.bump();
        c->ptab_sets = 0;
        c->h_ptab.clear();
        return EMI_OK;
    }
    if (nsets != c->B) return fail(c, EMI_ERR_ARG, "emi_set_model_params_batch: %d sets, the batch is %d (0 removes the table)", nsets, c->B);
    if (nparams != c->nparams || (nparams > 0 && !params))
        return fail(c, EMI_ERR_ARG, "emi_set_model_params_batch: the model takes %d parameters, got %d", c->nparams, nparams);
    if (c->nch > 0)
        return fail(c, EMI_ERR_UNSUPPORTED, "emi_set_model_params_batch: contexts with delays (emi_set_delays) take the shared parameter set only");
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<double> rows((size_t)nsets * EMI_MAX_PARAMS, 0.0);
    for (int b = 0; b < nsets; ++b)
        for (int i = 0; i < nparams; ++i) rows[(size_t)b * EMI_MAX_PARAMS + i] = params[(size_t)b * nparams + i];
    c->keep.bump();             // the model-invariant rows of VALS are functions of the parameters
    EMI_TRY(upload_real(c, c->d_ptab, rows.data(), rows.size()));      // (rounded once, as fill_node_args rounds the shared set)
    c->h_ptab.assign(params, params + (size_t)nsets * nparams);
    c->ptab_sets = nsets;
    return EMI_OK;
}

int emi_get_model_params_batch(emi_ctx_t c, double* params, int* nsets, int* nparams) {
    if (!c) return EMI_ERR_ARG;
    if (nsets) *nsets = c->ptab_sets;
    if (nparams) *nparams = c->model < 0 ? 0 : c->nparams;
    if (params && c->ptab_sets > 0) std::copy(c->h_ptab.begin(), c->h_ptab.end(), params);
    return EMI_OK;
}

int emi_set_delays(emi_ctx_t c, int x_horizon, int u_horizon, double dt) {
    if (!c || x_horizon < 0 || u_horizon < 0) return fail(c, EMI_ERR_ARG, "emi_set_delays: horizons must be >= 0");
    if (c->model < 0) return fail(c, EMI_ERR_STATE, "emi_set_model / emi_set_model_source must precede emi_set_delays");
    if (has_param_table(c) && std::max(x_horizon - 1, 0) * c->ns + u_horizon > 0)
        return fail(c, EMI_ERR_UNSUPPORTED, "emi_set_delays: the context holds a per-instance parameter table (emi_set_model_params_batch), "
                    "which contexts with delays do not take");
    c->keep.bump();
    const int nxd = std::max(x_horizon - 1, 0) * c->ns;
    // nc_free + nxd + uh * nc_free = nc  (the model's control count includes the delayed values)
    const int rest = c->nc - nxd;
    if (nxd + u_horizon == 0) { c->xh = x_horizon; c->uh = 0; c->nch = 0; return EMI_OK; }
    if (!(dt > 0)) return fail(c, EMI_ERR_ARG, "emi_set_delays: dt must be positive");
    if (rest < 1 || rest % (1 + u_horizon) != 0)
        return fail(c, EMI_ERR_ARG, "emi_set_delays: the model has %d controls, which is not nc + %d delayed states + %d x nc delayed controls for any nc >= 1",
                    c->nc, nxd, u_horizon);
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "emi_set_delays: f64 contexts only");
    c->xh = x_horizon;
    c->uh = u_horizon;
    c->nch = c->nc - rest / (1 + u_horizon);
    c->delay_dt = dt;
    c->delay_dirty = true;
    c->odel_dirty = true;
    c->adjw_dirty = true;
    return EMI_OK;
}

int emi_get_delays(emi_ctx_t c, int* x_horizon, int* u_horizon, int* n_delayed) {
    if (!c) return EMI_ERR_ARG;
    if (x_horizon) *x_horizon = c->xh;
    if (u_horizon) *u_horizon = c->uh;
    if (n_delayed) *n_delayed = c->nch;
    return EMI_OK;
}

int emi_set_path(emi_ctx_t c, int np, int nsets, const double* recs, int px_state, int py_state) {
    if (!c || np < 0) return fail(c, EMI_ERR_ARG, "emi_set_path: bad argument");
    if (c->model < 0) return fail(c, EMI_ERR_STATE, "emi_set_model must precede emi_set_path");
    c->keep.bump();             // the row layout of VALS
    if (np > 0 && (!recs || nsets < 1)) return fail(c, EMI_ERR_ARG, "emi_set_path: null table");
    if (px_state < 0 || px_state >= c->ns || py_state < 0 || py_state >= c->ns || px_state == py_state)
        return fail(c, EMI_ERR_ARG, "emi_set_path: state indices (%d,%d) out of range", px_state, py_state);
    HIP_TRY(c, hipSetDevice(c->device));
    bool has_track = false;
    for (size_t i = 0; i < (size_t)np * nsets; ++i) {
        const int kind = (int)recs[i * EMI_PATH_REC];
        if (kind != EMI_PATH_ELLIPSE && kind != EMI_PATH_DISC && kind != EMI_PATH_TRACK)
            return fail(c, EMI_ERR_ARG, "emi_set_path: record %zu has unknown kind %d", i, kind);
        has_track = has_track || kind == EMI_PATH_TRACK;
    }
    int st = upload_real(c, c->d_path, recs, (size_t)np * nsets * EMI_PATH_REC);
    if (st) return st;
    c->path_has_track = has_track;
    c->np = np;
    c->path_sets = np > 0 ? nsets : 0;
    c->px = px_state;
    c->py = py_state;
    return EMI_OK;
}

int emi_set_tracks(emi_ctx_t c, int ntracks, int nsets, const double* xc, const double* yc) {
    if (!c || ntracks < 0) return fail(c, EMI_ERR_ARG, "emi_set_tracks: bad argument");
    if (c->M <= 0) return fail(c, EMI_ERR_STATE, "emi_set_mesh must precede emi_set_tracks");
    c->keep.bump();
    if (ntracks > 0 && (!xc || !yc || nsets < 1)) return fail(c, EMI_ERR_ARG, "emi_set_tracks: null table");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)ntracks * nsets * c->M;
    int st;
    if ((st = upload_real(c, c->d_trkx, xc, n))) return st;
    if ((st = upload_real(c, c->d_trky, yc, n))) return st;
    c->ntracks = ntracks;
    c->track_sets = ntracks > 0 ? nsets : 0;
    return EMI_OK;
}

int emi_set_track_waypoints(emi_ctx_t c, int ntracks, int nsets, int ld, const int* counts, const double* t, const double* x,
                            const double* y) {
    if (!c || ntracks < 0) return fail(c, EMI_ERR_ARG, "emi_set_track_waypoints: bad argument");
    if (ntracks == 0) {
        c->wp_ntracks = c->wp_sets = c->wp_ld = 0;
        return EMI_OK;
    }
    if (!t || !x || !y || nsets < 1) return fail(c, EMI_ERR_ARG, "emi_set_track_waypoints: null table");
    if (ld < 2) return fail(c, EMI_ERR_ARG, "emi_set_track_waypoints: ld %d is below the 2 waypoints a track needs", ld);
    const size_t rows = (size_t)nsets * ntracks, n = rows * ld;
    std::vector<int> cnt(rows, ld);
    for (size_t r = 0; r < rows; ++r) {
        const int set = (int)(r / ntracks), trk = (int)(r % ntracks);
        if (counts) cnt[r] = counts[r];
        if (cnt[r] < 2 || cnt[r] > ld)
            return fail(c, EMI_ERR_ARG, "emi_set_track_waypoints: set %d, track %d has %d waypoints (2 .. ld = %d)", set, trk, cnt[r], ld);
        for (int s = 0; s + 1 < cnt[r]; ++s)
            if (!(t[r * ld + s + 1] > t[r * ld + s]))
                return fail(c, EMI_ERR_ARG, "emi_set_track_waypoints: set %d, track %d: the times of waypoints %d and %d are not ascending", set,
                            trk, s, s + 1);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // a launch in flight may still read tables that have to move
    HIP_TRY(c, c->d_wp.reserve(3 * n));
    HIP_TRY(c, c->d_wp_cnt.reserve(rows));
    const double* src[3] = {t, x, y};
    for (int q = 0; q < 3; ++q) HIP_TRY(c, hipMemcpyAsync(c->d_wp.p + q * n, src[q], n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_wp_cnt.p, cnt.data(), rows * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->wp_ntracks = ntracks;
    c->wp_sets = nsets;
    c->wp_ld = ld;
    return EMI_OK;
}

int emi_tracks_from_waypoints_dev(emi_ctx_t c, int n, const void* dSetMap) {
    if (!c) return EMI_ERR_ARG;
    if (c->M <= 0) return fail(c, EMI_ERR_STATE, "emi_set_mesh must precede emi_tracks_from_waypoints_dev");
    if (c->wp_ntracks <= 0) return fail(c, EMI_ERR_STATE, "emi_tracks_from_waypoints_dev: emi_set_track_waypoints has not been called");
    if (n < 0 || (!dSetMap && n != 0 && n != c->wp_sets) || (dSetMap && n == 0))
        return fail(c, EMI_ERR_ARG, "emi_tracks_from_waypoints_dev: n = %d (without a map 0 or the table's %d sets, with one >= 1)", n, c->wp_sets);
    const int sets = dSetMap ? n : c->wp_sets;
    if ((long long)sets * c->wp_ntracks > 0x7fffffffLL) return fail(c, EMI_ERR_ARG, "emi_tracks_from_waypoints_dev: %d sets of %d tracks", sets, c->wp_ntracks);
    c->keep.bump();
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t total = (size_t)sets * c->wp_ntracks * c->M, rb = c->f32 ? 4 : 8, wn = (size_t)c->wp_sets * c->wp_ntracks * c->wp_ld;
    EMI_TRY(ensure(c, c->d_trkx, total * rb));
    EMI_TRY(ensure(c, c->d_trky, total * rb));
    const double* node_t = (const double*)c->d_t.p;
    if (c->f32) {               // d_t holds the rounded times; the centres are those of the double ones
        if (c->wp_nt_dirty || c->d_wp_nt.cap < (size_t)c->M) {
            const double h = (c->tf - c->t0) / 2.0;
            std::vector<double> nt(c->M);
            for (int k = 0; k < c->M; ++k) nt[k] = c->t0 + h * (c->h_tau[k] + 1.0);
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, c->d_wp_nt.reserve(nt.size()));
            HIP_TRY(c, hipMemcpyAsync(c->d_wp_nt.p, nt.data(), nt.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            c->wp_nt_dirty = false;
        }
        node_t = c->d_wp_nt.p;
    }
    const emi::TrackWaypointArgs a{c->d_wp.p, c->d_wp.p + wn, c->d_wp.p + 2 * wn, node_t, c->d_wp_cnt.p, (const int*)dSetMap,
                                   c->d_trkx.p, c->d_trky.p, sets, c->wp_ntracks, c->wp_ld, c->M, 0};
    HIP_TRY(c, c->f32 ? emi::launch_track_waypoints<float>(a, c->stream) : emi::launch_track_waypoints<double>(a, c->stream));
    c->ntracks = c->wp_ntracks;
    c->track_sets = sets;
    return EMI_OK;
}

int emi_get_tracks(emi_ctx_t c, double* xc, double* yc) {
    if (!c || !xc || !yc) return fail(c, EMI_ERR_ARG, "emi_get_tracks: null argument");
    if (c->M <= 0 || c->ntracks <= 0 || c->track_sets <= 0)
        return fail(c, EMI_ERR_STATE, "emi_get_tracks: the context holds no centres (emi_set_tracks or emi_tracks_from_waypoints_dev on this mesh)");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->track_sets * c->ntracks * c->M;
    EMI_TRY(download_real(c, xc, c->d_trkx.p, n));
    return download_real(c, yc, c->d_trky.p, n);
}

int emi_get_layout(emi_ctx_t c, emi_layout_t* o) {
    if (!c || !o) return EMI_ERR_ARG;
    o->model = c->model;
    o->ns = c->ns;
    o->nc = c->nc;
    o->np = np_total(c);
    o->M = c->M;
    o->B = c->B;
    o->nres = nres_of(c);
    o->nvals = nvals_of(c);
    o->nhess = nhess_of(c);
    o->real_bytes = c->f32 ? 4 : 8;
    o->px = c->px;
    o->py = c->py;
    o->t0 = c->t0;
    o->tf = c->tf;
    return EMI_OK;
}

// Per-instance NLP numbering (DESIGN.md "NLP layout"):
//   variables   z: state i node k -> i*M + k ; control c node k -> (ns+c)*M + k
//   constraints g: defect (i,k) -> i*M + k ; events ns*M + e (e < 2 ns) ;
//                  path (j,k) -> ns*M + 2 ns + j*M + k
int emi_jac_structure(emi_ctx_t c, int* rows, int* cols) {
    if (!c || !rows || !cols) return EMI_ERR_ARG;
    if (c->M <= 0 || c->model < 0) return fail(c, EMI_ERR_STATE, "mesh and model must be set");
    const int M = c->M, ns = c->ns, nv = c->ns + c->nc;
    size_t e = 0;
    for (int i = 0; i < ns; ++i)
        for (int v = 0; v < nv; ++v)
            for (int k = 0; k < M; ++k, ++e) { rows[e] = i * M + k; cols[e] = v * M + k; }
    for (int j = 0; j < c->np; ++j)                      // rows of the record table: two partials, (px, py)
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < M; ++k, ++e) {
                rows[e] = ns * M + 2 * ns + j * M + k;
                cols[e] = (s == 0 ? c->px : c->py) * M + k;
            }
    for (int j = 0; j < c->np_model; ++j)                // traced rows: one partial per variable of the model's list
        for (size_t q = 0; q < c->pvars.size(); ++q)
            for (int k = 0; k < M; ++k, ++e) {
                rows[e] = ns * M + 2 * ns + (c->np + j) * M + k;
                cols[e] = c->pvars[q] * M + k;
            }
    for (int v = 0; v < nv; ++v)
        for (int k = 0; k < M; ++k, ++e) { rows[e] = -1; cols[e] = v * M + k; }
    return EMI_OK;
}

int emi_invariant_rows(int model, int np, unsigned char* mask, int* nvals) {
    int ns, nc;
    if (np < 0 || emi_model_dims(model, &ns, &nc, nullptr)) return EMI_ERR_ARG;
    if (nvals) *nvals = ns * (ns + nc) + 2 * np + (ns + nc);
    if (mask && !emi::invariant_rows(model, np, mask)) return EMI_ERR_ARG;
    return EMI_OK;
}

int emi_dev_alloc(emi_ctx_t c, size_t bytes, void** dptr) {
    if (!c || !dptr) return EMI_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMalloc(dptr, bytes));
    return EMI_OK;
}
int emi_dev_free(emi_ctx_t c, void* dptr) {
    if (!c) return EMI_ERR_ARG;
    HIP_TRY(c, hipFree(dptr));
    return EMI_OK;
}
int emi_h2d(emi_ctx_t c, void* dst, const void* src, size_t bytes) {
    if (!c || !dst || !src) return EMI_ERR_ARG;
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}
int emi_d2h(emi_ctx_t c, void* dst, const void* src, size_t bytes) {
    if (!c || !dst || !src) return EMI_ERR_ARG;
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}

int emi_timer_start(emi_ctx_t c) {
    if (!c) return EMI_ERR_ARG;
    HIP_TRY(c, hipEventRecord(c->t_start, c->stream));
    return EMI_OK;
}

int emi_timer_stop(emi_ctx_t c, float* ms) {
    if (!c || !ms) return EMI_ERR_ARG;
    HIP_TRY(c, hipEventRecord(c->t_stop, c->stream));
    HIP_TRY(c, hipEventSynchronize(c->t_stop));
    HIP_TRY(c, hipEventElapsedTime(ms, c->t_start, c->t_stop));
    return EMI_OK;
}

int emi_profile_enable(emi_ctx_t c, int on) {
    if (!c) return EMI_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->profile = (on >= 0 && on <= 3) ? on : 1;
    c->prof_used = 0;
    return EMI_OK;
}

int emi_profile_read(emi_ctx_t c, float* node_ms, int* node_launches, float* defect_ms,
                     int* defect_launches, float* pass_ms, int* overlapped_passes) {
    if (!c) return EMI_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->stream2) HIP_TRY(c, hipStreamSynchronize(c->stream2));
    float nm = 0, dm = 0, fm = 0;
    int nl = 0, dl = 0, fl = 0;
    for (size_t i = 0; i < c->prof_used; ++i) {
        ProfEvents& pe = c->prof[i];
        float ms = 0;
        if (pe.fused && pe.level == -1) {
            HIP_TRY(c, hipEventElapsedTime(&ms, pe.ev[K0], pe.ev[K1]));
            dm += ms; ++dl; fm += ms; ++fl;
            continue;
        }
        if (pe.fused) {
            if (pe.level == 1) {
                HIP_TRY(c, hipEventElapsedTime(&ms, pe.ev[E0], pe.ev[E1]));
                fm += ms;
            }
            ++fl;
            if (pe.level == 1 || pe.level == 2) {
                HIP_TRY(c, hipEventElapsedTime(&ms, pe.ev[K0], pe.ev[K1]));
                dm += ms;
                ++dl;
            }
            if (pe.level == 1 || pe.level == 3) {
                HIP_TRY(c, hipEventElapsedTime(&ms, pe.ev[K2], pe.ev[K3]));
                nm += ms;
                ++nl;
            }
            continue;
        }
        if (pe.has_node && pe.level != 2) {
            HIP_TRY(c, hipEventElapsedTime(&ms, pe.ev[E0], pe.ev[E1]));
            nm += ms;
            ++nl;
        }
        if (pe.has_defect && pe.level != 3) {
            HIP_TRY(c, hipEventElapsedTime(&ms, pe.ev[E1], pe.ev[E2]));
            dm += ms;
            ++dl;
        }
    }
    c->prof_used = 0;
    if (node_ms) *node_ms = nm;
    if (node_launches) *node_launches = nl;
    if (defect_ms) *defect_ms = dm;
    if (defect_launches) *defect_launches = dl;
    if (pass_ms) *pass_ms = fm;
    if (overlapped_passes) *overlapped_passes = fl;
    return EMI_OK;
}

int emi_set_option(emi_ctx_t c, const char* name, int value) {
    if (!c || !name) return EMI_ERR_ARG;
    if (strcmp(name, "cu_split") == 0) {
        // experiment: spatial instead of temporal sharing of the chip between the MFMA and the streaming kernel
        hipDeviceProp_t prop;
        HIP_TRY(c, hipGetDeviceProperties(&prop, c->device));
        const int ncu = prop.multiProcessorCount;
        if (value < 0 || value >= ncu) return fail(c, EMI_ERR_ARG, "cu_split must be in [0, %d)", ncu);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (c->s_mfma) { HIP_TRY(c, hipStreamDestroy(c->s_mfma)); c->s_mfma = nullptr; }
        if (c->s_node) { HIP_TRY(c, hipStreamDestroy(c->s_node)); c->s_node = nullptr; }
        c->cu_split = value;
        if (value > 0) {
            const int words = (ncu + 31) / 32;
            std::vector<uint32_t> m1(words, 0u), m2(words, 0u);
            for (int i = 0; i < ncu; ++i) (i < value ? m1 : m2)[i / 32] |= 1u << (i % 32);
            HIP_TRY(c, hipExtStreamCreateWithCUMask(&c->s_mfma, words, m1.data()));
            HIP_TRY(c, hipExtStreamCreateWithCUMask(&c->s_node, words, m2.data()));
            if (!c->ev_join2) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_join2, hipEventDisableTiming));
        }
        return EMI_OK;
    }
    if (strcmp(name, "blocks_generic") == 0) {      // emi_kkt_blocks_*: the run-time-nv assembly kernel also where a templated one exists
        if (value != 0 && value != 1) return fail(c, EMI_ERR_ARG, "blocks_generic must be 0 or 1");
        c->blk_generic = value;
        return EMI_OK;
    }
    if (strcmp(name, "kkt_method") == 0) {
        if (value != 0 && value != 1) return fail(c, EMI_ERR_ARG, "kkt_method must be 0 (LU) or 1 (Schur complement + Cholesky)");
        c->kkt_method = value;
        return EMI_OK;
    }
    if (strncmp(name, "kkt_", 4) == 0) {        // the process-wide switches of the Newton step (emi_kkt.hip)
        if (strcmp(name, "kkt_cholesky") == 0 && value != 1 && value != 2)
            return fail(c, EMI_ERR_ARG, "kkt_cholesky must be 1 (one-level blocked Cholesky) or 2 (two-level form from 1024 rows)");
        if (emi::kkt_set_option(name, value)) return EMI_OK;
        return fail(c, EMI_ERR_ARG, "unknown option %s", name);
    }
    for (const OptionRow& o : OPTIONS) {
        if (strcmp(name, o.name) != 0) continue;
        if (!o.accepts(value)) return fail(c, EMI_ERR_ARG, "%s", o.message);
        c->*o.member = o.stored(value);
        return EMI_OK;
    }
    return fail(c, EMI_ERR_ARG, "unknown option '%s'", name);
}

}  // extern "C"
