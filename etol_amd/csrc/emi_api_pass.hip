// emi_api_pass.hip -- the evaluation pass of the C ABI: choose_form (the ONE place that picks among the launch forms, by the policy of
// emi_pass_plan.hpp, which policy_in hands the context to), one function per launch form, emi_eval_* / emi_hess_*, the delayed values, and
// what reports the policy (emi_plan_pass, emi_last_path, emi_last_defect_kernel, the emi_debug_* calls).
#include "emi_ctx.hpp"

using namespace emi_api;

namespace {

// What the launch policy reads of a context (emi_pass_plan.hpp: plan_pass, plan_piece, store_mode_for, report_pass are pure functions of
// this and the batch).  The one place where the policy meets emi_ctx_t.
emi::PassPolicyIn policy_in(emi_ctx_t c) {
    emi::PassPolicyIn in;
    in.ns = c->ns;
    in.M = c->M;
    in.real_bytes = c->f32 ? 4 : 8;
    in.rows = nres_of(c) + nvals_of(c);
    if (c->model == EMI_MODEL_SOURCE) in.model_class = emi::rtc_has_symdefect(c->rtc) ? emi::PASS_MODEL_RTC : emi::PASS_MODEL_NONE;
    else in.model_class = emi::pass_model_supported(c->model) ? emi::PASS_MODEL_BUILTIN : emi::PASS_MODEL_NONE;
    in.rtc_sw_large = emi::rtc_pass_sw_large(c->rtc);
    in.f32 = c->f32;
    in.symmetric = c->symmetric;
    in.has_dfrag = c->has_dfrag;
    in.allow_fused = c->allow_fused;
    in.overlap_mode = c->overlap_mode;
    in.sym_ct = c->sym_ct;
    in.sym_ksplit = c->sym_ksplit;
    in.sym_cpart = c->sym_cpart;
    in.sym_gblk = c->sym_gblk;
    in.sym_cx = c->sym_cx;
    in.sym_nst = c->sym_nst;
    in.sym_hs = c->sym_hs;
    in.sym_ctc = c->sym_ctc;
    in.sym_bk = c->sym_bk;
    in.sym_dop = c->sym_dop;
    in.sym_res = c->sym_res;
    in.pass_order = c->pass_order;
    in.node_store = c->node_store;
    in.slice = c->slice;
    in.small_rows = c->small_rows;
    in.param_table = has_param_table(c);
    return in;
}

// One launch of the evaluation pass: instances [first, first + B) of the context's batch.  The whole batch as a rule; pieces of it
// where plan_piece says so.  The context is not written to on the way: the batch of a launch is this argument.
struct Launch { int first, B; bool keep = false; };      // keep: the model-invariant VALS rows are in place already (emi_eval_dev decides)
// ... and its arrays (device memory, in the context's real type), already at the launch's first instance
struct PassIO { const void *X, *U; void *RES, *VALS, *COST; };

PassIO io_at(emi_ctx_t c, const PassIO& io, int first) {
    const size_t row = (size_t)first * c->M * (c->f32 ? 4 : 8);
    return PassIO{(const char*)io.X + row * c->ns, (const char*)io.U + row * c->nc, (char*)io.RES + row * nres_of(c),
                  io.VALS ? (char*)io.VALS + row * nvals_of(c) : nullptr, (char*)io.COST + (size_t)first * (c->f32 ? 4 : 8)};
}

template <typename T>
void fill_node_args(emi_ctx_t c, Launch L, emi::NodeArgs<T>& a, const PassIO& io) {
    a.X = (const T*)io.X;
    a.U = (const T*)io.U;
    a.RES = (T*)io.RES;
    a.VALS = (T*)io.VALS;
    a.cost_part = (T*)c->d_cost_part.p + (size_t)L.first * emi::node_chunks(c->M);
    a.cost = (T*)io.COST;
    a.cost_ticket = nullptr;
    a.w = (const T*)c->d_w.p;
    a.node_t = (const T*)c->d_t.p;
    a.Ddiag = (const T*)c->d_Ddiag.p;
    a.path = (const T*)c->d_path.p + (c->path_sets > 1 ? (size_t)L.first * c->np * EMI_PATH_REC : 0);
    a.track_x = (const T*)c->d_trkx.p + (c->track_sets > 1 ? (size_t)L.first * c->ntracks * c->M : 0);
    a.track_y = (const T*)c->d_trky.p + (c->track_sets > 1 ? (size_t)L.first * c->ntracks * c->M : 0);
    a.M = c->M;
    a.B = L.B;
    a.np = np_total(c);
    a.nres = nres_of(c);
    a.nvals = nvals_of(c);
    a.path_sets = c->path_sets;
    a.track_sets = c->track_sets;
    a.ntracks = c->ntracks;
    a.px = c->px;
    a.py = c->py;
    a.store_mode = emi::store_mode_for(policy_in(c), L.B);
    a.keep = L.keep ? 1 : 0;
    a.h = (T)((c->tf - c->t0) / 2.0);
    a.sgn = c->maximize ? T(-1) : T(1);
    for (int i = 0; i < EMI_MAX_PARAMS; ++i) a.P.p[i] = (T)c->params[i];
}

// Delayed values.  Row k of W(delay) holds the Lagrange basis of the LGL nodes at the node coordinate of max(t_k - delay, t0):
// what PSOPT's get_delayed_state / get_delayed_control hand ePSOPT::dae (reference src/ePSOPT/ePSOPT.cpp:231-248) -- the value
// at t - delay of the polynomial that interpolates the variable's node values ("Legendre" collocation: Lagrange interpolation).
// PSOPT 5.0.0 is not in the reference tree; times before t0 are CLAMPED to t0 here (the history of a delayed variable is its
// initial value), which is an assumption of this build, stated in include/emi355x.h and DESIGN.md section 5.
// Barycentric form with the LGL weights lambda_j ~ (-1)^j sqrt(w_j) (w_j = 2 / (N (N+1) P_N(tau_j)^2)).
void delay_matrix(const std::vector<double>& tau, const std::vector<double>& w, double t0, double tf, double delay, double* W) {
    const int M = (int)tau.size();
    std::vector<double> lam(M);
    for (int j = 0; j < M; ++j) lam[j] = ((j & 1) ? -1.0 : 1.0) * std::sqrt(w[j]);
    const double hh = (tf - t0) / 2.0;
    for (int k = 0; k < M; ++k) {
        double ts = t0 + hh * (tau[k] + 1.0) - delay;
        if (ts < t0) ts = t0;
        const double x = (ts - t0) / hh - 1.0;
        double* row = W + (size_t)k * M;
        int hit = -1;
        for (int j = 0; j < M; ++j)
            if (x == tau[j]) hit = j;
        if (ts <= t0) hit = 0;
        if (hit >= 0) {
            for (int j = 0; j < M; ++j) row[j] = j == hit ? 1.0 : 0.0;
            continue;
        }
        double den = 0.0;
        for (int j = 0; j < M; ++j) {
            row[j] = lam[j] / (x - tau[j]);
            den += row[j];
        }
        for (int j = 0; j < M; ++j) row[j] /= den;
    }
}

// dU_free [B][nc - nch][M] -> *dU_ext [B][nc][M] = [U | x(t - dt) .. x(t - (xh-1) dt) | u(t - dt) .. u(t - uh dt)], the delayed
// rows as products with W on the general MFMA defect kernel (rows += Z . W^T onto zeroed rows)
int extend_controls(emi_ctx_t c, const void* dX, const void* dU_free, const void** dU_ext) {
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "delayed values: f64 contexts only");
    if (c->points_only) return fail(c, EMI_ERR_STATE, "delayed values need a collocation mesh (this context holds a points-only mesh)");
    const int M = c->M, ncf = c->nc - c->nch;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->attr_set) {
        HIP_TRY(c, emi::defect_f64_set_attr());
        c->attr_set = true;
    }
    int st;
    if ((st = ensure_delay_matrices(c))) return st;
    const size_t row = (size_t)M * 8;
    if ((st = ensure(c, c->d_uext, (size_t)c->B * c->nc * row))) return st;
    HIP_TRY(c, hipMemsetAsync(c->d_uext.p, 0, (size_t)c->B * c->nc * row, c->stream));
    HIP_TRY(c, hipMemcpy2DAsync(c->d_uext.p, (size_t)c->nc * row, dU_free, (size_t)ncf * row, (size_t)ncf * row, c->B, hipMemcpyDeviceToDevice, c->stream));
    double* base = (double*)c->d_uext.p + (size_t)ncf * M;
    for (int i = 1; i < c->xh; ++i) {       // x(t - i dt): all states against W[i-1]
        emi::DefectArgs a{(const double*)dX, (const double*)c->d_W.p + (size_t)(i - 1) * M * M, base + (size_t)(i - 1) * c->ns * M,
                          c->B * c->ns, M, c->ns, c->nc};
        HIP_TRY(c, emi::launch_defect_f64(a, c->stream));
    }
    base += (size_t)std::max(c->xh - 1, 0) * c->ns * M;
    for (int i = 1; i <= c->uh; ++i) {      // u(t - i dt): the caller's controls against W[i-1]
        emi::DefectArgs a{(const double*)dU_free, (const double*)c->d_W.p + (size_t)(i - 1) * M * M, base + (size_t)(i - 1) * ncf * M,
                          c->B * ncf, M, ncf, c->nc};
        HIP_TRY(c, emi::launch_defect_f64(a, c->stream));
    }
    *dU_ext = c->d_uext.p;
    return EMI_OK;
}

// The forms a launch of the pass can take.  choose_form is the one place that picks among them; emi_last_path asks it too.
enum class Form {
    PassF64,        // form_pass_f64: emi_pass_f64_kernel, MFMA-role and node-role workgroups in one grid
    TwoKernelF64,   // form_two_kernel_f64: even/odd MFMA defect kernel and node kernel, on one or two streams or on CU-split streams
    PassF32,        // form_pass_f32: emi_pass_f32_kernel, the fp32 pass as one launch
    TwoStreamF32,   // form_two_stream_f32: fp32 MFMA defect kernel beside the full node kernel ("overlap_mode" 2)
    Sequential,     // form_sequential: node kernel, then the general (or skinny) defect kernel, on the context's stream
};
struct FormChoice {
    Form form = Form::Sequential;
    bool small = false;     // Sequential: the skinny streaming defect kernel instead of the MFMA one
    emi::PassPlan plan;     // PassF64 (and TwoKernelF64, which it declined): what plan_pass (emi_pass_plan.hpp) decided
    bool overlapped() const { return form == Form::PassF64 || form == Form::TwoKernelF64; }
};

FormChoice choose_form(emi_ctx_t c, Launch L, unsigned flags) {
    const bool nodes = flags & EMI_EVAL_NODES, defect = flags & EMI_EVAL_DEFECT, jac = !(flags & EMI_EVAL_NOJAC);
    FormChoice ch;
    const emi::PassPolicyIn in = policy_in(c);
    // a handful of instances: the stand-alone MFMA kernels would have a few workgroups to run and a skinny streaming product wins
    // (21 us at B = 1) -- unless the whole pass can go as ONE launch with its K range sliced, which is faster still (13 - 15 us for
    // any batch up to 16 instances: profiles/r03_notes.md section 7)
    ch.small = defect && !c->f32 && L.B > 0 && L.B * c->ns <= in.small_rows && emi::defect_small_supported(L.B * c->ns) &&
               !(nodes && jac && emi::pass_takes_small_batches(in));
    if (nodes && defect && !ch.small && emi::pass_overlapped(in)) {
        ch.plan = emi::plan_pass(in, L.B, jac);
        ch.form = ch.plan.one_launch ? Form::PassF64 : Form::TwoKernelF64;
    } else if (c->f32 && nodes && defect && jac && !c->rtc && c->allow_fused && !in.param_table) {
        if ((c->overlap_mode == 3 || (c->overlap_mode == 0 && c->f32_one_launch)) && emi::pass_f32_supported(c->model, L.B * c->ns, c->M, L.B))
            ch.form = Form::PassF32;
        else if (c->overlap_mode == 2 && emi::defect_f32_mfma_supported(c->M))
            ch.form = Form::TwoStreamF32;
    }
    return ch;
}

// the record of the next profiled launch; the list owns every event from the moment it exists (a record whose events could not
// all be created is completed by the next call)
int next_prof_record(emi_ctx_t c, ProfEvents** out) {
    if (c->prof_used == c->prof.size()) c->prof.emplace_back();
    ProfEvents& pe = c->prof[c->prof_used];
    for (hipEvent_t& e : pe.ev)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    ++c->prof_used;
    *out = &pe;
    return EMI_OK;
}

// One side of a profiling bracket: event `which` of the launch's record on stream s, when the launch is profiled (pe) at one of
// the levels in `levels` (emi_profile_enable: AT1 every bracket, AT2 the defect kernel only, AT3 the node kernel only)
constexpr unsigned AT1 = 1u << 1, AT2 = 1u << 2, AT3 = 1u << 3, AT_ANY = AT1 | AT2 | AT3;
int prof_mark(emi_ctx_t c, ProfEvents* pe, ProfMark which, unsigned levels, hipStream_t s) {
    if (pe && pe->level > 0 && ((levels >> pe->level) & 1u)) HIP_TRY(c, hipEventRecord(pe->ev[which], s));
    return EMI_OK;
}

// ---- what emi_last_defect_kernel reports (the names a rocprofv3 kernel trace shows), each built here and nowhere else
const char* const NAME_PASS_F32 = "emi_pass_f32_kernel (MFMA + node roles, one launch)";
const char* const NAME_RING1_F64 = "emi_symdefect_ring_f64_kernel";
const char* name_defect_f32(emi_ctx_t c, bool mfma) {
    return !mfma ? "emi_defect_f32_kernel" : (c->f32_ring ? "emi_defect_f32_ring_kernel" : "emi_defect_f32_mfma_kernel");
}
const char* name_defect_f64(bool small) { return small ? "emi_defect_small_f64_kernel" : "emi_defect_f64_kernel"; }
std::string name_pass_f64(const emi::SymPlan& plan) {
    return "emi_pass_f64_kernel<SW=" + std::to_string(plan.sw) + "> (MFMA + node roles, one launch" +
           (plan.ks > 1 ? ", " + std::to_string(plan.ks) + " K slices per tile" : "") + ")" +
           (plan.bk == 16 ? " [K tiles of 16]" : "") + (plan.ct == 2 ? " [128-column tiles]" : "") + (plan.hs == 2 ? " [K range in two halves per workgroup]" : "") +
           (plan.dop ? " [De/Do from L2]" : "");
}
std::string name_symdefect(emi_ctx_t c, const emi::SymPlan& plan, bool in_kernel_combine) {
    if (plan.ring1) return c->sym_ct == 1 || c->sym_ct == 2 ? "emi_symdefect_f64_kernel" : NAME_RING1_F64;
    return "emi_symdefect_ring2_f64_kernel<SW=" + std::to_string(plan.sw) + ">" +
           (plan.ks > 1 ? " x" + std::to_string(plan.ks) + (in_kernel_combine ? " K slices (in-kernel combine)" : " K slices + emi_symdefect_combine_kernel") : "");
}

// arguments of the even/odd MFMA role for a launch, unsplit and in the plain tile order (the forms set what their plan changes)
emi::SymDefectArgs sym_defect_args(emi_ctx_t c, Launch L, const PassIO& io) {
    emi::SymDefectArgs sa;
    sa.X = (const double*)io.X;
    sa.U = (const double*)io.U;
    sa.RES = (double*)io.RES;
    sa.node_t = (const double*)c->d_t.p;
    sa.De = (const double*)c->d_De.p;
    sa.Do = (const double*)c->d_Do.p;
    sa.Dfrag = c->has_dfrag ? (const double*)c->d_Dfrag.p : nullptr;
    sa.M = c->M;
    sa.B = L.B;
    sa.nres = nres_of(c);
    sa.h = (c->tf - c->t0) / 2.0;
    sa.order = c->sym_order;
    sa.ablate = c->sym_ablate;
    sa.ksplit = 1;
    sa.slab = nullptr;
    sa.tile_ticket = nullptr;
    sa.cpart = sa.cx = 0;
    sa.mfma_first = 0;
    for (int i = 0; i < EMI_MAX_PARAMS; ++i) sa.P.p[i] = c->params[i];
    return sa;
}

emi::DefectArgsF32 defect_args_f32(emi_ctx_t c, Launch L, const PassIO& io) {
    return emi::DefectArgsF32{(const float*)io.X, (const float*)c->d_D.p, (float*)io.RES, L.B * c->ns, c->M, c->ns, nres_of(c)};
}

// The work table of a launch on the device (emi_pass_work.hpp): the context's copy where the key is cached -- a steady-state call does no
// more than compare keys: no synchronisation, no allocation, no copy -- else built by pass_work_build and uploaded on the context's
// stream, ahead of the launch that reads it.  The slot keeps the host copy, which so outlives the asynchronous copy; a slot that gives
// way is reused only once the stream has drained (launches in flight read its table, the copy reads its host array).
int pass_work_table(emi_ctx_t c, const emi::PassWorkKey& key, const emi::PassWork** out) {
    emi_api::PassWorkCache& pc = c->pass_work;
    for (emi_api::PassWorkCache::Slot& sl : pc.slot)
        if (sl.used && sl.key == key) {
            sl.stamp = ++pc.clock;
            *out = sl.dev.p;
            return EMI_OK;
        }
    emi_api::PassWorkCache::Slot* lru = &pc.slot[0];     // the first free slot, else the least recently used one
    for (emi_api::PassWorkCache::Slot& sl : pc.slot)
        if (lru->used && (!sl.used || sl.stamp < lru->stamp)) lru = &sl;
    std::vector<emi::PassWork> table;
    const char* why = "";
    if (!emi::pass_work_build(key, table, &why))
        return fail(c, EMI_ERR_UNSUPPORTED, "emi_eval: the launch does not fit the work table of the one-launch pass (%s)", why);
    if (lru->used) HIP_TRY(c, hipStreamSynchronize(c->stream));
    lru->used = false;
    HIP_TRY(c, lru->dev.reserve(table.size()));
    lru->host.swap(table);
    HIP_TRY(c, hipMemcpyAsync(lru->dev.p, lru->host.data(), lru->host.size() * sizeof(emi::PassWork), hipMemcpyHostToDevice, c->stream));
    lru->key = key;
    lru->used = true;
    lru->stamp = ++pc.clock;
    ++pc.uploads;
    *out = lru->dev.p;
    return EMI_OK;
}

// The fp64 pass as ONE launch, by the plan the chooser made: MFMA-role and node-role workgroups in one grid, K slices combined
// and COST finished in-kernel by ticket.
int form_pass_f64(emi_ctx_t c, Launch L, const PassIO& io, const emi::PassPlan& pp, ProfEvents* pe) {
    const emi::SymPlan& plan = pp.sym;
    emi::SymDefectArgs sa = sym_defect_args(c, L, io);
    emi::NodeArgs<double> na;
    fill_node_args(c, L, na, io);
    sa.mfma_first = pp.mfma_first;
    sa.cpart = plan.cpart;
    sa.cx = plan.cx;
    if (plan.ks > 1) {
        EMI_TRY(ensure(c, c->d_slab, plan.slab_bytes));
        EMI_TRY(ensure_zeroed(c, c->d_tile_ticket, (size_t)plan.tiles * 4, c->stream));
        sa.ksplit = plan.ks;
        sa.slab = (double*)c->d_slab.p;
        sa.tile_ticket = (unsigned*)c->d_tile_ticket.p;
    }
    EMI_TRY(ensure_zeroed(c, c->d_ticket, (size_t)L.B * 4, c->stream));
    na.cost_ticket = (unsigned*)c->d_ticket.p;
    const emi::PassWorkKey key = emi::pass_work_for(plan, c->ns, L.B, c->M, pp.mfma_first);
    const emi::PassWork* work = nullptr;
    EMI_TRY(pass_work_table(c, key, &work));
    EMI_TRY(prof_mark(c, pe, K0, AT_ANY, c->stream));
    if (c->rtc) HIP_TRY(c, emi::rtc_launch_pass(c->rtc, sa, na, plan.sw, c->stream, key, work));
    else HIP_TRY(c, emi::launch_pass(c->model, sa, na, c->stream, plan, key, work));
    EMI_TRY(prof_mark(c, pe, K1, AT_ANY, c->stream));
    if (pe) pe->level = -1;                 // one bracket: the pass kernel
    c->last_defect_kernel = name_pass_f64(plan);
    return EMI_OK;
}

// the stand-alone even/odd MFMA defect kernel of the two-kernel form on stream s, K slices by "sym_ksplit"
int launch_symdefect_f64(emi_ctx_t c, Launch L, emi::SymDefectArgs& sa, hipStream_t s) {
    if (c->rtc) {
        HIP_TRY(c, emi::rtc_launch_symdefect(c->rtc, sa, s));
        c->last_defect_kernel = NAME_RING1_F64;
        return EMI_OK;
    }
    const emi::SymPlan plan = emi::plan_symdefect(c->ns, L.B, c->M, c->sym_ct, c->sym_ksplit, c->sym_cpart, c->sym_gblk, c->sym_cx);
    if (plan.slab_bytes) EMI_TRY(ensure(c, c->d_slab, plan.slab_bytes));
    sa.ksplit = plan.ring1 ? 1 : plan.ks;
    sa.slab = (double*)c->d_slab.p;
    sa.cpart = plan.cpart;
    sa.cx = plan.cx;
    if (sa.ksplit > 1 && c->sym_combine) {
        EMI_TRY(ensure_zeroed(c, c->d_tile_ticket, (size_t)plan.tiles * 4, s));
        sa.tile_ticket = (unsigned*)c->d_tile_ticket.p;
    }
    const unsigned bit = 1u << c->sym_ct;
    HIP_TRY(c, emi::launch_symdefect(c->model, sa, s, !(c->fused_attr_mask & bit), c->sym_ct, plan));
    c->fused_attr_mask |= bit;
    c->last_defect_kernel = name_symdefect(c, plan, sa.tile_ticket != nullptr);
    return EMI_OK;
}

// The fp64 pass as two kernels that read X, U and write disjoint outputs.  "overlap_mode" 1: back to back on the context's stream;
// otherwise forked onto a second stream (or, with "cu_split", onto two CU-masked streams) and joined again.  The MFMA kernel goes
// first and takes one workgroup per CU (LDS-shaped); the streaming kernel's waves fill the rest of every CU.
int form_two_kernel_f64(emi_ctx_t c, Launch L, const PassIO& io, bool jac, ProfEvents* pe) {
    emi::SymDefectArgs sa = sym_defect_args(c, L, io);
    emi::NodeArgs<double> na;
    fill_node_args(c, L, na, io);
    const bool two = c->overlap_mode != 1;
    const bool split = two && c->cu_split > 0;
    if (two && !split) EMI_TRY(need_stream2(c));
    hipStream_t s1 = split ? c->s_mfma : c->stream;
    hipStream_t s2 = split ? c->s_node : (two ? c->stream2 : c->stream);
    if (two) {
        HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(s2, c->ev_fork, 0));
        if (split) HIP_TRY(c, hipStreamWaitEvent(s1, c->ev_fork, 0));
    }
    EMI_TRY(prof_mark(c, pe, K0, AT1 | AT2, s1));
    EMI_TRY(launch_symdefect_f64(c, L, sa, s1));
    EMI_TRY(prof_mark(c, pe, K1, AT1 | AT2, s1));
    // COST is finished inside the node kernel (last workgroup of an instance, by ticket, in chunk order): one launch
    // and one kernel boundary less at the end of every pass (emi_cost_finish_kernel alone was 5 us)
    if (c->cost_in_kernel) {
        EMI_TRY(ensure_zeroed(c, c->d_ticket, (size_t)L.B * 4, s2));
        na.cost_ticket = (unsigned*)c->d_ticket.p;
    }
    EMI_TRY(prof_mark(c, pe, K2, AT1 | AT3, s2));
    if (c->rtc && jac && na.store_mode == 2 && c->M % 2 == 0) HIP_TRY(c, emi::rtc_launch_nodes_nt(c->rtc, na, s2));
    else if (c->rtc) HIP_TRY(c, emi::rtc_launch_nodes<double>(c->rtc, na, jac, false, s2));
    else HIP_TRY(c, emi::launch_nodes<double>(c->model, na, jac, false, s2));
    EMI_TRY(prof_mark(c, pe, K3, AT1 | AT3, s2));
    if (!c->cost_in_kernel) HIP_TRY(c, emi::launch_cost_finish<double>(na.cost_part, na.cost, L.B, emi::node_chunks(c->M), na.sgn * na.h, s2));
    if (two) {
        HIP_TRY(c, hipEventRecord(c->ev_join, s2));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
        if (split) {
            HIP_TRY(c, hipEventRecord(c->ev_join2, s1));
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join2, 0));
        }
    }
    EMI_TRY(prof_mark(c, pe, E1, AT1, c->stream));
    EMI_TRY(prof_mark(c, pe, E2, AT1, c->stream));
    return EMI_OK;
}

// fp32 contexts (config 5): the pass as ONE launch -- MFMA-role and node-role workgroups in one grid, the defect rows zeroed
// here and completed by float atomics from both roles (emi_defect_f32.hip), COST finished in-kernel by ticket
int form_pass_f32(emi_ctx_t c, Launch L, const PassIO& io, ProfEvents* pe) {
    emi::NodeArgs<float> na;
    fill_node_args(c, L, na, io);
    const size_t rowb = (size_t)c->M * 4;
    HIP_TRY(c, hipMemset2DAsync(io.RES, (size_t)nres_of(c) * rowb, 0, (size_t)c->ns * rowb, L.B, c->stream));
    EMI_TRY(ensure_zeroed(c, c->d_ticket, (size_t)L.B * 4, c->stream));
    na.cost_ticket = (unsigned*)c->d_ticket.p;
    EMI_TRY(prof_mark(c, pe, K0, AT_ANY, c->stream));
    HIP_TRY(c, emi::launch_pass_f32(c->model, defect_args_f32(c, L, io), na, c->pass_order >= 0 ? c->pass_order : 0, c->stream));
    EMI_TRY(prof_mark(c, pe, K1, AT_ANY, c->stream));
    if (pe) { pe->level = -1; pe->fused = true; }
    c->last_defect_kernel = NAME_PASS_F32;
    return EMI_OK;
}

// fp32 contexts (config 5), only when asked for ("overlap_mode" 2): the f32 MFMA defect kernel ACCUMULATES onto
// -h f, so a values-only node kernel writes -h f first and the MFMA kernel follows it on the context's stream, while
// the full node kernel (Jacobian values, cost; no defect rows) runs beside them on the second stream.  Measured at
// B = 256, M = 4096: 1.076 ms against 1.082 ms back to back -- both kernels stretch (MFMA 0.93 -> 1.03 ms, node
// 0.16 -> 0.80 ms), nothing is gained, so the default stays sequential (profiles/r02_notes.md)
int form_two_stream_f32(emi_ctx_t c, Launch L, const PassIO& io, ProfEvents* pe) {
    emi::NodeArgs<float> pre, full;
    PassIO values_only = io;
    values_only.VALS = nullptr;
    fill_node_args(c, L, pre, values_only);
    fill_node_args(c, L, full, io);
    EMI_TRY(ensure(c, c->d_cost_part2, (size_t)L.B * emi::node_chunks(c->M) * 4));
    EMI_TRY(need_stream2(c));
    pre.cost_part = (float*)c->d_cost_part2.p;      // its cost partials go nowhere
    pre.np = 0;                                      // ... and it leaves the path rows to the full kernel
    // (round 4, "f32_ring_wgs" 1: the ring kernel at one workgroup per CU, which costs it nothing, leaves the node kernel's waves
    // room on every SIMD; the node kernel is then released only once the values-only kernel is through, so that it does not fill the
    // chip before the ring kernel's workgroups arrive)
    const bool fork_late = c->f32_ring_wgs == 1;
    if (!fork_late) {
        HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    }
    HIP_TRY(c, emi::launch_nodes<float>(c->model, pre, false, true, c->stream));
    if (fork_late) {
        HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    }
    EMI_TRY(prof_mark(c, pe, K0, AT1 | AT2, c->stream));
    HIP_TRY(c, emi::launch_defect_f32_mfma(defect_args_f32(c, L, io), c->stream, c->f32_ring, c->f32_ring_wgs));
    EMI_TRY(prof_mark(c, pe, K1, AT1 | AT2, c->stream));
    c->last_defect_kernel = name_defect_f32(c, true);
    EMI_TRY(prof_mark(c, pe, K2, AT1 | AT3, c->stream2));
    HIP_TRY(c, emi::launch_nodes<float>(c->model, full, true, false, c->stream2));
    EMI_TRY(prof_mark(c, pe, K3, AT1 | AT3, c->stream2));
    HIP_TRY(c, emi::launch_cost_finish<float>(full.cost_part, full.cost, L.B, emi::node_chunks(c->M), full.sgn * full.h, c->stream2));
    HIP_TRY(c, hipEventRecord(c->ev_join, c->stream2));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    if (pe) pe->fused = true;
    EMI_TRY(prof_mark(c, pe, E1, AT1, c->stream));
    EMI_TRY(prof_mark(c, pe, E2, AT1, c->stream));
    return EMI_OK;
}

// the node kernel by itself (it writes -h f into the defect rows, which the defect kernel then adds D X onto), then COST
template <typename T>
int launch_nodes_alone(emi_ctx_t c, Launch L, const PassIO& io, bool jac) {
    emi::NodeArgs<T> a;
    fill_node_args(c, L, a, io);
    // (a per-instance parameter table: the tabled instantiations, on the rows from the launch's first instance on)
    const T* tab = param_rows<T>(c, L.first);
    if (tab && c->rtc) HIP_TRY(c, emi::rtc_launch_nodes_tab<T>(c->rtc, a, tab, jac, c->stream));
    else if (tab) HIP_TRY(c, emi::launch_nodes_tab<T>(c->model, a, tab, jac, c->stream));
    else if (c->rtc) HIP_TRY(c, emi::rtc_launch_nodes<T>(c->rtc, a, jac, true, c->stream));
    else HIP_TRY(c, emi::launch_nodes<T>(c->model, a, jac, true, c->stream));
    HIP_TRY(c, emi::launch_cost_finish<T>(a.cost_part, a.cost, L.B, emi::node_chunks(c->M), a.sgn * a.h, c->stream));
    return EMI_OK;
}

// The general sequence on the context's stream: node kernel, then defect kernel (either alone where the flags ask for one).
int form_sequential(emi_ctx_t c, Launch L, const PassIO& io, unsigned flags, bool small, ProfEvents* pe) {
    const bool jac = !(flags & EMI_EVAL_NOJAC);
    if (flags & EMI_EVAL_NODES) EMI_TRY(c->f32 ? launch_nodes_alone<float>(c, L, io, jac) : launch_nodes_alone<double>(c, L, io, jac));
    EMI_TRY(prof_mark(c, pe, E1, AT_ANY, c->stream));
    if ((flags & EMI_EVAL_DEFECT) && c->f32) {
        const bool mfma = emi::defect_f32_mfma_supported(c->M) && c->allow_fused && !has_param_table(c);      // (a table: the route of "overlap" 0)
        if (mfma) HIP_TRY(c, emi::launch_defect_f32_mfma(defect_args_f32(c, L, io), c->stream, c->f32_ring, c->f32_ring_wgs));
        else HIP_TRY(c, emi::launch_defect_f32(defect_args_f32(c, L, io), c->stream));
        c->last_defect_kernel = name_defect_f32(c, mfma);
    } else if (flags & EMI_EVAL_DEFECT) {
        emi::DefectArgs a{(const double*)io.X, (const double*)c->d_D.p, (double*)io.RES, L.B * c->ns, c->M, c->ns, nres_of(c)};
        if (small) HIP_TRY(c, emi::launch_defect_small_f64(a, c->stream));
        else HIP_TRY(c, emi::launch_defect_f64(a, c->stream));
        c->last_defect_kernel = name_defect_f64(small);
    }
    EMI_TRY(prof_mark(c, pe, E2, AT1 | AT2, c->stream));
    return EMI_OK;
}

// One launch of the pass: the argument checks, the profiling record, then the form the chooser names.
int eval_launch(emi_ctx_t c, Launch L, const PassIO& io, unsigned flags) {
    const bool nodes = flags & EMI_EVAL_NODES, defect = flags & EMI_EVAL_DEFECT;
    const bool jac = !(flags & EMI_EVAL_NOJAC);
    if (!nodes && !defect) return fail(c, EMI_ERR_ARG, "emi_eval: empty flags");
    if (defect && c->points_only) return fail(c, EMI_ERR_STATE, "emi_eval: the mesh has no differentiation matrix (points-only mesh): EMI_EVAL_NODES only");
    if (!io.X || !io.RES || (nodes && (!io.U || !io.COST || (jac && !io.VALS))))
        return fail(c, EMI_ERR_ARG, "emi_eval: null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->attr_set) {
        HIP_TRY(c, emi::defect_f64_set_attr());
        c->attr_set = true;
    }
    const FormChoice ch = choose_form(c, L, flags);
    ProfEvents* pe = nullptr;
    if (c->profile) {
        EMI_TRY(next_prof_record(c, &pe));
        pe->has_node = nodes;
        pe->has_defect = defect;
        pe->fused = ch.overlapped();
        pe->level = c->profile;
        EMI_TRY(prof_mark(c, pe, E0, pe->fused ? AT1 : AT1 | AT3, c->stream));
    }
    switch (ch.form) {
        case Form::PassF64: return form_pass_f64(c, L, io, ch.plan, pe);
        case Form::TwoKernelF64: return form_two_kernel_f64(c, L, io, jac, pe);
        case Form::PassF32: return form_pass_f32(c, L, io, pe);
        case Form::TwoStreamF32: return form_two_stream_f32(c, L, io, pe);
        case Form::Sequential: break;
    }
    return form_sequential(c, L, io, flags, ch.small, pe);
}

}  // namespace

// W[d] = W((d + 1) dt) of the mesh in force on the device, for the evaluations and for the adjoint pass (whichever comes first)
int emi_api::ensure_delay_matrices(emi_ctx_t c) {
    if (!c->delay_dirty) return EMI_OK;
    const int M = c->M, nd = std::max(c->xh - 1, c->uh);
    std::vector<double> W((size_t)nd * M * M);
    for (int d = 0; d < nd; ++d) delay_matrix(c->h_tau, c->h_w, c->t0, c->tf, (d + 1) * c->delay_dt, W.data() + (size_t)d * M * M);
    EMI_TRY(upload_real(c, c->d_W, W.data(), W.size()));       // (complete on return: W is a local)
    c->delay_dirty = false;
    return EMI_OK;
}

// the second stream of the two-stream forms (node kernel beside the MFMA defect kernel), created on first use
int emi_api::need_stream2(emi_ctx_t c) {
    if (c->stream2) return EMI_OK;
    if (hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess) {
        c->stream2 = nullptr;
        return fail(c, EMI_ERR_HIP, "cannot create the second stream of the two-stream pass");
    }
    return EMI_OK;
}

extern "C" {

int emi_delay_matrix(int M, const double* tau, const double* w, double t0, double tf, double delay, double* W) {
    if (M < 2 || !tau || !w || !W || !(tf > t0) || delay < 0) return EMI_ERR_ARG;
    delay_matrix(std::vector<double>(tau, tau + M), std::vector<double>(w, w + M), t0, tf, delay, W);
    return EMI_OK;
}

int emi_eval_dev(emi_ctx_t c, const void* dX, const void* dU, void* dRES, void* dVALS, void* dCOST,
                 unsigned flags) {
    int st = ready(c);
    if (st) return st;
    if (c->nch > 0 && dX && dU && (st = extend_controls(c, dX, dU, &dU))) return st;     // delayed values appended to the controls
    // large batches go out in pieces only where something forces them (plan_piece); not while per-kernel profiling is on
    int piece = 0;
    const emi::PassPolicyIn in = policy_in(c);
    // (a context with a parameter table: only the pieces the "slice" option asks for -- the sequential route has no operand offsets to
    // keep below 4 GB; each piece reads the table's rows from its first instance on)
    if (!c->profile && (flags & EMI_EVAL_ALL) == EMI_EVAL_ALL && (emi::pass_overlapped(in) || (in.param_table && in.slice > 0)) && dX && dU && dRES &&
        dCOST && (dVALS || (flags & EMI_EVAL_NOJAC)))
        piece = emi::plan_piece(in, c->B);
    const PassIO io{dX, dU, dRES, dVALS, dCOST};
    // EMI_EVAL_KEEP_INVARIANT: honoured where this pass writes the Jacobian into the buffer the record names, under the generation
    // it was made in; any other Jacobian pass writes everything and renews the record -- once ALL its pieces are out.  Passes that
    // write no Jacobian (line searches interleave them) leave the record alone.
    const emi::KeepRecord::Pass kp = c->keep.begin_pass((flags & EMI_EVAL_NODES) && !(flags & EMI_EVAL_NOJAC),
                                                        flags & EMI_EVAL_KEEP_INVARIANT, dVALS);
    flags &= ~(unsigned)EMI_EVAL_KEEP_INVARIANT;
    if (piece <= 0) st = eval_launch(c, Launch{0, c->B, kp.keep}, io, flags);
    for (int first = 0; piece > 0 && first < c->B && st == EMI_OK; first += piece)
        st = eval_launch(c, Launch{first, std::min(piece, c->B - first), kp.keep}, io_at(c, io, first), flags);
    c->keep.end_pass(kp, dVALS, st == EMI_OK);
    return st;
}

int emi_eval_host(emi_ctx_t c, const double* X, const double* U, double* RES, double* VALS,
                  double* COST, unsigned flags) {
    int st = ready(c);
    if (st) return st;
    if (!X || !U) return fail(c, EMI_ERR_ARG, "emi_eval_host: null input");
    const size_t rb = c->f32 ? 4 : 8;
    const size_t nX = (size_t)c->B * c->ns * c->M, nU = (size_t)c->B * (c->nc - c->nch) * c->M;
    const size_t nR = (size_t)c->B * nres_of(c) * c->M, nV = (size_t)c->B * nvals_of(c) * c->M;
    if ((st = upload_real(c, c->s_X, X, nX))) return st;
    if ((st = upload_real(c, c->s_U, U, nU))) return st;
    if ((st = ensure(c, c->s_RES, nR * rb))) return st;
    if ((st = ensure_vals_staging(c, nV * rb))) return st;
    if ((st = ensure(c, c->s_COST, (size_t)c->B * rb))) return st;
    if (!(flags & EMI_EVAL_NODES)) {
        // accumulate-only form: the caller's RES is the starting value
        if (!RES) return fail(c, EMI_ERR_ARG, "emi_eval_host: defect-only needs RES in/out");
        if ((st = upload_real(c, c->s_RES, RES, nR))) return st;
    }
    // (the staging buffer is the context's own: the record knows whether it still holds the invariant rows)
    if ((st = emi_eval_dev(c, c->s_X.p, c->s_U.p, c->s_RES.p, c->s_VALS.p, c->s_COST.p, flags | EMI_EVAL_KEEP_INVARIANT))) return st;
    if ((st = download_real(c, RES, c->s_RES.p, nR))) return st;
    if (!(flags & EMI_EVAL_NOJAC) && (flags & EMI_EVAL_NODES))
        if ((st = download_real(c, VALS, c->s_VALS.p, nV))) return st;
    if (flags & EMI_EVAL_NODES)
        if ((st = download_real(c, COST, c->s_COST.p, c->B))) return st;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}

int emi_hess_dev(emi_ctx_t c, const void* dX, const void* dU, const void* dLamF, const void* dLamC,
                 double sigma, void* dH) {
    int st = ready(c);
    if (st) return st;
    if (!dX || !dU || !dLamF || !dH || (np_total(c) > 0 && !dLamC))
        return fail(c, EMI_ERR_ARG, "emi_hess: null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->nch > 0 && (st = extend_controls(c, dX, dU, &dU))) return st;
    auto fill = [&](auto& a) {
        using T = typename std::remove_reference<decltype(a.h)>::type;
        a.X = (const T*)dX; a.U = (const T*)dU; a.lamF = (const T*)dLamF; a.lamC = (const T*)dLamC;
        a.H = (T*)dH; a.w = (const T*)c->d_w.p; a.node_t = (const T*)c->d_t.p;
        a.path = (const T*)c->d_path.p;
        a.M = c->M; a.B = c->B; a.np = np_total(c); a.path_sets = c->path_sets; a.px = c->px; a.py = c->py;
        a.h = (T)((c->tf - c->t0) / 2.0); a.sgn = c->maximize ? T(-1) : T(1); a.sigma = (T)sigma;
        for (int i = 0; i < EMI_MAX_PARAMS; ++i) a.P.p[i] = (T)c->params[i];
    };
    if (c->f32) {
        emi::HessArgs<float> a;
        fill(a);
        const float* tab = param_rows<float>(c, 0);
        if (tab && c->rtc) HIP_TRY(c, emi::rtc_launch_hess_tab<float>(c->rtc, a, tab, c->stream));
        else if (tab) HIP_TRY(c, emi::launch_hess_tab<float>(c->model, a, tab, c->stream));
        else if (c->rtc) HIP_TRY(c, emi::rtc_launch_hess<float>(c->rtc, a, c->stream));
        else HIP_TRY(c, emi::launch_hess<float>(c->model, a, c->stream));
    } else {
        emi::HessArgs<double> a;
        fill(a);
        const double* tab = param_rows<double>(c, 0);
        if (tab && c->rtc) HIP_TRY(c, emi::rtc_launch_hess_tab<double>(c->rtc, a, tab, c->stream));
        else if (tab) HIP_TRY(c, emi::launch_hess_tab<double>(c->model, a, tab, c->stream));
        else if (c->rtc) HIP_TRY(c, emi::rtc_launch_hess<double>(c->rtc, a, c->stream));
        else HIP_TRY(c, emi::launch_hess<double>(c->model, a, c->stream));
    }
    return EMI_OK;
}

int emi_hess_host(emi_ctx_t c, const double* X, const double* U, const double* LamF,
                  const double* LamC, double sigma, double* H) {
    int st = ready(c);
    if (st) return st;
    if (!X || !U || !LamF || !H || (np_total(c) > 0 && !LamC)) return fail(c, EMI_ERR_ARG, "emi_hess_host: null pointer");
    const size_t rb = c->f32 ? 4 : 8;
    const size_t nX = (size_t)c->B * c->ns * c->M, nU = (size_t)c->B * (c->nc - c->nch) * c->M;
    const size_t nC = (size_t)c->B * np_total(c) * c->M, nH = (size_t)c->B * nhess_of(c) * c->M;
    if ((st = upload_real(c, c->s_X, X, nX))) return st;
    if ((st = upload_real(c, c->s_U, U, nU))) return st;
    if ((st = upload_real(c, c->s_LF, LamF, nX))) return st;
    if (nC && (st = upload_real(c, c->s_LC, LamC, nC))) return st;
    if ((st = ensure(c, c->s_H, nH * rb))) return st;
    if ((st = emi_hess_dev(c, c->s_X.p, c->s_U.p, c->s_LF.p, c->s_LC.p, sigma, c->s_H.p))) return st;
    return download_real(c, H, c->s_H.p, nH);
}

int emi_plan_pass(emi_ctx_t c, int B, emi_pass_plan_t* out) {
    if (!c || !out || B < 1) return EMI_ERR_ARG;
    if (c->M <= 0 || c->model < 0) return fail(c, EMI_ERR_STATE, "emi_plan_pass: mesh and model must be set");
    memset(out, 0, sizeof *out);
    emi::report_pass(policy_in(c), B, out);
    return EMI_OK;
}

int emi_plan_pass_residency(emi_ctx_t c, int B, int* res) {
    if (!c || !res || B < 1) return EMI_ERR_ARG;
    if (c->M <= 0 || c->model < 0) return fail(c, EMI_ERR_STATE, "emi_plan_pass_residency: mesh and model must be set");
    emi_pass_plan_t plan;
    memset(&plan, 0, sizeof plan);
    emi::report_pass(policy_in(c), B, &plan, nullptr, res);
    return EMI_OK;
}

int emi_last_path(emi_ctx_t c, int* fused) {
    if (!c || !fused) return EMI_ERR_ARG;
    *fused = choose_form(c, Launch{0, c->B}, EMI_EVAL_ALL).overlapped() ? 1 : 0;
    return EMI_OK;
}

int emi_debug_pass_roles(int nm, int nn, int order, int* out_role, int out_cap) {
    if (nm < 0 || nn < 0 || nm + nn < 1 || !out_role || out_cap < nm + nn) return EMI_ERR_ARG;
    for (int j = 0; j < nm + nn; ++j) {
        const emi::PassRole r = emi::pass_role_of(j, nm, nn, order);
        out_role[j] = r.mfma ? r.index : -1 - r.index;
    }
    return EMI_OK;
}

int emi_debug_pass_work(int ns, int B, int M, int sw, int ctc, int ksplit, int hs, int sym_cpart, int sym_gblk, int sym_cx, int order, int* out,
                        int out_cap, int* info) {
    if (ns < 1 || B < 1 || M < 128 || M % 128 != 0 || sw < 1 || ns % sw != 0 || (ctc != 1 && ctc != 2) || ksplit < 1 || (hs != 1 && hs != 2) || !info)
        return EMI_ERR_ARG;
    // the tile order as a launch of the pass plans it (plan_tiles): the plan's own K slices, made legal in 8-deep K tiles
    emi::SymPlan p = emi::plan_symdefect(ns, B, M, emi::symdefect_ct_of(ns, sw), emi::legal_ks((M / 2) / 8, ksplit), sym_cpart, sym_gblk, sym_cx, 8, ctc);
    if (p.ring1 || p.sw != sw || p.ct != ctc) return EMI_ERR_UNSUPPORTED;
    p.hs = hs;
    const emi::PassWorkKey key = emi::pass_work_for(p, ns, B, M, order);
    std::vector<emi::PassWork> table;
    if (!emi::pass_work_build(key, table)) return EMI_ERR_UNSUPPORTED;
    const int vals[12] = {(int)key.blocks(), key.nm, key.nn, key.nm8, key.nn8, key.nbx, key.ntiles, key.ngrp, key.cpart, key.cx, key.ks, key.nsg};
    for (int i = 0; i < 12; ++i) info[i] = vals[i];
    for (int g = 0; out && g < (int)key.blocks() && 5 * (g + 1) <= out_cap; ++g) {
        const emi::PassWork e = table[(size_t)emi::pass_work_index(g, key.per_xcd())];
        int* o = out + 5 * (size_t)g;
        o[0] = emi::pass_work_role(e);
        o[1] = o[2] = o[3] = o[4] = 0;
        if (o[0] == emi::PASS_WORK_MFMA) {
            o[1] = emi::pass_work_ntile(e);
            o[2] = emi::pass_work_grp(e);
            o[3] = emi::pass_work_kslice(e);
        } else if (o[0] == emi::PASS_WORK_NODE) {
            o[1] = emi::pass_work_bx(e, 0);
            o[2] = emi::pass_work_b(e, 0);
            o[3] = hs == 2 && emi::pass_work_has_chunk(e, 1) ? emi::pass_work_bx(e, 1) : -1;
            o[4] = hs == 2 && emi::pass_work_has_chunk(e, 1) ? emi::pass_work_b(e, 1) : -1;
        }
    }
    return EMI_OK;
}

int emi_debug_pass_work_uploads(emi_ctx_t c, unsigned long long* uploads, int* tables) {
    if (!c || !uploads) return EMI_ERR_ARG;
    *uploads = c->pass_work.uploads;
    int n = 0;
    for (const emi_api::PassWorkCache::Slot& sl : c->pass_work.slot) n += sl.used ? 1 : 0;
    if (tables) *tables = n;
    return EMI_OK;
}

int emi_debug_tile_order(int ns, int B, int M, int sym_ct, int sym_cpart, int* out_tile, int out_cap, int* ntiles_total, int* cpart,
                         int* cx) {
    return emi_debug_tile_order2(ns, B, M, sym_ct, sym_cpart, 0, 0, out_tile, out_cap, ntiles_total, cpart, cx);
}

int emi_debug_tile_order2(int ns, int B, int M, int sym_ct, int sym_cpart, int sym_gblk, int sym_cx, int* out_tile, int out_cap,
                          int* ntiles_total, int* cpart, int* cx) {
    if (ns < 1 || B < 1 || M < 128 || M % 128 != 0 || !ntiles_total) return EMI_ERR_ARG;
    const emi::SymPlan p = emi::plan_symdefect(ns, B, M, sym_ct, 1, sym_cpart, sym_gblk, sym_cx);
    if (p.ring1 || p.sw < 1) return EMI_ERR_UNSUPPORTED;
    const int ntiles = (M / 2) / 64, ngrp = ((B + 15) / 16) * (ns / p.sw), total = ntiles * ngrp;
    *ntiles_total = total;
    if (cpart) *cpart = p.cpart;
    if (cx) *cx = p.cx;
    for (int t = 0; t < total && t < out_cap && out_tile; ++t) {
        const emi::RingTile rt = emi::ring_tile_of(t, ntiles, ngrp, p.cpart, p.cx, ns / p.sw);
        out_tile[t] = rt.ntile + ntiles * rt.grp;
    }
    return EMI_OK;
}

int emi_debug_operator_fragments(int M, const double* D, double* out) {
    if (M < 128 || M % 128 != 0 || !D || !out) return EMI_ERR_ARG;
    std::vector<double> De, Do;
    if (!even_odd_halves(M, D, De, Do)) return EMI_ERR_UNSUPPORTED;
    emi::operator_fragments(M, De.data(), Do.data(), out);
    return EMI_OK;
}

/* name of the kernel that produced the defect rows in the last emi_eval_dev of this context (for reports) */
const char* emi_last_defect_kernel(emi_ctx_t c) {
    if (!c) return "";
    return c->last_defect_kernel.c_str();
}

}  // extern "C"
