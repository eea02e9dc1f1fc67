// emi_api_pass.hip -- the evaluation pass of the C ABI: the launch policy (plan_pass, plan_piece, choose_form: the ONE definition of
// each), one function per launch form, emi_eval_* / emi_hess_*, the delayed values, and what reports the policy (emi_plan_pass,
// emi_last_path, emi_last_defect_kernel, the emi_debug_* calls).
#include "emi_ctx.hpp"

using namespace emi_api;

namespace {

// the even/odd MFMA defect kernel beside the node kernel: needs an exactly centro-antisymmetric D
bool overlapped_path(emi_ctx_t c) {
    if (c->f32 || !c->allow_fused || !c->symmetric || c->M <= 0 || c->model < 0) return false;
    if (c->model == EMI_MODEL_SOURCE) return emi::rtc_has_symdefect(c->rtc) && c->M % 128 == 0;
    return emi::fused_supported(c->model, c->M, c->sym_ct);
}

// the one-launch pass in its small-batch form (SW = 1, plain stores) is available to this context by the default dispatch
bool pass_takes_small_batches(emi_ctx_t c, int B) {
    if (!overlapped_path(c) || (c->overlap_mode != 0 && c->overlap_mode != 3) || c->M % 128 != 0) return false;
    if (c->rtc) return emi::rtc_pass_supported(c->rtc, B, c->M, 1, 1, 0);
    const emi::SymPlan p = emi::plan_symdefect(c->ns, B, c->M, 7, 1, c->sym_cpart, c->sym_gblk, c->sym_cx);
    return emi::pass_supported(c->model, c->ns, B, c->M, p);
}

// Result-store flavour of the node role for a launch of B instances ("node_store" forces it).  Non-temporal once a pass writes
// about what the Infinity Cache holds (256 MB; RES + VALS above 230 MiB): measured on the one-launch pass, M = 1024
// (profiles/r03_mid_sweep.json): 256 instances (244 MiB) 0.0581 ms against 0.0720 with plain stores, 320: 0.0749 / 0.0973,
// 384: 0.0879 / 0.1050; 224 instances (214 MiB): plain 0.0557 / nt 0.0606, 128: 0.0338 / 0.0354.  (Round 2 switched at 300 MB of
// VALS, i.e. above 384 instances: the 256 .. 384 band ran 20 % slow.)
// Below that: write-through (sc1) stores for the built-in fp64 models since the end of round 4 -- plain stores leave a small pass's results
// dirty in L2 for the write-back at the end of the kernel, write-through streams them out while the kernel runs.  One box, ms per pass plain /
// sc1 (profiles/r04_mid_sweep_sc1_stores.jsonl): 1 instance 0.0125 / 0.0105, 16: 0.0149 / 0.0128, 32: 0.0176 / 0.0172, 64: 0.0209 / 0.0215,
// 80: 0.0233 / 0.0221, 112: 0.0290 / 0.0283, 128: 0.0291 / 0.0286, 144: 0.0305 / 0.0296, 192: 0.0434 / 0.0430, 224: 0.0532 / 0.0505.
// (Run-time compiled models hold a plain and a non-temporal instantiation only.)
int store_mode_for(emi_ctx_t c, int B) {
    if (c->node_store >= 0) return c->node_store;
    if ((size_t)B * (nvals_of(c) + nres_of(c)) * c->M * (c->f32 ? 4 : 8) > ((size_t)230 << 20)) return 2;
    // (17 .. 32 tiles -- 33 .. 64 instances at 1024 nodes, the two-slice band -- are the one place where plain stores stay ahead: 48 instances
    // 0.0197 / 0.0203, 64: 0.0209 / 0.0215)
    const int tiles16 = ((B + 15) / 16) * (c->M / 128);
    if (tiles16 > 16 && tiles16 <= 32) return 0;
    return (!c->rtc && !c->f32) ? 1 : 0;
}

// Everything the default dispatch decides about ONE launch of the evaluation pass as emi_pass_f64_kernel, in one place:
// plan_pass() is what choose_form / form_pass_f64 launch by and what emi_plan_pass reports (tests and tools read the policy from the
// library instead of restating it).
struct PassPlan {
    bool one_launch = false;    // the pass goes out as ONE launch (MFMA-role + node-role workgroups)
    emi::SymPlan sym;           // MFMA role: states per workgroup, K slices per tile, ring stages, tile order
    int tiles16 = 0;            // 16-instance x 128-node tiles of the launch (what the thresholds below are written in)
    int store_mode = 0;         // node role: 0 plain, 1 sc1, 2 non-temporal, 3 nt sc1
    int mfma_first = 0;         // block order (pass_role_of): 1 MFMA workgroups first, 0 evenly interleaved, >= 100: at that % of the even density
};

// The pass as ONE launch: MFMA-role and node-role workgroups in one grid, COST finished in-kernel -- since round 3 at EVERY
// batch size (round 2: two streams between 384 and 767 instances, which ran 20 - 25 % under the rest).  One box, interleaved
// rounds, M = 1024, ms per pass, best one-launch form against the round-2 choice (profiles/r03_mid_sweep.json): 256: 0.0581 /
// 0.0731, 320: 0.0749 / 0.0927, 384: 0.0879 / 0.1177 (two streams), 448: 0.1035 / 0.1038, 512: 0.1188 / 0.1162, 576: 0.1332 /
// 0.1777, 640: 0.146 / 0.155, 704: 0.160 / 0.181.
//   * SW (states per MFMA workgroup): 1 below 128 sixteen-instance x 128-node tiles (more workgroups than CUs), else 2;
//   * K slices per tile ("sym_ksplit"; partial sums combined in-kernel by ticket, in slice order).  By itself only where the MFMA
//     role has fewer workgroups than the chip has places for them, i.e. where a pass waits for one 64-tile dependency chain per
//     workgroup: 4 slices while that keeps the role within 256 workgroups, 2 within 512.  One box, M = 1024, ms per pass
//     unsplit / 2 / 4 slices (tools/mid_sweep.py, profiles/r03_notes.md section 7): B = 8: 0.0204 / 0.0148 / 0.0140,
//     16: 0.0235 / 0.0179 / 0.0155, 32: 0.0242 / 0.0190 / 0.0192, 64: 0.0257 / 0.0218 / 0.0261, 80: 0.0263 / 0.0249 / 0.0312,
//     96: 0.0288 / 0.0290 / 0.0407, 128: 0.0333 / 0.0387 / 0.0496 (from ~500 workgroups the split loses: three and more MFMA
//     waves per SIMD share the matrix pipe and the node role starts behind them);
//   * block order (pass_role_of): MFMA workgroups first below 208 tiles (their 64-tile dependency chains start at once, the
//     streaming workgroups fill in behind; since the end of round 4 only below 144 tiles: 1.5 x the even density from there, see
//     deep_band below), at 1.25 x the even density up to 384 tiles, at 1.1 x up to 768, evenly interleaved
//     from there (B >= 768, where "first" would hold the node role back: 0.288 against 0.222 at 1024).  (Round 2 measured
//     "first" against "interleaved" WITH PLAIN STORES at 256 instances and found interleaved ahead, 0.0727 / 0.0748; with
//     non-temporal stores "first" wins up to 448 instances: 256: 0.0581 against 0.0756 interleaved.  End of round 3, one box,
//     e9 node-evals/s at first / 1.25 x / 1.5 x / even: 448 instances 4.21 / 4.41 / 4.22 / 4.31, 512: 3.60 / 4.32 / 4.38 / 4.22,
//     640: 3.76 / 4.48 / 4.37 / 4.37, 704: 3.89 / 4.63 / 4.45 / 4.50; ms per pass at even / 1.1 x / 1.25 x: 768: 0.1747 /
//     0.1696 / 0.1760, 896: 0.1964 / 0.1959 / 0.2022, 1024: 0.2230 / 0.2200 / 0.2304, 1536: 0.3215 / 0.3219 / 0.3411,
//     2048: 0.4239 / 0.4227 / 0.4415);
//   * tile order: grouped (an XCD's MFMA tiles and node workgroups walk the same instance groups together) for launches of more
//     than 2048 instances in whole super-blocks, else column partitions by mesh size (plan_symdefect);
//   * stores: store_mode_for (non-temporal from about 256 instances).
// Every choice can be forced through emi_set_option (sym_ct, sym_ksplit, sym_cpart, sym_gblk, sym_cx, sym_nst, pass_order,
// node_store); a run-time compiled model holds two instantiations of the pass kernel -- SW = 1 with plain stores (small batches)
// and SW = 2 (1 for an odd number of states) with non-temporal stores (large ones) -- and is planned within those.
PassPlan plan_pass(emi_ctx_t c, int B, bool jac) {
    PassPlan p;
    p.tiles16 = ((B + 15) / 16) * (c->M / 128);
    p.store_mode = store_mode_for(c, B);
    const bool auto_mode = c->overlap_mode == 0;
    if (!((c->overlap_mode == 3 || auto_mode) && jac) || c->M % 128 != 0) return p;
    const bool auto_ct = auto_mode && (c->sym_ct == 0 || c->sym_ct == 4);
    const int gblk = (c->sym_gblk == 0 && c->sym_cpart == 0 && B > 2048 && B % 256 == 0) ? 2 : c->sym_gblk;
    const int gblk_first = (auto_ct || c->rtc) ? gblk : c->sym_gblk;
    int ct = c->sym_ct;                                  // 5 / 6 / 7 / 8 = SW NS / 2 / 1 / 3 (plan_symdefect)
    // Round 4: between 64 and 127 tiles (128 .. 255 instances at 1024 nodes: the shard of config 4) two states per workgroup with K
    // tiles of 16 -- half the barriers and counted waits of the MFMA role's dependency chain, which is what such a pass waits for.
    // One box, ms per pass, SW = 1 / 8-deep (the round-3 choice) against SW = 2 / 16-deep (profiles/r04_mid_sweep.jsonl): 128 instances
    // 0.0320 / 0.0300, 192: 0.0482 / 0.0442; at 64 instances the sliced SW = 1 form stays ahead (0.0210 / 0.0269), from 256 the 8-deep
    // SW = 2 form (0.0548 / 0.0617).
    // End of round 4 (profiles/r04_mid_sweep_small_72_120.jsonl, one box, ms per pass): the rule "2 K slices while the MFMA role stays within
    // 512 workgroups" held up to 80 instances, where the finer sweep found 0.0324 ms against 0.0208 at 64 and 0.0277 at 96.  SW = 1 with 2
    // slices / SW = 1 unsplit 8-deep / SW = 1 unsplit 16-deep / SW = 2 unsplit 16-deep: 72 instances 0.0323 / 0.0246 / 0.0231 / 0.0261, 80:
    // 0.0324 / 0.0248 / 0.0234 / 0.0267, 96: 0.0363 / 0.0278 / 0.0266 / 0.0278, 112: 0.0411 / 0.0338 / 0.0335 / 0.0291.  So: above 32 tiles
    // (64 instances) no slices any more; 33 .. 48 tiles one state per workgroup with 16-deep K tiles (deep_small), from 49 tiles two states
    // (deep_mid, which began at 64 tiles).
    const bool deep_base = auto_ct && !c->rtc && c->sym_bk == 0 && c->sym_ksplit == 0 && c->sym_nst == 3;
    // (both for an even number of states above two, where they were measured: the 6-state quadrotor)
    const bool deep_mid = deep_base && c->ns % 2 == 0 && c->ns > 2 && p.tiles16 >= 49 && p.tiles16 < 128;
    const bool deep_small = deep_base && c->ns % 2 == 0 && c->ns > 2 && p.tiles16 >= 33 && p.tiles16 < 49;
    if (c->rtc) ct = (p.store_mode == 2 && emi::rtc_pass_sw_large(c->rtc) == 2) ? 6 : 7;
    else if (auto_ct) ct = (p.tiles16 < 128 && !deep_mid) ? 7 : 6;
    emi::SymPlan plan = emi::plan_symdefect(c->ns, B, c->M, ct, 1, c->sym_cpart, gblk_first, c->sym_cx);
    if (plan.ring1) plan = emi::plan_symdefect(c->ns, B, c->M, 5, 1, c->sym_cpart, c->sym_gblk, c->sym_cx);
    int ks_want = c->sym_ksplit;
    if (ks_want == 0 && auto_ct && !deep_mid && !deep_small) ks_want = plan.tiles * 4 <= 256 ? 4 : (plan.tiles * 2 <= 512 ? 2 : 1);
    if (ks_want > 1) {
        const int ct_now = plan.sw == c->ns ? 5 : (plan.sw == 2 ? 6 : (plan.sw == 3 ? 8 : 7));
        plan = emi::plan_symdefect(c->ns, B, c->M, ct_now, ks_want, c->sym_cpart, c->rtc ? gblk : c->sym_gblk, c->sym_cx);
    } else {
        plan.ks = 1;
    }
    plan.nst = c->rtc ? 3 : c->sym_nst;
    // K tiles of 16 (built-in models, SW 1 or 2, three stages, unsplit): "sym_bk" 16 forces them
    // ... and between 208 and 767 tiles (416 .. 1535 instances, SW = 2 at 1.25 x / 1.1 x the even MFMA density): one box, ms per pass 8- /
    // 16-deep, 448 instances 0.1112 / 0.1018, 512: 0.1226 / 0.1151, 576: 0.1351 / 0.1277, 640: 0.1492 / 0.1431, 768: 0.1675 / 0.1649,
    // 896: 0.1921 / 0.1896, 1024: 0.2164 / 0.2143; not at 256 .. 384 instances (MFMA workgroups first: 320: 0.0752 / 0.0924) nor from 2048
    // (0.4147 / 0.4205; 4096 in the grouped order 1.081 / 1.175)
    // (up to 1024 tiles -- 2048 instances -- since the end of round 4: with the pass kernel's register allocation stated, 8- / 16-deep at 1536
    // instances 0.3204 / 0.3117, 1792: 0.3725 / 0.3611, 2048: 0.4441 / 0.4322, profiles/r04_mid_sweep_1280_2048.jsonl)
    const bool deep_large = auto_ct && !c->rtc && c->sym_bk == 0 && c->sym_nst == 3 && c->pass_order < 0 && p.tiles16 >= 208 && p.tiles16 <= 1024;
    // ... and between 144 and 207 tiles (288 .. 415 instances) TOGETHER with the MFMA workgroups at 1.5 x the even density instead of all
    // of them first: from ~300 instances the role's 3 x tiles workgroups no longer fit beside the node role (64 places per XCD), which then
    // starts a workgroup generation late.  End of round 4, one box, ms per pass, first + 8-deep (the choice until then) / 1.5 x + 16-deep:
    // 288 instances 0.0730 / 0.0699, 320: 0.0859 / 0.0754, 352: 0.1004 / 0.0820, 384: 0.1022 / 0.0875; 272: 0.0644 / 0.0698 (stays),
    // 416 (1.25 x + 16-deep already): 0.0946 / 0.0951 (profiles/r04_mid_sweep_band_288_416.jsonl)
    const bool deep_band = auto_ct && !c->rtc && c->sym_bk == 0 && c->sym_nst == 3 && c->pass_order < 0 && c->ns % 2 == 0 && c->ns > 2 &&
                           p.tiles16 >= 144 && p.tiles16 < 208;
    const int bk_want = c->sym_bk ? c->sym_bk : ((deep_mid || deep_small || deep_large || deep_band) ? 16 : 8);
    if (bk_want == 16 && !c->rtc && plan.ks == 1 && (plan.sw == 1 || plan.sw == 2) && plan.nst == 3) plan.bk = 16;
    // two column sub-tiles per MFMA workgroup ("sym_ctc" 2; built-in models, SW = 2, unsplit, three stages): the plan is made again with
    // the wider tiles (tile counts and tile order change with the column width)
    // By itself for launches of more than 2048 instances (the grouped tile order; inputs beyond the Infinity Cache, where every operand
    // read is an HBM read): one box, ms per pass one / two sub-tiles, 4096 instances 1.181 / 1.101, 16384: 4.407 / 4.044 (3.81e9 -> 4.15e9
    // node-evals/s) with column blocks of one 128-column tile; at 2048 instances 0.4736 / 0.4636, at 1024 and below the narrow form is ahead
    // (0.2222 / 0.2425: the wide workgroups need 60 KB of LDS and 160 registers) (profiles/r04_mid_sweep.jsonl)
    const bool wide_large = auto_ct && c->sym_ctc == 0 && B > 2048 && B % 256 == 0 && c->sym_cpart == 0;
    const int ctc_want = c->sym_ctc ? c->sym_ctc : (wide_large ? 2 : 1);
    if (ctc_want == 2 && !c->rtc && plan.ks == 1 && plan.sw == 2 && plan.nst == 3 && c->M % 256 == 0) {
        const int bk_keep = plan.bk;
        plan = emi::plan_symdefect(c->ns, B, c->M, 6, 1, c->sym_cpart, gblk_first, (wide_large && c->sym_cx == 0) ? 1 : c->sym_cx, bk_keep, 2);
        plan.ks = 1;
        plan.nst = 3;
        plan.bk = bk_keep;
    }
    // the K range in two halves inside the workgroup ("sym_hs" 2; built-in models, SW 1 or 2, unsplit, one sub-tile, three stages)
    const int hs_want = c->sym_hs ? c->sym_hs : 1;
    if (hs_want == 2 && !c->rtc && plan.ks == 1 && plan.ct == 1 && (plan.sw == 1 || plan.sw == 2) && plan.nst == 3 &&
        ((c->M / 2) / plan.bk) % 4 == 0)
        plan.hs = 2;
    // De / Do fragments straight from L2 into the MFMA waves' registers instead of through the operand ring ("sym_dop" 2; built-in models,
    // SW 1 or 2 of more states, 16-deep K tiles, unsplit, one sub-tile, three stages; the context holds the fragment-order copy)
    // By itself from 216 tiles (432 instances) through the range of deep_large.  One box, M = 1024, ms per pass through the ring / straight
    // from L2 (tools/mid_sweep.py dop1,dop2; profiles/r06_mid_sweep_dop.jsonl): 432 instances 0.0903 / 0.0865, 512: 0.1002 / 0.0975, 768: 0.1446 /
    // 0.1412, 1024: 0.1879 / 0.1836, 1536: 0.2790 / 0.2735, 2048: 0.3771 / 0.3671.  Below that neither form is ahead: the pass time moves with how
    // the workgroups of the two roles fill the chip, not with the K loop (128: 0.0261 / 0.0262, 176: 0.0412 / 0.0392, 224: 0.0425 / 0.0434, 288:
    // 0.0614 / 0.0631, 352: 0.0774 / 0.0714, 416: 0.0824 / 0.0835; SW = 1: 80 instances 0.0192 / 0.0208, 96: 0.0246 / 0.0240), so those stay.
    const int dop_want = c->sym_dop ? c->sym_dop : ((deep_large && p.tiles16 >= 216) ? 2 : 1);
    if (dop_want == 2 && !c->rtc && c->has_dfrag && plan.bk == 16 && plan.ks == 1 && plan.ct == 1 && plan.hs == 1 && plan.nst == 3 &&
        plan.sw != c->ns && (plan.sw == 1 || plan.sw == 2))
        plan.dop = true;
    p.sym = plan;
    p.mfma_first = c->pass_order >= 0 ? c->pass_order
                                      : (deep_band ? 150 : (p.tiles16 < 208 ? 1 : (p.tiles16 < 384 ? 125 : (p.tiles16 < 768 ? 110 : 0))));
    p.one_launch = c->rtc ? emi::rtc_pass_supported(c->rtc, B, c->M, plan.sw, plan.ks, p.store_mode)
                          : emi::pass_supported(c->model, c->ns, B, c->M, plan);
    return p;
}

// Large batches: the instances one launch of emi_eval_dev's default dispatch takes (0: the whole batch in one).  Round 2 cut
// everything above 2048 instances into 1024-instance launches (the two-stream form drifted apart on long launches); with the pass
// as ONE launch that buys nothing, and inputs of more than ~256 MB no longer stay in the Infinity Cache from one pass to the next,
// which is what really slows a large batch (B = 16384: 3.47e9 node-evals/s sliced or not, profiles/r03_notes.md).  Now: one launch
// over the whole batch in the GROUPED tile order: 4.10e9 /s at 16384 instances, 4.13e9 at 4096.  Pieces remain only where
// something forces them: the "slice" option (> 0: pieces of that many instances once B > 2 slice), the 32-bit operand offsets of
// the MFMA role (X of a launch below 4 GB), and a remainder that is not a multiple of 256 instances (the grouped order wants whole
// super-blocks on every XCD) as a second launch.
int plan_piece(emi_ctx_t c, int B) {
    const long long cap = ((0xFFFFFFFFLL / ((long long)c->ns * c->M * 8)) / 256) * 256;     // instances whose X stays below 4 GB
    int piece = 0;
    if (c->slice > 0) { if (B > 2 * c->slice) piece = c->slice; }
    else if (B > 2048) piece = (int)std::min<long long>(cap > 0 ? cap : 256, B - B % 256);
    return piece >= B ? 0 : piece;
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
    a.store_mode = store_mode_for(c, L.B);
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
    PassPlan plan;          // PassF64 (and TwoKernelF64, which it declined): what plan_pass decided
    bool overlapped() const { return form == Form::PassF64 || form == Form::TwoKernelF64; }
};

FormChoice choose_form(emi_ctx_t c, Launch L, unsigned flags) {
    const bool nodes = flags & EMI_EVAL_NODES, defect = flags & EMI_EVAL_DEFECT, jac = !(flags & EMI_EVAL_NOJAC);
    FormChoice ch;
    // a handful of instances: the stand-alone MFMA kernels would have a few workgroups to run and a skinny streaming product wins
    // (21 us at B = 1) -- unless the whole pass can go as ONE launch with its K range sliced, which is faster still (13 - 15 us for
    // any batch up to 16 instances: profiles/r03_notes.md section 7)
    ch.small = defect && !c->f32 && L.B > 0 && L.B * c->ns <= c->small_rows && emi::defect_small_supported(L.B * c->ns) &&
               !(nodes && jac && pass_takes_small_batches(c, L.B));
    if (nodes && defect && !ch.small && overlapped_path(c)) {
        ch.plan = plan_pass(c, L.B, jac);
        ch.form = ch.plan.one_launch ? Form::PassF64 : Form::TwoKernelF64;
    } else if (c->f32 && nodes && defect && jac && !c->rtc && c->allow_fused) {
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

// The fp64 pass as ONE launch, by the plan the chooser made: MFMA-role and node-role workgroups in one grid, K slices combined
// and COST finished in-kernel by ticket.
int form_pass_f64(emi_ctx_t c, Launch L, const PassIO& io, const PassPlan& pp, ProfEvents* pe) {
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
    EMI_TRY(prof_mark(c, pe, K0, AT_ANY, c->stream));
    if (c->rtc) HIP_TRY(c, emi::rtc_launch_pass(c->rtc, sa, na, plan.sw, c->stream));
    else HIP_TRY(c, emi::launch_pass(c->model, sa, na, c->stream, plan));
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
    if (c->rtc) HIP_TRY(c, emi::rtc_launch_nodes<T>(c->rtc, a, jac, true, c->stream));
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
        const bool mfma = emi::defect_f32_mfma_supported(c->M) && c->allow_fused;
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
    if (!c->profile && !c->f32 && (flags & EMI_EVAL_ALL) == EMI_EVAL_ALL && overlapped_path(c) && dX && dU && dRES && dCOST &&
        (dVALS || (flags & EMI_EVAL_NOJAC)))
        piece = plan_piece(c, c->B);
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
        if (c->rtc) HIP_TRY(c, emi::rtc_launch_hess<float>(c->rtc, a, c->stream));
        else HIP_TRY(c, emi::launch_hess<float>(c->model, a, c->stream));
    } else {
        emi::HessArgs<double> a;
        fill(a);
        if (c->rtc) HIP_TRY(c, emi::rtc_launch_hess<double>(c->rtc, a, c->stream));
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
    const int piece = (!c->f32 && overlapped_path(c)) ? plan_piece(c, B) : 0;
    const int first = piece > 0 ? piece : B;    // instances of the first launch
    out->piece = piece;
    out->tail = piece > 0 ? B % piece : 0;
    if (!c->f32 && overlapped_path(c)) {
        const PassPlan p = plan_pass(c, first, true);
        out->one_launch = p.one_launch ? 1 : 0;
        out->sw = p.sym.sw;
        out->ksplit = p.sym.ks;
        out->ring_stages = p.sym.nst;
        out->k_tile = p.sym.bk;
        out->column_tiles = p.sym.ct;
        out->k_halves = p.sym.hs;
        out->cpart = p.sym.cpart;
        out->cx = p.sym.cx;
        out->mfma_workgroups = p.sym.tiles * p.sym.ks;
        out->store_mode = p.store_mode;
        out->block_order = p.mfma_first;
        out->tiles16 = p.tiles16;
    }
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
