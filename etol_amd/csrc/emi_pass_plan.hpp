// emi_pass_plan.hpp -- the launch policy of the fp64 evaluation pass, host-only (no HIP header, no context: it compiles with a plain
// C++ compiler and is walked without a device by tests/harness/pass_plan_main.cpp, `make check-pass-plan`).  It holds
//   * the FORM TABLE (EMI_PASS_FORMS): the instantiations of emi_pass_f64_kernel the library holds for a built-in model, written once --
//     launch_pass_planned (emi_symdefect.hip) instantiates and dispatches by walking the same list -- and the two a run-time compiled
//     model program holds (EMI_PASS_FORMS_RTC, emi_rtc.hip);
//   * resolve_form: the one place where a wanted feature is snapped to a form that exists;
//   * PassPolicyIn: what the policy reads (emi_api_pass.hip fills it from the context);
//   * the BAND TABLE (PASS_BANDS): the defaults by launch size, each row with the measurements behind it;
//   * plan_symdefect, store_mode_for, plan_pass, plan_piece, report_pass as pure functions of PassPolicyIn and the batch;
//   * pass_work_for: the key of the work table of a planned launch (the table itself: emi_pass_work.hpp).
// A new kernel form is one row of EMI_PASS_FORMS (plus its precondition in form_fits, if it has one) and one row of PASS_BANDS.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <climits>

#include "emi355x.h"
#include "emi_pass_work.hpp"

namespace emi {

constexpr int PASS_TI = 16;     // instances per MFMA tile (FUSED_TI of emi_args.hpp; emi_kernels.hpp asserts that they agree)

// which even/odd MFMA defect kernel a launch uses (plan_symdefect; the one-launch pass: plan_pass)
struct SymPlan {
    bool ring1 = false;       // the one-workgroup-per-CU ring kernel / register-staged forms (sym_ct 1..3)
    int sw = 0;               // state-split ring: states per workgroup
    int ks = 1;               // ... and K slices per tile (> 1: partial sums through a slab, combined in-kernel by ticket or by a second launch)
    int nst = 3;              // ring stages of the one-launch pass (3 or 4: K tiles in flight = nst - 1)
    int bk = 8;               // depth of a K tile of the one-launch pass (8, or 16: SW 1 / 2 with three stages)
    int hs = 1;               // 2: the K range of a tile in two halves inside a 512-thread workgroup, combined through LDS (SW 1 / 2, unsplit, one sub-tile)
    int ct = 1;               // 64-column sub-tiles per MFMA workgroup of the one-launch pass (2: SW = 2, unsplit, M % 256 == 0)
    bool dop = false;         // one-launch pass: the MFMA role's De / Do fragments straight from L2, not through the ring (SW 1 / 2, bk 16, unsplit,
                              // one sub-tile, three stages; needs SymDefectArgs::Dfrag)
    int res = 2;              // one-launch pass: resident workgroups per CU the launch states (3: the direct-operator forms only, "sym_res")
    size_t slab_bytes = 0;
    int cpart = 0, cx = 0;    // tile order (SymDefectArgs::cpart, cx): 0 = plain, > 0 column partitions, < 0 grouped (-G)
    int tiles = 0;            // tiles of the launch (instance groups x column tiles x state groups): tickets of an in-kernel combine
};

// the even/odd MFMA kernels exist for meshes of whole 128-node tiles (the register-staged wide form, sym_ct 2: 256-node tiles)
inline bool symdefect_shape_ok(int M, int ct) {
    if (ct == 0 || (ct >= 4 && ct <= 8)) return M >= 128 && M % 128 == 0;
    const int w = ct == 2 ? 2 : 1;     // ct == 3 is the ring variant of the 64-column tiling
    return ct >= 1 && ct <= 3 && M >= 128 * w && M % (128 * w) == 0;
}

// K slices of a tile of nkt K tiles as the K loop can take them: they divide the K tiles, leave at least two per slice, and an even number
inline int legal_ks(int nkt, int ks) {
    while (ks > 1 && (nkt % ks != 0 || nkt / ks < 2 || (nkt / ks) % 2 != 0)) ks >>= 1;
    return ks < 1 ? 1 : ks;
}

// States per workgroup of the state-split ring for the variant code ct ("sym_ct"); 0: the one-workgroup-per-CU ring kernel instead.
// The variant for a batch (ct 0 / 4), by what was measured on MI355X with the node kernel running beside it
// (profiles/r02_pass_variants.json; 6-state model, 1024 nodes; "tiles" = 16-instance x 64-half-index tiles):
//   >= 448 tiles (B = 1024: 512): SW = 2 -- 78 registers and 36 KB of LDS per workgroup leave the streaming
//      kernel's waves the room they need on every CU (pass 0.24-0.25 ms against 0.26-0.27 with 60 KB workgroup pairs);
//   320 .. 447 tiles (B = 768): SW = NS, all workgroups resident at once, two per CU (0.172 ms against 0.198);
//   192 .. 319 tiles (B = 512): the one-workgroup-per-CU ring kernel, whose grid is then a single round;
//   fewer (the shard of config 4: 128 instances = 64 tiles for 256 CUs): SW = 1 (<= 96 tiles) or 2, i.e. more workgroups
//      than CUs (0.055 ms at 128 instances; SW = NS with 4 K slices, the choice before the K loop was software-pipelined: 0.089).
// ct 5 / 6 / 7 / 8 force SW = NS / 2 / 1 / 3 (1 where that does not divide the states).
inline int symdefect_sw(int ns, int tiles, int ct) {
    if (ct == 0 || ct == 4) {
        if (tiles >= 448) return (ns % 2 == 0 && ns > 2) ? 2 : ns;
        if (tiles >= 320) return ns;
        if (tiles >= 192) return 0;
        return (tiles <= 96 || ns % 2 != 0 || ns <= 2) ? 1 : 2;
    }
    if (ct < 5 || ct > 8) return 0;
    const int sw = ct == 5 ? ns : (ct == 6 ? 2 : (ct == 8 ? 3 : 1));
    return ns % sw != 0 ? 1 : sw;
}
// ... and the code that forces a given SW
inline int symdefect_ct_of(int ns, int sw) { return sw == ns ? 5 : (sw == 2 ? 6 : (sw == 3 ? 8 : 7)); }

// Tiles, K slices and tile order of a launch of the state-split ring (two-kernel form and one-launch pass); ksplit_opt > 0 forces the
// slice count, ct_cols 2 asks for 128-column tiles (one-launch pass, SW = 2, unsplit).
inline SymPlan plan_symdefect(int ns, int B, int M, int ct, int ksplit_opt, int cpart_opt = 0, int gblk_opt = 0, int cx_opt = 0, int bk_opt = 8,
                              int ct_cols = 1) {
    SymPlan p;
    p.bk = bk_opt == 16 ? 16 : 8;
    const int mtiles = (B + PASS_TI - 1) / PASS_TI;
    const int tiles = mtiles * ((M / 2) / 64);    // in 64-column tiles: what the thresholds of symdefect_sw are written in
    p.sw = symdefect_sw(ns, tiles, ct);
    if (p.sw == 0) {
        p.ring1 = true;
        return p;
    }
    if (ksplit_opt > 0) p.ks = legal_ks((M / 2) / p.bk, ksplit_opt);
    p.ct = (ct_cols == 2 && p.sw == 2 && p.ks == 1 && M % 256 == 0) ? 2 : 1;      // column sub-tiles per workgroup (one-launch pass, SW = 2, unsplit)
    p.tiles = (tiles / p.ct) * (ns / p.sw);
    {   // tile order: the share of De / Do an XCD works on should stay in its 4 MB L2 beside everything else (<= 2 MB)
        const int ntiles = (M / 2) / (64 * p.ct), ngrp = mtiles * (ns / p.sw);
        const int target_cols = std::max(1, 4096 / M / p.ct);   // column tiles whose two panels (512 M bytes each per 64 columns) make 2 MB
        auto valid = [&](int cp) { return cp >= 1 && cp <= 8 && ntiles % cp == 0 && ngrp % (8 / cp) == 0 && (ngrp * ntiles) % 8 == 0; };
        int cp = 0;
        if (cpart_opt > 0) cp = valid(cpart_opt) ? cpart_opt : 0;
        else if (cpart_opt == 0 && tiles >= 192)    // (small batches: an XCD's few tiles do not walk the panels often enough to matter)
            for (int c = 1; c <= 8 && !cp; c *= 2)
                if (valid(c) && (ntiles / c <= target_cols || c == 8 || !valid(2 * c))) cp = c;
        if (gblk_opt > 0 && mtiles % (8 * gblk_opt) == 0 && (ngrp * ntiles) % 8 == 0) {
            // grouped order ("sym_gblk"): super-blocks of gblk instance groups per XCD, column blocks of cx tiles
            int cxg = cx_opt > 0 ? cx_opt : 2;
            while (cxg > 1 && ntiles % cxg != 0) --cxg;
            p.cpart = -gblk_opt;
            p.cx = cxg;
        } else if (cp > 0) {
            p.cpart = cp;
            p.cx = 1;                                            // largest divisor of the partition's column count within the target
            for (int d = 1; d <= std::min(ntiles / cp, target_cols); ++d)
                if ((ntiles / cp) % d == 0) p.cx = d;
            if (cp == 1 && p.cx == ntiles) p.cpart = p.cx = 0;   // that is the plain order
        }
    }
    if (p.ks > 1) p.slab_bytes = (size_t)p.tiles * p.ks * (2 * p.sw * 4) * 256 * sizeof(double);
    return p;
}

// ---- the form table ---------------------------------------------------------------------------------------------------------------
// SW class of a row: all the states of the model, or 2 (an even number of states above 2), 3 (above 3, divisible by 3), 1
enum PassSwClass { SWC_NS = 0, SWC_1 = 1, SWC_2 = 2, SWC_3 = 3, SWC_LARGE = 4 /* run-time compiled: 2 for an even number of states above 2, else 1 */ };
constexpr bool pass_class_applies(int cls, int ns) {
    return cls == SWC_2 ? (ns > 2 && ns % 2 == 0) : (cls == SWC_3 ? (ns > 3 && ns % 3 == 0) : true);
}
constexpr int pass_class_sw(int cls, int ns) { return cls == SWC_NS ? ns : (cls == SWC_LARGE ? ((ns % 2 == 0 && ns > 2) ? 2 : 1) : cls); }

// The instantiations of emi_pass_f64_kernel<Model, SW, 2, store, NST, BK, CT, HS, keep, DOP> for a built-in model, every store flavour of
// each.  X(SW class, ring stages, K-tile depth, column sub-tiles, K halves, De / Do from L2, K slices allowed, stores: -1 every flavour).
// A plan is matched to the rows from the top; for a 2-state model SW = 2 is the NS row.
#define EMI_PASS_FORMS(X)                   \
    X(SWC_NS, 3, 8, 1, 1, false, true, -1)  \
    X(SWC_2, 3, 8, 1, 2, false, false, -1)  \
    X(SWC_2, 3, 16, 1, 2, false, false, -1) \
    X(SWC_2, 3, 8, 2, 1, false, false, -1)  \
    X(SWC_2, 3, 16, 2, 1, false, false, -1) \
    X(SWC_2, 3, 16, 1, 1, true, false, -1)  \
    X(SWC_2, 3, 16, 1, 1, false, false, -1) \
    X(SWC_2, 4, 8, 1, 1, false, true, -1)   \
    X(SWC_2, 3, 8, 1, 1, false, true, -1)   \
    X(SWC_3, 3, 8, 1, 1, false, true, -1)   \
    X(SWC_1, 3, 8, 1, 2, false, false, -1)  \
    X(SWC_1, 3, 16, 1, 2, false, false, -1) \
    X(SWC_1, 3, 16, 1, 1, true, false, -1)  \
    X(SWC_1, 3, 16, 1, 1, false, false, -1) \
    X(SWC_1, 4, 8, 1, 1, false, true, -1)   \
    X(SWC_1, 3, 8, 1, 1, false, true, -1)
// ... and the two a run-time compiled model program holds: SW = 1 with plain stores (small batches) and the large-batch SW with
// non-temporal stores (K slices are a run-time argument of the kernel)
#define EMI_PASS_FORMS_RTC(X)             \
    X(SWC_1, 3, 8, 1, 1, false, true, 0)  \
    X(SWC_LARGE, 3, 8, 1, 1, false, true, 2)

struct PassForm {
    int cls, nst, bk, ct, hs;
    bool dop, slices;
    int stores;     // -1: every store flavour; else the one flavour of the row (2: launches with non-temporal stores, 0: all others)
};
#define EMI_PASS_FORM_ROW(CLS, NST, BK, CT, HS, DOP, SLICES, STORES) {CLS, NST, BK, CT, HS, DOP, SLICES, STORES},
// (inline: ONE table in the program, so that a row found in one translation unit is a row of the table in every other)
inline constexpr PassForm PASS_FORMS[] = {EMI_PASS_FORMS(EMI_PASS_FORM_ROW)};
inline constexpr PassForm PASS_FORMS_RTC[] = {EMI_PASS_FORMS_RTC(EMI_PASS_FORM_ROW)};
#undef EMI_PASS_FORM_ROW
constexpr int N_PASS_FORMS = sizeof PASS_FORMS / sizeof PASS_FORMS[0], N_PASS_FORMS_RTC = sizeof PASS_FORMS_RTC / sizeof PASS_FORMS_RTC[0];

enum PassModelClass { PASS_MODEL_NONE = 0, PASS_MODEL_BUILTIN = 1, PASS_MODEL_RTC = 2 };   // built-in with pass kernels / run-time compiled with them
struct PassShape {
    int ns = 0, M = 0;
    int model_class = PASS_MODEL_NONE;
    bool has_dfrag = false;     // the context holds the fragment-order copy of De / Do
    int store_mode = 0;         // run-time compiled models: the store flavour picks the row
};
struct PassWants {
    int sw = 0, ks = 1, nst = 3, bk = 8, ct = 1, hs = 1;
    bool dop = false;
    int res = 2;        // resident workgroups per CU the launch states: 2 or 3
};
// Resident workgroups per CU a launch of a row may state.  Not a column of the table: every row states 2, and a direct-operator row (12 /
// 24 KB of LDS, at most 160 registers) is held a second time with an allocation that admits a third (launch_pass_model instantiates it
// beside KEEP and the store flavour).  The staged rows need 72 KB of LDS at 16-deep tiles: a third workgroup never fits.
constexpr int pass_form_max_res(const PassForm& f) { return f.dop ? 3 : 2; }
struct PassResolved {
    const PassForm* row = nullptr;      // null: no form for this model and shape
    int sw = 0, ks = 1;
    int res = 2;                        // resident workgroups per CU granted
    explicit operator bool() const { return row != nullptr; }
};

// what a row asks of the shape beyond its SW class
inline bool form_fits(const PassForm& f, const PassShape& s) {
    if (f.ct == 2 && s.M % 256 != 0) return false;
    if (f.hs == 2 && ((s.M / 2) / f.bk) % 4 != 0) return false;
    if (f.dop && !s.has_dfrag) return false;
    if (f.stores >= 0 && (f.stores == 2) != (s.store_mode == 2)) return false;
    return true;
}

inline const PassForm* find_form(const PassShape& s, int sw, bool sliced, int nst, int bk, int ct, int hs, bool dop) {
    const bool rtc = s.model_class == PASS_MODEL_RTC;
    const PassForm* rows = rtc ? PASS_FORMS_RTC : PASS_FORMS;
    const int n = s.model_class == PASS_MODEL_NONE ? 0 : (rtc ? N_PASS_FORMS_RTC : N_PASS_FORMS);
    if (sw < 1 || s.M < 128 || s.M % 128 != 0 || s.ns % sw != 0) return nullptr;
    for (int i = 0; i < n; ++i) {
        const PassForm& f = rows[i];
        if (pass_class_applies(f.cls, s.ns) && pass_class_sw(f.cls, s.ns) == sw && f.nst == nst && f.bk == bk && f.ct == ct && f.hs == hs && f.dop == dop &&
            (f.slices || !sliced) && form_fits(f, s))
            return &f;
    }
    return nullptr;
}

// The wanted form snapped to one that exists: the ONLY place where a feature gives way.  SW and the K slices stand (the caller made the
// slice count legal: legal_ks); the plain form of that SW -- three stages, 8-deep K tiles, one sub-tile, undivided K, operands through the
// ring -- is the start, and each further want is granted, in this order, where a row holds it TOGETHER with everything granted before it:
//   1. four ring stages           (so: 16-deep tiles, wide tiles, halves and De / Do from L2 come with three stages only);
//   2. K tiles of 16              (only with three stages and unsplit);
//   3. two column sub-tiles       (SW = 2, unsplit, three stages, M % 256 == 0; keeps the K-tile depth granted);
//   4. the K range in two halves  (so: ct = 2 before hs = 2; unsplit, three stages);
//   5. De / Do from L2            (so: hs = 2 before dop; 16-deep, unsplit, one sub-tile, three stages, the fragment copy in place);
//   6. three resident workgroups  (last: only with a row that takes De / Do from L2, pass_form_max_res; it picks no other row).
// A want no row holds is dropped, never the launch: SW = NS and SW = 3 have the plain form only.
inline PassResolved resolve_form(const PassWants& w, const PassShape& s) {
    PassResolved r;
    const bool sliced = w.ks > 1;
    int nst = 3, bk = 8, ct = 1, hs = 1;
    bool dop = false;
    if (!find_form(s, w.sw, sliced, nst, bk, ct, hs, dop)) return r;
    if (w.nst == 4 && find_form(s, w.sw, sliced, 4, bk, ct, hs, dop)) nst = 4;
    if (w.bk == 16 && find_form(s, w.sw, sliced, nst, 16, ct, hs, dop)) bk = 16;
    if (w.ct == 2 && find_form(s, w.sw, sliced, nst, bk, 2, hs, dop)) ct = 2;
    if (w.hs == 2 && find_form(s, w.sw, sliced, nst, bk, ct, 2, dop)) hs = 2;
    if (w.dop && find_form(s, w.sw, sliced, nst, bk, ct, hs, true)) dop = true;
    r.row = find_form(s, w.sw, sliced, nst, bk, ct, hs, dop);
    r.sw = w.sw;
    r.ks = w.ks;
    r.res = (w.res == 3 && r.row && pass_form_max_res(*r.row) >= 3) ? 3 : 2;
    return r;
}

// ---- what the policy reads --------------------------------------------------------------------------------------------------------
struct PassPolicyIn {
    int ns = 0, M = 0;
    int real_bytes = 8;             // bytes per value
    int rows = 0;                   // nres + nvals: result rows a pass writes per instance and node
    int model_class = PASS_MODEL_NONE;
    int rtc_sw_large = 0;           // run-time compiled: SW of its large-batch instantiation
    bool f32 = false, symmetric = false, has_dfrag = false;
    // the options (emi_set_option), as the context holds them
    int allow_fused = 1, overlap_mode = 0, sym_ct = 0, sym_ksplit = 0, sym_cpart = 0, sym_gblk = 0, sym_cx = 0, sym_nst = 3, sym_hs = 0, sym_ctc = 0,
        sym_bk = 0, sym_dop = 0, sym_res = 0, pass_order = -1, node_store = -1, slice = 0, small_rows = 24;
    // the context holds a per-instance parameter table (emi_set_model_params_batch): the MFMA forms evaluate f in their epilogue for 16
    // instances per tile, one per lane, and have no tabled instantiation -- such a context takes the sequential route, as under "overlap" 0
    bool param_table = false;
};

// the even/odd MFMA defect kernel beside the node kernel (or both roles in one launch): needs an exactly centro-antisymmetric D
inline bool pass_overlapped(const PassPolicyIn& in) {
    if (in.f32 || !in.allow_fused || in.param_table || !in.symmetric || in.M <= 0 || in.model_class == PASS_MODEL_NONE) return false;
    if (in.model_class == PASS_MODEL_RTC) return in.M % 128 == 0;
    return symdefect_shape_ok(in.M, in.sym_ct);
}

inline int pass_tiles16(const PassPolicyIn& in, int B) { return ((B + 15) / 16) * (in.M / 128); }

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
inline int store_mode_for(const PassPolicyIn& in, int B) {
    if (in.node_store >= 0) return in.node_store;
    if ((size_t)B * in.rows * in.M * in.real_bytes > ((size_t)230 << 20)) return 2;
    // (17 .. 32 tiles -- 33 .. 64 instances at 1024 nodes, the two-slice band -- are the one place where plain stores stay ahead: 48 instances
    // 0.0197 / 0.0203, 64: 0.0209 / 0.0215)
    const int tiles16 = pass_tiles16(in, B);
    if (tiles16 > 16 && tiles16 <= 32) return 0;
    return (in.model_class != PASS_MODEL_RTC && !in.f32) ? 1 : 0;
}

// ---- the band table: the defaults of ONE launch by its size -----------------------------------------------------------------------
// The pass as ONE launch: MFMA-role and node-role workgroups in one grid, COST finished in-kernel -- since round 3 at EVERY
// batch size (round 2: two streams between 384 and 767 instances, which ran 20 - 25 % under the rest).  One box, interleaved
// rounds, M = 1024, ms per pass, best one-launch form against the round-2 choice (profiles/r03_mid_sweep.json): 256: 0.0581 /
// 0.0731, 320: 0.0749 / 0.0927, 384: 0.0879 / 0.1177 (two streams), 448: 0.1035 / 0.1038, 512: 0.1188 / 0.1162, 576: 0.1332 /
// 0.1777, 640: 0.146 / 0.155, 704: 0.160 / 0.181.
// A row is keyed by tiles16 (16-instance x 128-node tiles of the launch) and gives the default wants; the first row that holds the
// launch and whose conditions are met is taken.  The conditional rows (the 16-deep bands of round 4 and later) are for built-in models
// under the default dispatch ("overlap_mode" 0, "sym_ct" 0 / 4) and stand back where an option they were not measured with is set; the
// unconditional rows below them (round 3) hold every launch.
enum PassBandNeeds : unsigned {
    BAND_EVEN_NS = 1u,      // an even number of states above two, where the row was measured: the 6-state quadrotor
    BAND_FREE_KS = 2u,      // "sym_ksplit" unset
    BAND_FREE_DEPTH = 4u,   // "sym_bk" unset and three ring stages ("sym_nst")
    BAND_FREE_ORDER = 8u,   // "pass_order" unset
    BAND_DEFAULT = 16u,     // built-in model, default dispatch
    BAND_FREE_RES = 32u,    // "sym_res" unset and neither "sym_dop" 1 nor K halves, wide tiles or K slices asked for: free to state three resident
                            // workgroups (a row whose order and operand source were measured with them; otherwise it stands back and the row
                            // behind it, measured with two, holds the launch)
};
enum PassKsRule {
    KS_UNSPLIT,
    // K slices per tile ("sym_ksplit"; partial sums combined in-kernel by ticket, in slice order).  By itself only where the MFMA
    // role has fewer workgroups than the chip has places for them, i.e. where a pass waits for one 64-tile dependency chain per
    // workgroup: 4 slices while that keeps the role within 256 workgroups, 2 within 512.  One box, M = 1024, ms per pass
    // unsplit / 2 / 4 slices (tools/mid_sweep.py, profiles/r03_notes.md section 7): B = 8: 0.0204 / 0.0148 / 0.0140,
    // 16: 0.0235 / 0.0179 / 0.0155, 32: 0.0242 / 0.0190 / 0.0192, 64: 0.0257 / 0.0218 / 0.0261, 80: 0.0263 / 0.0249 / 0.0312,
    // 96: 0.0288 / 0.0290 / 0.0407, 128: 0.0333 / 0.0387 / 0.0496 (from ~500 workgroups the split loses: three and more MFMA
    // waves per SIMD share the matrix pipe and the node role starts behind them)
    KS_BY_WORKGROUPS,
};
struct PassBand {
    int lo, hi;         // tiles16, both inclusive
    unsigned needs;
    int sw_ct;          // SW class as the "sym_ct" code: 7 = one state per MFMA workgroup, 6 = two
    PassKsRule ks;
    int bk;             // K-tile depth
    int dop;            // operand source: 1 De / Do through the ring, 2 straight from L2
    int order;          // block order (pass_role_of): 1 MFMA workgroups first, 0 evenly interleaved, >= 100: at that % of the even density
    int res = 2;        // resident workgroups per CU the launch states ("sym_res"): 3 only beside dop 2, and only where it was measured ahead
};
constexpr unsigned BAND_DEEP = BAND_DEFAULT | BAND_FREE_DEPTH;
inline constexpr PassBand PASS_BANDS[] = {
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
    // (both for an even number of states above two, where they were measured: the 6-state quadrotor)
    {33, 48, BAND_DEEP | BAND_FREE_KS | BAND_EVEN_NS, 7, KS_UNSPLIT, 16, 1, 1},            // deep_small
    // Three resident workgroups per CU ("sym_res" 3: the direct-operator form with a register allocation that admits a third wave per SIMD,
    // 768 places on the chip instead of 512) at 80 tiles (145 .. 160 instances): the first size whose workgroups of both roles (240 + 320) are no
    // longer all resident at two per CU.  One box each, ms per pass median (min - max), deep_mid / direct form, three resident, MFMA workgroups
    // first (profiles/residency_sweep.jsonl, profiles/residency_notes.md section 3): 152 instances 0.0334 (0.0334 - 0.0334) / 0.0310 (0.0309 -
    // 0.0311), 160: 0.0333 (0.0333 - 0.0333) / 0.0311 (0.0311 - 0.0312), and 0.0342 (0.0342 - 0.0343) / 0.0312 (0.0311 - 0.0314) on another box.
    // Not at 144 (0.0271 either way) nor at 176 (0.0408 / 0.0425) and 192 (0.0411 / 0.0439).
    {80, 80, BAND_DEEP | BAND_FREE_KS | BAND_EVEN_NS | BAND_FREE_RES, 6, KS_UNSPLIT, 16, 2, 1, 3},     // deep_mid, three resident
    {49, 127, BAND_DEEP | BAND_FREE_KS | BAND_EVEN_NS, 6, KS_UNSPLIT, 16, 1, 1},           // deep_mid
    // ... and between 144 and 207 tiles (288 .. 415 instances) TOGETHER with the MFMA workgroups at 1.5 x the even density instead of all
    // of them first: from ~300 instances the role's 3 x tiles workgroups no longer fit beside the node role (64 places per XCD), which then
    // starts a workgroup generation late.  End of round 4, one box, ms per pass, first + 8-deep (the choice until then) / 1.5 x + 16-deep:
    // 288 instances 0.0730 / 0.0699, 320: 0.0859 / 0.0754, 352: 0.1004 / 0.0820, 384: 0.1022 / 0.0875; 272: 0.0644 / 0.0698 (stays),
    // 416 (1.25 x + 16-deep already): 0.0946 / 0.0951 (profiles/r04_mid_sweep_band_288_416.jsonl)
    {144, 207, BAND_DEEP | BAND_FREE_ORDER | BAND_EVEN_NS, 6, KS_BY_WORKGROUPS, 16, 1, 150},   // deep_band
    // K tiles of 16 between 208 and 767 tiles (416 .. 1535 instances, SW = 2 at 1.25 x / 1.1 x the even MFMA density): one box, ms per pass 8- /
    // 16-deep, 448 instances 0.1112 / 0.1018, 512: 0.1226 / 0.1151, 576: 0.1351 / 0.1277, 640: 0.1492 / 0.1431, 768: 0.1675 / 0.1649,
    // 896: 0.1921 / 0.1896, 1024: 0.2164 / 0.2143; not at 256 .. 384 instances (MFMA workgroups first: 320: 0.0752 / 0.0924) nor from 2048
    // (0.4147 / 0.4205; 4096 in the grouped order 1.081 / 1.175)
    // (up to 1024 tiles -- 2048 instances -- since the end of round 4: with the pass kernel's register allocation stated, 8- / 16-deep at 1536
    // instances 0.3204 / 0.3117, 1792: 0.3725 / 0.3611, 2048: 0.4441 / 0.4322, profiles/r04_mid_sweep_1280_2048.jsonl)
    {208, 215, BAND_DEEP | BAND_FREE_ORDER, 6, KS_BY_WORKGROUPS, 16, 1, 125},              // deep_large
    // De / Do fragments straight from L2 into the MFMA waves' registers instead of through the operand ring ("sym_dop" 2; built-in models,
    // SW 1 or 2 of more states, 16-deep K tiles, unsplit, one sub-tile, three stages; the context holds the fragment-order copy)
    // By itself from 216 tiles (432 instances) through the range of deep_large.  One box, M = 1024, ms per pass through the ring / straight
    // from L2 (tools/mid_sweep.py dop1,dop2; profiles/r06_mid_sweep_dop.jsonl): 432 instances 0.0903 / 0.0865, 512: 0.1002 / 0.0975, 768: 0.1446 /
    // 0.1412, 1024: 0.1879 / 0.1836, 1536: 0.2790 / 0.2735, 2048: 0.3771 / 0.3671.  Below that neither form is ahead: the pass time moves with how
    // the workgroups of the two roles fill the chip, not with the K loop (128: 0.0261 / 0.0262, 176: 0.0412 / 0.0392, 224: 0.0425 / 0.0434, 288:
    // 0.0614 / 0.0631, 352: 0.0774 / 0.0714, 416: 0.0824 / 0.0835; SW = 1: 80 instances 0.0192 / 0.0208, 96: 0.0246 / 0.0240), so those stay.
    // ... with three resident workgroups per CU and the MFMA workgroups at 1.1 x the even density from 512 tiles (1024 .. 2048 instances): node
    // workgroups that wait on the write stream no longer hold the places MFMA workgroups could compute in.  One box, timed regions of 0.4 s, five
    // interleaved rounds, ms per pass median (min - max), shipped choice (two resident; 1.1 x up to 1535 instances, even from there) / three
    // resident at 1.1 x (profiles/residency_sweep.jsonl, "sweep": "large"): 1024 instances 0.1794 (0.1793 - 0.1796) / 0.1747 (0.1744 - 0.1748),
    // 1152: 0.2007 (0.2005 - 0.2008) / 0.1950 (0.1948 - 0.1951), 1280: 0.2219 (0.2217 - 0.2221) / 0.2150 (0.2148 - 0.2151), 1536: 0.2669 (0.2666 -
    // 0.2670) / 0.2555 (0.2554 - 0.2556), 1792: 0.3101 (0.3100 - 0.3106) / 0.2963 (0.2962 - 0.2972), 2048: 0.3541 (0.3537 - 0.3545) / 0.3367 (0.3366 -
    // 0.3370): 2.6 - 4.9 %, 13 - 27 times the shipped choice's spread, every run below every run.  Two resident at 1.1 x from 1536 instances gains
    // 0 - 1 % only, so it is the residency.  Not below: 768 instances 0.1371 / 0.1361 (twice the spread), 896: 0.1581 / 0.1553 with one run of
    // the five at 0.1685; at 432 and 512 nothing is gained at any of five orders (0.0854 / 0.0849 and 0.0981 / 0.0995 at best).
    // (for an even number of states above two, where it was measured, and unless an option says otherwise: BAND_FREE_RES)
    {512, 1024, BAND_DEEP | BAND_FREE_ORDER | BAND_EVEN_NS | BAND_FREE_RES, 6, KS_BY_WORKGROUPS, 16, 2, 110, 3},   // deep_large, De / Do from L2, three resident
    {216, 383, BAND_DEEP | BAND_FREE_ORDER, 6, KS_BY_WORKGROUPS, 16, 2, 125},              // deep_large, De / Do from L2
    {384, 767, BAND_DEEP | BAND_FREE_ORDER, 6, KS_BY_WORKGROUPS, 16, 2, 110},
    {768, 1024, BAND_DEEP | BAND_FREE_ORDER, 6, KS_BY_WORKGROUPS, 16, 2, 0},
    // Round 3, every launch:
    //   * SW (states per MFMA workgroup): 1 below 128 sixteen-instance x 128-node tiles (more workgroups than CUs), else 2;
    //   * block order (pass_role_of): MFMA workgroups first below 208 tiles (their 64-tile dependency chains start at once, the
    //     streaming workgroups fill in behind; since the end of round 4 only below 144 tiles: 1.5 x the even density from there, see
    //     deep_band above), at 1.25 x the even density up to 384 tiles, at 1.1 x up to 768, evenly interleaved
    //     from there (B >= 768, where "first" would hold the node role back: 0.288 against 0.222 at 1024).  (Round 2 measured
    //     "first" against "interleaved" WITH PLAIN STORES at 256 instances and found interleaved ahead, 0.0727 / 0.0748; with
    //     non-temporal stores "first" wins up to 448 instances: 256: 0.0581 against 0.0756 interleaved.  End of round 3, one box,
    //     e9 node-evals/s at first / 1.25 x / 1.5 x / even: 448 instances 4.21 / 4.41 / 4.22 / 4.31, 512: 3.60 / 4.32 / 4.38 / 4.22,
    //     640: 3.76 / 4.48 / 4.37 / 4.37, 704: 3.89 / 4.63 / 4.45 / 4.50; ms per pass at even / 1.1 x / 1.25 x: 768: 0.1747 /
    //     0.1696 / 0.1760, 896: 0.1964 / 0.1959 / 0.2022, 1024: 0.2230 / 0.2200 / 0.2304, 1536: 0.3215 / 0.3219 / 0.3411,
    //     2048: 0.4239 / 0.4227 / 0.4415).
    {0, 127, 0, 7, KS_BY_WORKGROUPS, 8, 1, 1},
    {128, 207, 0, 6, KS_BY_WORKGROUPS, 8, 1, 1},
    {208, 383, 0, 6, KS_BY_WORKGROUPS, 8, 1, 125},
    {384, 767, 0, 6, KS_BY_WORKGROUPS, 8, 1, 110},
    {768, INT_MAX, 0, 6, KS_BY_WORKGROUPS, 8, 1, 0},
};

// ... and the one default that goes by instances, not tiles: launches of more than 2048 instances in whole super-blocks of 256.
//   * tile order: grouped (an XCD's MFMA tiles and node workgroups walk the same instance groups together), else column partitions by
//     mesh size (plan_symdefect);
//   * two column sub-tiles per MFMA workgroup ("sym_ctc" 2; built-in models, SW = 2, unsplit, three stages) in column blocks of one
//     128-column tile (inputs beyond the Infinity Cache, where every operand read is an HBM read): one box, ms per pass one / two sub-tiles,
//     4096 instances 1.181 / 1.101, 16384: 4.407 / 4.044 (3.81e9 -> 4.15e9 node-evals/s) with column blocks of one 128-column tile; at 2048
//     instances 0.4736 / 0.4636, at 1024 and below the narrow form is ahead (0.2222 / 0.2425: the wide workgroups need 60 KB of LDS and 160
//     registers) (profiles/r04_mid_sweep.jsonl)
struct PassLargeBatch { int above, whole; int gblk, ct, cx; };
inline constexpr PassLargeBatch PASS_LARGE_BATCH = {2048, 256, 2, 2, 1};

inline const PassBand& band_for(const PassPolicyIn& in, int tiles16, bool auto_ct) {
    unsigned met = 0;
    if (in.ns % 2 == 0 && in.ns > 2) met |= BAND_EVEN_NS;
    if (in.sym_ksplit == 0) met |= BAND_FREE_KS;
    if (in.sym_bk == 0 && in.sym_nst == 3) met |= BAND_FREE_DEPTH;
    if (in.pass_order < 0) met |= BAND_FREE_ORDER;
    // (three resident workgroups come with the direct form only: an option that takes that form away -- resolve_form -- takes the row away)
    if (in.sym_res == 0 && in.sym_dop != 1 && in.sym_hs <= 1 && in.sym_ctc <= 1 && in.sym_ksplit <= 1) met |= BAND_FREE_RES;
    if (auto_ct && in.model_class == PASS_MODEL_BUILTIN) met |= BAND_DEFAULT;
    const PassBand* b = PASS_BANDS;
    while (!(tiles16 >= b->lo && tiles16 <= b->hi && (b->needs & ~met) == 0)) ++b;      // (the unconditional rows hold every launch)
    return *b;
}

// Everything the default dispatch decides about ONE launch of the evaluation pass as emi_pass_f64_kernel: what choose_form /
// form_pass_f64 (emi_api_pass.hip) launch by and what emi_plan_pass reports.  The fields of `sym` are those of the form that is launched.
struct PassPlan {
    bool one_launch = false;    // the pass goes out as ONE launch (MFMA-role + node-role workgroups)
    SymPlan sym;                // MFMA role: states per workgroup, K slices per tile, ring stages, tile order
    int tiles16 = 0;            // 16-instance x 128-node tiles of the launch (what the bands are written in)
    int store_mode = 0;         // node role: 0 plain, 1 sc1, 2 non-temporal, 3 nt sc1
    int mfma_first = 0;         // block order (pass_role_of): 1 MFMA workgroups first, 0 evenly interleaved, >= 100: at that % of the even density
};

// Tiles and tile order for the resolved form: ONE plan_symdefect call, at the column width of the form.
// (A 2-state model has no SW = 2 rows: where it asks for two column sub-tiles and the shape would allow them, its NS form goes out in the
// tile order planned for the wide tiles, as it always did; the tile count is that of the form.)
inline SymPlan plan_tiles(const PassPolicyIn& in, int B, const PassWants& w, const PassResolved& r, int gblk, int band_cx) {
    const PassForm& f = *r.row;
    const bool wide_order = f.ct == 2 || (in.model_class == PASS_MODEL_BUILTIN && w.ct == 2 && r.sw == 2 && r.ks == 1 && w.nst == 3 && in.M % 256 == 0);
    const int cx = in.sym_cx ? in.sym_cx : (wide_order ? band_cx : 0);
    SymPlan p = plan_symdefect(in.ns, B, in.M, symdefect_ct_of(in.ns, r.sw), r.ks, in.sym_cpart, gblk, cx, 8, wide_order ? 2 : 1);
    p.tiles = p.tiles * p.ct / f.ct;
    p.nst = f.nst;
    p.bk = f.bk;
    p.ct = f.ct;
    p.hs = f.hs;
    p.dop = f.dop;
    p.res = r.res;
    return p;
}

// The key of the work table of a planned launch (emi_pass_work.hpp): what the blocks of its grid do follows from the form's tiles and
// K slices, its tile order and the block order, and from nothing else.
inline PassWorkKey pass_work_for(const SymPlan& sym, int ns, int B, int M, int order) {
    return pass_work_key(ns, B, M, sym.sw, sym.ct, sym.ks, sym.hs, sym.cpart, sym.cx, order);
}

// Every choice can be forced through emi_set_option (sym_ct, sym_ksplit, sym_cpart, sym_gblk, sym_cx, sym_nst, sym_bk, sym_ctc, sym_hs,
// sym_dop, sym_res, pass_order, node_store); a run-time compiled model is planned within its two instantiations.
inline PassPlan plan_pass(const PassPolicyIn& in, int B, bool jac) {
    PassPlan p;
    p.tiles16 = pass_tiles16(in, B);
    p.store_mode = store_mode_for(in, B);
    const bool auto_mode = in.overlap_mode == 0, rtc = in.model_class == PASS_MODEL_RTC;
    if (!((in.overlap_mode == 3 || auto_mode) && jac) || in.M % 128 != 0) return p;
    const bool auto_ct = auto_mode && (in.sym_ct == 0 || in.sym_ct == 4);
    // 1. the defaults of the band (and of a large batch)
    const PassBand& band = band_for(in, p.tiles16, auto_ct);
    const bool large = B > PASS_LARGE_BATCH.above && B % PASS_LARGE_BATCH.whole == 0 && in.sym_cpart == 0;
    const bool wide_large = auto_ct && large && in.sym_ctc == 0;       // (the wide tiles and their column blocks come together)
    // 2. options that are set override them
    const int ct_code = rtc ? ((p.store_mode == 2 && in.rtc_sw_large == 2) ? 6 : 7) : (auto_ct ? band.sw_ct : in.sym_ct);
    PassWants w;
    w.sw = symdefect_sw(in.ns, p.tiles16, ct_code);
    if (w.sw == 0) w.sw = in.ns;            // (the one-workgroup-per-CU ring kernel has no one-launch form: all the states)
    w.ks = in.sym_ksplit;
    if (w.ks == 0 && auto_ct && band.ks == KS_BY_WORKGROUPS) {
        const int wgs = p.tiles16 * (in.ns / w.sw);
        w.ks = wgs * 4 <= 256 ? 4 : (wgs * 2 <= 512 ? 2 : 1);
    }
    w.ks = legal_ks((in.M / 2) / 8, w.ks);         // (slices are planned in 8-deep K tiles: deeper tiles go unsplit)
    w.nst = in.sym_nst;
    w.bk = in.sym_bk ? in.sym_bk : band.bk;
    w.ct = in.sym_ctc ? in.sym_ctc : (wide_large ? PASS_LARGE_BATCH.ct : 1);
    w.hs = in.sym_hs ? in.sym_hs : 1;
    w.dop = (in.sym_dop ? in.sym_dop : band.dop) == 2;
    w.res = (in.sym_res ? in.sym_res : band.res) == 3 ? 3 : 2;
    // (the grouped order by default: not for a built-in model whose K slices an option set)
    const int gblk = (large && in.sym_gblk == 0 && (rtc || (auto_ct && w.ks == 1))) ? PASS_LARGE_BATCH.gblk : in.sym_gblk;
    // 3. the form that exists, and its tiles
    PassShape s;
    s.ns = in.ns;
    s.M = in.M;
    s.model_class = in.model_class;
    s.has_dfrag = in.has_dfrag;
    s.store_mode = p.store_mode;
    const PassResolved r = resolve_form(w, s);
    if (!r) return p;
    p.sym = plan_tiles(in, B, w, r, gblk, wide_large ? PASS_LARGE_BATCH.cx : 0);
    p.mfma_first = in.pass_order >= 0 ? in.pass_order : band.order;
    p.one_launch = true;
    return p;
}

// the one-launch pass in its small-batch form (SW = 1, plain stores) is available by the default dispatch
inline bool pass_takes_small_batches(const PassPolicyIn& in) {
    if (!pass_overlapped(in) || (in.overlap_mode != 0 && in.overlap_mode != 3) || in.M % 128 != 0) return false;
    PassShape s;
    s.ns = in.ns;
    s.M = in.M;
    s.model_class = in.model_class;
    PassWants w;
    w.sw = 1;
    return (bool)resolve_form(w, s);
}

// Large batches: the instances one launch of emi_eval_dev's default dispatch takes (0: the whole batch in one).  Round 2 cut
// everything above 2048 instances into 1024-instance launches (the two-stream form drifted apart on long launches); with the pass
// as ONE launch that buys nothing, and inputs of more than ~256 MB no longer stay in the Infinity Cache from one pass to the next,
// which is what really slows a large batch (B = 16384: 3.47e9 node-evals/s sliced or not, profiles/r03_notes.md).  Now: one launch
// over the whole batch in the GROUPED tile order: 4.10e9 /s at 16384 instances, 4.13e9 at 4096.  Pieces remain only where
// something forces them: the "slice" option (> 0: pieces of that many instances once B > 2 slice), the 32-bit operand offsets of
// the MFMA role (X of a launch below 4 GB), and a remainder that is not a multiple of 256 instances (the grouped order wants whole
// super-blocks on every XCD) as a second launch.
inline int plan_piece(const PassPolicyIn& in, int B) {
    const long long cap = ((0xFFFFFFFFLL / ((long long)in.ns * in.M * 8)) / 256) * 256;     // instances whose X stays below 4 GB
    int piece = 0;
    if (in.slice > 0) { if (B > 2 * in.slice) piece = in.slice; }
    else if (B > 2048) piece = (int)std::min<long long>(cap > 0 ? cap : 256, B - B % 256);
    return piece >= B ? 0 : piece;
}

// what emi_plan_pass reports for a batch of B instances (*out zeroed by the caller); *dop: the operand source of the form, which the
// report has no field for, *res: the resident workgroups per CU it states, likewise (0: the pass does not go out as one launch)
inline void report_pass(const PassPolicyIn& in, int B, emi_pass_plan_t* out, bool* dop = nullptr, int* res = nullptr) {
    if (dop) *dop = false;
    if (res) *res = 0;
    if (!pass_overlapped(in)) return;
    const int piece = plan_piece(in, B);
    out->piece = piece;
    out->tail = piece > 0 ? B % piece : 0;
    const PassPlan p = plan_pass(in, piece > 0 ? piece : B, true);     // the first launch
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
    if (dop) *dop = p.sym.dop;
    if (res) *res = p.one_launch ? p.sym.res : 0;
}

}  // namespace emi
