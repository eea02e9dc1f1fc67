// pass_residency_main.cpp -- the residency rule of the fp64 evaluation pass (etol_amd/csrc/emi_pass_plan.hpp, host-only: "sym_res",
// PassWants::res, resolve_form step 6, PassBand::res) as a stand-alone program under the host sanitizers (`make check-pass-residency`):
// no Python, no device.
//   (no argument)                          hold the rule over a grid of contexts, batches and options:
//                                            * three resident workgroups per CU are stated only by a launch of a direct-operator row;
//                                            * "sym_res" 3 is granted whenever the plan resolves to such a row, "sym_res" 2 always;
//                                            * a want no row holds is dropped, never the launch, and it picks no other row: but for the
//                                              residency, the plans under "sym_res" 2 and 3 are the same;
//                                            * built-in models only;
//                                            * the options combine in the order resolve_form documents;
//                                            * the default by band is the one profiles/residency_notes.md arrives at.
//   plan NS NC M B [option=value ...]      print the plan of one context with its residency (np=N: with N path rows)
// The contexts are those of pass_plan_main.cpp: a symmetric LGL mesh (so the fragment copy of De / Do exists), no path rows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "emi_pass_plan.hpp"

namespace {

using emi::PassPolicyIn;

struct Option {
    const char* name;
    int PassPolicyIn::*field;
    std::vector<int> values;
};
// the options the residency is crossed with (each alone, beside "sym_res" and "sym_dop")
const std::vector<Option> CROSSED = {
    {"none", &PassPolicyIn::sym_cx, {0}},
    {"sym_ct", &PassPolicyIn::sym_ct, {5, 6, 7, 8}},
    {"sym_ksplit", &PassPolicyIn::sym_ksplit, {1, 2, 4}},
    {"sym_bk", &PassPolicyIn::sym_bk, {8, 16}},
    {"sym_ctc", &PassPolicyIn::sym_ctc, {2}},
    {"sym_hs", &PassPolicyIn::sym_hs, {2}},
    {"sym_nst", &PassPolicyIn::sym_nst, {4}},
    {"pass_order", &PassPolicyIn::pass_order, {0, 1, 110, 150}},
    {"node_store", &PassPolicyIn::node_store, {0, 2}},
    {"overlap_mode", &PassPolicyIn::overlap_mode, {1, 2, 3}},
    {"slice", &PassPolicyIn::slice, {256}},
};
// every option a `plan` call takes
const std::vector<Option> NAMED = {
    {"sym_ct", &PassPolicyIn::sym_ct, {}},         {"sym_ksplit", &PassPolicyIn::sym_ksplit, {}}, {"sym_bk", &PassPolicyIn::sym_bk, {}},
    {"sym_ctc", &PassPolicyIn::sym_ctc, {}},       {"sym_hs", &PassPolicyIn::sym_hs, {}},         {"sym_nst", &PassPolicyIn::sym_nst, {}},
    {"sym_cpart", &PassPolicyIn::sym_cpart, {}},   {"sym_gblk", &PassPolicyIn::sym_gblk, {}},     {"pass_order", &PassPolicyIn::pass_order, {}},
    {"node_store", &PassPolicyIn::node_store, {}}, {"overlap_mode", &PassPolicyIn::overlap_mode, {}}, {"slice", &PassPolicyIn::slice, {}},
    {"sym_dop", &PassPolicyIn::sym_dop, {}},       {"sym_cx", &PassPolicyIn::sym_cx, {}},         {"sym_res", &PassPolicyIn::sym_res, {}},
};
const int BATCHES[] = {1, 16, 64, 128, 144, 160, 192, 256, 320, 431, 432, 512, 768, 1024, 1536, 2048, 2049, 4096};
struct Model { const char* name; int ns, nc; };
const Model MODELS[] = {{"pointmass2", 2, 2}, {"quadrotor6", 6, 2}};
const int MESHES[] = {128, 256, 1024};

// a built-in fp64 context on a symmetric mesh of M nodes, no path rows, default options
PassPolicyIn context(int ns, int nc, int M) {
    PassPolicyIn in;
    in.ns = ns;
    in.M = M;
    in.real_bytes = 8;
    in.rows = ns + ns * (ns + nc) + (ns + nc);
    in.model_class = emi::PASS_MODEL_BUILTIN;
    in.symmetric = true;
    in.has_dfrag = M % 128 == 0;
    return in;
}

struct Planned {
    emi_pass_plan_t p;
    bool dop;
    int res;
};
Planned plan_of(const PassPolicyIn& in, int B) {
    Planned q;
    std::memset(&q.p, 0, sizeof q.p);
    emi::report_pass(in, B, &q.p, &q.dop, &q.res);
    return q;
}

void print_plan(const Planned& q) {
    const emi_pass_plan_t& p = q.p;
    std::printf("{\"one_launch\": %d, \"sw\": %d, \"ksplit\": %d, \"ring_stages\": %d, \"block_order\": %d, \"tiles16\": %d, \"k_tile\": %d, \"column_tiles\": %d, "
                "\"k_halves\": %d, \"store_mode\": %d, \"dop\": %d, \"res\": %d}\n",
                p.one_launch, p.sw, p.ksplit, p.ring_stages, p.block_order, p.tiles16, p.k_tile, p.column_tiles, p.k_halves, p.store_mode, q.dop ? 1 : 0, q.res);
}

int failures = 0;
#define EXPECT(cond, name)                                                                    \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, std::string(name).c_str(), #cond); \
            ++failures;                                                                       \
        }                                                                                     \
    } while (0)

// ---- the rule over the grid ----------------------------------------------------------------------------------------------------------
int walk_grid() {
    int cases = 0;
    for (const Model& m : MODELS)
        for (int M : MESHES)
            for (const Option& o : CROSSED)
                for (int v : o.values)
                    for (int dop = 0; dop <= 2; ++dop)
                        for (int B : BATCHES) {
                            PassPolicyIn in = context(m.ns, m.nc, M);
                            in.*(o.field) = v;
                            in.sym_dop = dop;
                            const std::string name = std::string(m.name) + " M=" + std::to_string(M) + " " + o.name + "=" + std::to_string(v) + " sym_dop=" +
                                                     std::to_string(dop) + " B=" + std::to_string(B);
                            Planned q[3];
                            const int wants[3] = {0, 2, 3};
                            for (int i = 0; i < 3; ++i) {
                                in.sym_res = wants[i];
                                q[i] = plan_of(in, B);
                                ++cases;
                                // what is stated: 2 or 3 by a launch of the pass kernel, nothing otherwise; 3 only beside a direct-operator row
                                EXPECT(q[i].res == (q[i].p.one_launch ? (q[i].res == 3 ? 3 : 2) : 0), name);
                                EXPECT(q[i].res != 3 || q[i].dop, name);
                                if (q[i].p.one_launch && q[i].res == 3) {
                                    emi::PassShape s;
                                    s.ns = in.ns, s.M = in.M, s.model_class = in.model_class, s.has_dfrag = in.has_dfrag, s.store_mode = q[i].p.store_mode;
                                    const emi::PassForm* row = emi::find_form(s, q[i].p.sw, q[i].p.ksplit > 1, q[i].p.ring_stages, q[i].p.k_tile,
                                                                              q[i].p.column_tiles, q[i].p.k_halves, q[i].dop);
                                    EXPECT(row && row->dop && emi::pass_form_max_res(*row) == 3, name);
                                }
                            }
                            // the launch is never dropped
                            EXPECT(q[1].p.one_launch == q[0].p.one_launch && q[2].p.one_launch == q[0].p.one_launch, name);
                            // "sym_res" 2 always holds; 3 is granted exactly where the row takes De / Do from L2
                            EXPECT(q[1].res == (q[1].p.one_launch ? 2 : 0), name);
                            EXPECT(q[2].res == (q[2].p.one_launch ? (q[2].dop ? 3 : 2) : 0), name);
                            // the residency picks no other row and no other order: 2 and 3 differ in nothing else
                            EXPECT(std::memcmp(&q[1].p, &q[2].p, sizeof q[1].p) == 0 && q[1].dop == q[2].dop, name);
                            // with De / Do through the ring forced, or an option that takes the direct form away (K halves, wide tiles, K slices), the
                            // bands measured with three resident workgroups stand back: the plan of "sym_res" 2
                            const bool takes_away = v > 1 && (o.field == &PassPolicyIn::sym_hs || o.field == &PassPolicyIn::sym_ctc || o.field == &PassPolicyIn::sym_ksplit);
                            if (dop == 1 || takes_away) EXPECT(q[0].res == q[1].res && std::memcmp(&q[0].p, &q[1].p, sizeof q[0].p) == 0 && q[0].dop == q[1].dop, name);
                        }
    return cases;
}

// ---- built-in models only --------------------------------------------------------------------------------------------------------------
void check_run_time_models() {
    for (int sw_large : {1, 2})
        for (int M : MESHES)
            for (int B : BATCHES)
                for (int dop : {0, 2}) {
                    PassPolicyIn in = context(6, 2, M);
                    in.model_class = emi::PASS_MODEL_RTC;
                    in.rtc_sw_large = sw_large;
                    in.sym_dop = dop;
                    in.sym_res = 3;
                    const Planned q = plan_of(in, B);
                    EXPECT(q.res == (q.p.one_launch ? 2 : 0) && !q.dop, "run-time compiled model M=" + std::to_string(M) + " B=" + std::to_string(B));
                }
    for (const emi::PassForm& f : emi::PASS_FORMS_RTC) EXPECT(emi::pass_form_max_res(f) == 2, "run-time compiled form table");
}

// ---- the order of resolve_form ---------------------------------------------------------------------------------------------------------
struct Want { int sw, ks, nst, bk, ct, hs; bool dop; int res; };
struct Got { int nst, bk, ct, hs; bool dop; int res; };
void check_order() {
    emi::PassShape s;
    s.ns = 6, s.M = 1024, s.model_class = emi::PASS_MODEL_BUILTIN, s.has_dfrag = true, s.store_mode = 2;
    const struct { const char* name; Want w; bool dfrag; Got g; } CASES[] = {
        // everything the direct form needs, and the third workgroup with it
        {"direct, two states", {2, 1, 3, 16, 1, 1, true, 3}, true, {3, 16, 1, 1, true, 3}},
        {"direct, one state", {1, 1, 3, 16, 1, 1, true, 3}, true, {3, 16, 1, 1, true, 3}},
        {"direct, residency 2", {2, 1, 3, 16, 1, 1, true, 2}, true, {3, 16, 1, 1, true, 2}},
        // the third workgroup is the LAST want: whatever took De / Do from L2 away took it too
        {"staged", {2, 1, 3, 16, 1, 1, false, 3}, true, {3, 16, 1, 1, false, 2}},
        {"four stages first", {2, 1, 4, 16, 1, 1, true, 3}, true, {4, 8, 1, 1, false, 2}},
        {"8-deep tiles", {2, 1, 3, 8, 1, 1, true, 3}, true, {3, 8, 1, 1, false, 2}},
        {"wide tiles before the operand source", {2, 1, 3, 16, 2, 1, true, 3}, true, {3, 16, 2, 1, false, 2}},
        {"halved K before the operand source", {2, 1, 3, 16, 1, 2, true, 3}, true, {3, 16, 1, 2, false, 2}},
        {"K slices", {2, 2, 3, 16, 1, 1, true, 3}, true, {3, 8, 1, 1, false, 2}},
        {"all the states", {6, 1, 3, 16, 1, 1, true, 3}, true, {3, 8, 1, 1, false, 2}},
        {"three states", {3, 1, 3, 16, 1, 1, true, 3}, true, {3, 8, 1, 1, false, 2}},
        {"no fragment copy", {2, 1, 3, 16, 1, 1, true, 3}, false, {3, 16, 1, 1, false, 2}},
    };
    for (const auto& c : CASES) {
        emi::PassWants w;
        w.sw = c.w.sw, w.ks = c.w.ks, w.nst = c.w.nst, w.bk = c.w.bk, w.ct = c.w.ct, w.hs = c.w.hs, w.dop = c.w.dop, w.res = c.w.res;
        s.has_dfrag = c.dfrag;
        const emi::PassResolved r = emi::resolve_form(w, s);
        EXPECT((bool)r, c.name);
        if (!r) continue;
        EXPECT(r.row->nst == c.g.nst && r.row->bk == c.g.bk && r.row->ct == c.g.ct && r.row->hs == c.g.hs && r.row->dop == c.g.dop, c.name);
        EXPECT(r.res == c.g.res && r.sw == c.w.sw && r.ks == c.w.ks, c.name);
    }
    // a shape that has no form at all has no residency either
    emi::PassWants w;
    w.sw = 4, w.res = 3;
    s.has_dfrag = true;
    EXPECT(!emi::resolve_form(w, s), "no form");
    // every row states 2; a direct-operator row may state 3, no other
    for (const emi::PassForm& f : emi::PASS_FORMS) EXPECT(emi::pass_form_max_res(f) == (f.dop ? 3 : 2), "form table");
}

// ---- the default by band (profiles/residency_notes.md) ---------------------------------------------------------------------------------
// the 6-state quadrotor at 1024 nodes, default options: {instances, residency, block order}: three resident workgroups per CU from 145 to
// 160 instances (MFMA workgroups first) and from 1009 to 2048 (at 1.1 x the even density), two everywhere else
const int DEFAULTS_1024[][3] = {{16, 2, 1},    {64, 2, 1},     {128, 2, 1},    {144, 2, 1},    {145, 3, 1},    {152, 3, 1},    {160, 3, 1},   {161, 2, 1},
                                {176, 2, 1},   {192, 2, 1},    {256, 2, 1},    {320, 2, 150},  {416, 2, 125},  {432, 2, 125},  {512, 2, 125}, {768, 2, 110},
                                {896, 2, 110}, {1008, 2, 110}, {1009, 3, 110}, {1024, 3, 110}, {1280, 3, 110}, {1536, 3, 110}, {1792, 3, 110}, {2048, 3, 110},
                                {4096, 2, 0}};
void check_defaults() {
    for (const auto& d : DEFAULTS_1024) {
        const Planned q = plan_of(context(6, 2, 1024), d[0]);
        EXPECT(q.p.one_launch == 1 && q.res == d[1] && q.p.block_order == d[2], "default at " + std::to_string(d[0]) + " instances");
        EXPECT(q.res != 3 || (q.dop && q.p.sw == 2 && q.p.k_tile == 16 && q.p.ksplit == 1), "default at " + std::to_string(d[0]) + " instances");
        // "sym_res" 2 gives the choice that was shipped with two: the order it was measured with, the operand source of its band
        PassPolicyIn two = context(6, 2, 1024);
        two.sym_res = 2;
        const Planned t = plan_of(two, d[0]);
        const int shipped_order = d[0] > 1535 && d[0] <= 2048 ? 0 : d[2];
        EXPECT(t.res == 2 && t.p.block_order == shipped_order && t.dop == (d[0] >= 417 && d[0] <= 2048), "two resident at " + std::to_string(d[0]) + " instances");
    }
    // a band states 3 only beside De / Do from L2, and only where "sym_res" is free to follow it
    for (const emi::PassBand& b : emi::PASS_BANDS)
        EXPECT(b.res == 2 || (b.res == 3 && b.dop == 2 && (b.needs & emi::BAND_FREE_RES)), "band table");
    // the 2-state model has no direct form: nothing it is asked makes it state 3
    for (int B : BATCHES) {
        PassPolicyIn in = context(2, 2, 1024);
        in.sym_res = 3, in.sym_dop = 2;
        EXPECT(plan_of(in, B).res == 2, "2-state model at " + std::to_string(B) + " instances");
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 6 && !std::strcmp(argv[1], "plan")) {
        PassPolicyIn in = context(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
        for (int i = 6; i < argc; ++i) {
            const char* eq = std::strchr(argv[i], '=');
            if (eq && std::string(argv[i], (size_t)(eq - argv[i])) == "np") {      // path rows: a defect row and two Jacobian rows each
                in.rows += 3 * std::atoi(eq + 1);
                continue;
            }
            const Option* hit = nullptr;
            for (const Option& o : NAMED)
                if (eq && std::string(argv[i], (size_t)(eq - argv[i])) == o.name) hit = &o;
            if (!hit) {
                std::fprintf(stderr, "unknown option: %s\n", argv[i]);
                return 2;
            }
            in.*(hit->field) = std::atoi(eq + 1);
        }
        print_plan(plan_of(in, std::atoi(argv[5])));
        return 0;
    }
    if (argc != 1) {
        std::fprintf(stderr, "usage: %s [plan NS NC M B [option=value ...]]\n", argv[0]);
        return 2;
    }
    const int cases = walk_grid();
    check_run_time_models();
    check_order();
    check_defaults();
    std::printf("pass residency: %d plans, %d failures\n", cases, failures);
    if (failures) return 1;
    std::printf("pass residency: ok\n");
    return 0;
}
