// param_table_plan_main.cpp -- what the launch policy of the evaluation pass (etol_amd/csrc/emi_pass_plan.hpp, host-only) makes of a
// context that holds a per-instance parameter table (PassPolicyIn::param_table), as a stand-alone program under the host sanitizers
// (`make check-param-table-plan`): no Python, no device.
//   (no argument)           over models, meshes, batches and the options that force a form: with a table the pass is never overlapped,
//                           nothing is planned as one launch, no pieces are cut and the report is the empty one of "overlap" 0; without
//                           one the input is the default-constructed one and the plan that of a context that never had a table
//   plan NS NC M B NP       print the plan of a built-in fp64 context with NP path rows, without and with a table, as one JSON object
// The contexts are those of tests/harness/pass_plan_main.cpp: a symmetric LGL mesh, built-in model.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "emi_pass_plan.hpp"

namespace {

using emi::PassPolicyIn;

PassPolicyIn context(int ns, int nc, int M, int np, bool f32 = false) {
    PassPolicyIn in;
    in.ns = ns;
    in.M = M;
    in.real_bytes = f32 ? 4 : 8;
    in.f32 = f32;
    in.rows = (ns + np) + ns * (ns + nc) + 2 * np + (ns + nc);
    in.model_class = emi::PASS_MODEL_BUILTIN;
    in.symmetric = !f32;
    in.has_dfrag = !f32 && M % 128 == 0;
    return in;
}

emi_pass_plan_t report(const PassPolicyIn& in, int B) {
    emi_pass_plan_t p;
    std::memset(&p, 0, sizeof p);
    emi::report_pass(in, B, &p);
    return p;
}

void print_plan(const char* key, const emi_pass_plan_t& p, const PassPolicyIn& in, const char* tail) {
    std::printf("\"%s\": {\"overlapped\": %d, \"one_launch\": %d, \"sw\": %d, \"ksplit\": %d, \"k_tile\": %d, \"column_tiles\": %d, \"store_mode\": %d, "
                "\"block_order\": %d, \"piece\": %d, \"tail\": %d, \"mfma_workgroups\": %d}%s",
                key, emi::pass_overlapped(in) ? 1 : 0, p.one_launch, p.sw, p.ksplit, p.k_tile, p.column_tiles, p.store_mode, p.block_order, p.piece, p.tail,
                p.mfma_workgroups, tail);
}

int fails = 0;
void expect(bool ok, const char* what, int ns, int M, int B, const char* opt, int v) {
    if (ok) return;
    ++fails;
    std::fprintf(stderr, "FAILED: %s (ns %d, M %d, B %d, %s=%d)\n", what, ns, M, B, opt, v);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 7 && !std::strcmp(argv[1], "plan")) {
        PassPolicyIn in = context(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[6]));
        const int B = std::atoi(argv[5]);
        std::printf("{");
        print_plan("shared", report(in, B), in, ", ");
        in.param_table = true;
        print_plan("table", report(in, B), in, "}\n");
        return 0;
    }
    if (argc != 1) {
        std::fprintf(stderr, "usage: %s [plan NS NC M B NP]\n", argv[0]);
        return 2;
    }
    struct Opt { const char* name; int PassPolicyIn::*field; int values[4]; };
    const Opt opts[] = {{"none", &PassPolicyIn::sym_ct, {0, 0, 0, 0}},           {"overlap_mode", &PassPolicyIn::overlap_mode, {1, 2, 3, 0}},
                        {"sym_ct", &PassPolicyIn::sym_ct, {3, 5, 6, 7}},         {"slice", &PassPolicyIn::slice, {16, 256, 1024, 0}},
                        {"sym_ksplit", &PassPolicyIn::sym_ksplit, {1, 2, 4, 8}}, {"small_rows", &PassPolicyIn::small_rows, {0, 24, 96, 24}}};
    const int models[][2] = {{2, 2}, {6, 2}, {12, 4}};
    const int meshes[] = {33, 50, 128, 256, 257, 1024, 4096};
    const int batches[] = {1, 3, 5, 7, 16, 64, 80, 112, 128, 256, 320, 512, 1024, 2049, 4096, 16384};
    emi_pass_plan_t empty;
    std::memset(&empty, 0, sizeof empty);
    long checked = 0;
    for (const auto& m : models)
        for (int M : meshes)
            for (int B : batches)
                for (const Opt& o : opts)
                    for (int v : o.values)
                        for (int f32 = 0; f32 < 2; ++f32) {
                            PassPolicyIn in = context(m[0], m[1], M, 3, f32 != 0);
                            in.*o.field = v;
                            PassPolicyIn off = in, tab = in, none = in;
                            tab.param_table = true;
                            none.allow_fused = 0;       // "overlap" 0: the route a context with a table takes
                            const emi_pass_plan_t pt = report(tab, B), pn = report(none, B), po = report(off, B);
                            expect(!emi::pass_overlapped(tab), "a context with a table is overlapped", m[0], M, B, o.name, v);
                            expect(!emi::pass_takes_small_batches(tab), "a context with a table takes the small-batch pass", m[0], M, B, o.name, v);
                            expect(!std::memcmp(&pt, &empty, sizeof pt), "the report of a context with a table is not the empty one", m[0], M, B, o.name, v);
                            expect(!std::memcmp(&pt, &pn, sizeof pt), "the report with a table differs from that of \"overlap\" 0", m[0], M, B, o.name, v);
                            expect(emi::store_mode_for(tab, B) == emi::store_mode_for(none, B), "store mode with a table differs from \"overlap\" 0", m[0], M, B,
                                   o.name, v);
                            // without a table: the flag's default is off, and the plan does not read it
                            expect(!off.param_table && !PassPolicyIn().param_table, "the flag is on by default", m[0], M, B, o.name, v);
                            // (under the default options, where tests/harness/pass_plan_main.cpp holds every point to one launch)
                            if (!std::strcmp(o.name, "none") && !f32 && m[0] <= 6 && M % 128 == 0 && M <= 1024)
                                expect(po.one_launch == 1, "a pass-eligible context without a table left the one-launch form", m[0], M, B, o.name, v);
                            ++checked;
                        }
    if (fails) return 1;
    std::printf("param table plan: ok (%ld contexts)\n", checked);
    return 0;
}
