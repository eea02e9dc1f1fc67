// pass_plan_main.cpp -- the launch policy of the fp64 evaluation pass (etol_amd/csrc/emi_pass_plan.hpp, host-only) as a stand-alone
// program under the host sanitizers (`make check-pass-plan`): no Python, no device.
//   (no argument)                          walk the grid of tools/api_identity.py plan (its TILE_STEPS, INSTANCES, FORCED and DEFAULTS, for
//                                          the 2-state and the 6-state model at 128, 256 and 1024 nodes) and hold every one-launch plan to
//                                          the form table, the K loop, the grid size and the pieces
//   grid                                   print the complete plan of every grid point, one JSON object per line
//   plan NS NC M B [option=value ...]      print the plan of one context (np=N: with N path rows)
// The contexts are those tools/api_identity.py makes: a symmetric LGL mesh (so the fragment copy of De / Do exists), no path rows.
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
// FORCED of tools/api_identity.py, in its order
const std::vector<Option> FORCED = {
    {"sym_ct", &PassPolicyIn::sym_ct, {0, 1, 2, 3, 4, 5, 6, 7, 8}},
    {"sym_ksplit", &PassPolicyIn::sym_ksplit, {0, 1, 2, 4, 8}},
    {"sym_bk", &PassPolicyIn::sym_bk, {0, 8, 16}},
    {"sym_ctc", &PassPolicyIn::sym_ctc, {0, 1, 2}},
    {"sym_hs", &PassPolicyIn::sym_hs, {0, 1, 2}},
    {"sym_nst", &PassPolicyIn::sym_nst, {3, 4}},
    {"sym_cpart", &PassPolicyIn::sym_cpart, {-1, 0, 1, 2, 4, 8}},
    {"sym_gblk", &PassPolicyIn::sym_gblk, {0, 1, 2, 4, 8, 64}},
    {"pass_order", &PassPolicyIn::pass_order, {-1, 0, 1, 100, 125, 150}},
    {"node_store", &PassPolicyIn::node_store, {-1, 0, 1, 2, 3}},
    {"overlap_mode", &PassPolicyIn::overlap_mode, {0, 1, 2, 3}},
    {"slice", &PassPolicyIn::slice, {0, 16, 256, 1024}},
    {"sym_dop", &PassPolicyIn::sym_dop, {0, 1, 2}},
    {"sym_cx", &PassPolicyIn::sym_cx, {0, 1, 2}},
};
const int TILE_STEPS[] = {32, 48, 127, 143, 207, 383, 767, 1024};      // the last launch within each threshold; the first beyond follows it
const int INSTANCES[] = {1, 16, 64, 2048, 2049, 4096, 16384};
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

std::vector<int> batches(int M) {
    const int per = M / 128;
    std::vector<int> out(INSTANCES, INSTANCES + sizeof INSTANCES / sizeof *INSTANCES);
    for (int lo : TILE_STEPS) {
        out.push_back(16 * (lo / per));
        out.push_back(16 * (lo / per) + 1);
    }
    return out;
}

struct Planned {
    emi_pass_plan_t p;
    bool dop;
};
Planned plan_of(const PassPolicyIn& in, int B) {
    Planned q;
    std::memset(&q.p, 0, sizeof q.p);
    emi::report_pass(in, B, &q.p, &q.dop);
    return q;
}

void print_plan(const std::string& name, const Planned& q) {
    const emi_pass_plan_t& p = q.p;
    std::printf("{\"case\": \"%s\", \"one_launch\": %d, \"sw\": %d, \"ksplit\": %d, \"ring_stages\": %d, \"cpart\": %d, \"cx\": %d, \"mfma_workgroups\": %d, "
                "\"store_mode\": %d, \"block_order\": %d, \"tiles16\": %d, \"piece\": %d, \"tail\": %d, \"k_tile\": %d, \"column_tiles\": %d, \"k_halves\": %d, "
                "\"dop\": %d}\n",
                name.c_str(), p.one_launch, p.sw, p.ksplit, p.ring_stages, p.cpart, p.cx, p.mfma_workgroups, p.store_mode, p.block_order, p.tiles16, p.piece,
                p.tail, p.k_tile, p.column_tiles, p.k_halves, q.dop ? 1 : 0);
}

int failures = 0;
#define EXPECT(cond, name)                                                                    \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, (name).c_str(), #cond); \
            ++failures;                                                                       \
        }                                                                                     \
    } while (0)

void check_plan(const std::string& name, const PassPolicyIn& in, int B, const Planned& q) {
    const emi_pass_plan_t& p = q.p;
    // the pieces cover the batch exactly, and X of a launch stays below 4 GB (32-bit operand offsets of the MFMA role)
    const int first = p.piece > 0 ? p.piece : B;
    EXPECT(p.piece >= 0 && p.piece < B && p.tail >= 0 && (p.piece == 0 ? p.tail == 0 : (B / p.piece) * p.piece + p.tail == B), name);
    if (!p.one_launch) return;
    EXPECT((long long)first * in.ns * in.M * 8 < (1LL << 32), name);
    // a row of the form table holds exactly what is reported
    emi::PassShape s;
    s.ns = in.ns;
    s.M = in.M;
    s.model_class = in.model_class;
    s.has_dfrag = in.has_dfrag;
    s.store_mode = p.store_mode;
    const emi::PassForm* row = emi::find_form(s, p.sw, p.ksplit > 1, p.ring_stages, p.k_tile, p.column_tiles, p.k_halves, q.dop);
    EXPECT(row != nullptr && row >= emi::PASS_FORMS && row < emi::PASS_FORMS + emi::N_PASS_FORMS, name);
    // ... and resolving it once more changes nothing
    emi::PassWants w;
    w.sw = p.sw, w.ks = p.ksplit, w.nst = p.ring_stages, w.bk = p.k_tile, w.ct = p.column_tiles, w.hs = p.k_halves, w.dop = q.dop;
    EXPECT(emi::resolve_form(w, s).row == row, name);
    // the K loop: the slices divide the K tiles and leave each an even number of them, at least two
    const int nkt = (in.M / 2) / p.k_tile;
    EXPECT(p.ksplit >= 1 && nkt % p.ksplit == 0 && (p.ksplit == 1 || (nkt / p.ksplit >= 2 && (nkt / p.ksplit) % 2 == 0)), name);
    // the grid of the MFMA role: instance groups x column tiles x state groups x slices
    EXPECT(in.ns % p.sw == 0 && p.mfma_workgroups == ((first + 15) / 16) * ((in.M / 2) / (64 * p.column_tiles)) * (in.ns / p.sw) * p.ksplit, name);
    EXPECT(p.tiles16 == ((first + 15) / 16) * (in.M / 128), name);
}

template <class F>
void walk_grid(F&& visit) {
    for (const Model& m : MODELS)
        for (int M : MESHES) {
            const std::vector<int> bs = batches(M);
            auto run = [&](const PassPolicyIn& in, const std::string& opt) {
                for (int B : bs)
                    if (B >= 1) visit(std::string(m.name) + " M=" + std::to_string(M) + " " + opt + " B=" + std::to_string(B), in, B);
            };
            run(context(m.ns, m.nc, M), "None=None");
            for (const Option& o : FORCED)
                for (int v : o.values) {
                    PassPolicyIn in = context(m.ns, m.nc, M);
                    in.*(o.field) = v;
                    run(in, std::string(o.name) + "=" + std::to_string(v));
                }
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
            for (const Option& o : FORCED)
                if (eq && std::string(argv[i], (size_t)(eq - argv[i])) == o.name) hit = &o;
            if (!hit) {
                std::fprintf(stderr, "unknown option: %s\n", argv[i]);
                return 2;
            }
            in.*(hit->field) = std::atoi(eq + 1);
        }
        print_plan(argv[1], plan_of(in, std::atoi(argv[5])));
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "grid")) {
        walk_grid([](const std::string& name, const PassPolicyIn& in, int B) { print_plan(name, plan_of(in, B)); });
        return 0;
    }
    if (argc != 1) {
        std::fprintf(stderr, "usage: %s [grid | plan NS NC M B [option=value ...]]\n", argv[0]);
        return 2;
    }
    int cases = 0, one_launch = 0;
    walk_grid([&](const std::string& name, const PassPolicyIn& in, int B) {
        const Planned q = plan_of(in, B);
        check_plan(name, in, B, q);
        ++cases;
        one_launch += q.p.one_launch;
    });
    // every row of the table is a form of its own, and the run-time list lies within the built-in one's plain forms
    for (int i = 0; i < emi::N_PASS_FORMS; ++i)
        for (int j = 0; j < i; ++j) {
            const emi::PassForm &a = emi::PASS_FORMS[i], &b = emi::PASS_FORMS[j];
            EXPECT(!(a.cls == b.cls && a.nst == b.nst && a.bk == b.bk && a.ct == b.ct && a.hs == b.hs && a.dop == b.dop), std::string("form table"));
        }
    std::printf("pass plan: %d cases, %d as one launch, %d failures\n", cases, one_launch, failures);
    if (failures) return 1;
    std::printf("pass plan: ok\n");
    return 0;
}
