// refine_book_main.cpp -- stand-alone check of the bookkeeping of the lock-step ladder and refinement (etol_amd/csrc/emi_refine_book.hpp),
// built with the host sanitizers (`make check-refine-book`).  It walks the book through the calls LadderRun (emi_ipm_ladder.hip) makes
// per rung, without a device: the statuses and estimates of every instance on every rung are scripted.  Every case is printed as one
// JSON line (the script, then per rung live / pos / the two maps / the two groups of retirees, then results, err and out), which
// tests/test_refine_book_cpu.py holds to the restated rule; the base case is also held here, to values worked out by hand.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "emi_refine_book.hpp"

namespace {

int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

using Ints = std::vector<int>;
const double NaN = std::numeric_limits<double>::quiet_NaN();
constexpr int OK = EMI_IPM_CONVERGED, ACC = EMI_IPM_ACCEPTABLE, BAD = EMI_IPM_MAX_ITER;

struct Case {
    std::string name;
    int B, nrungs, first_check;         // first_check < 0: never
    double tol;
    std::vector<Ints> status;           // [b][r]
    std::vector<std::vector<double>> err;
};

// what the driver saw of the book on one rung, before and after the rung's decision
struct Seen { Ints live, pos, row_map, caller_map, here_from, here_to, older_from, older_to; bool has_row_map, has_caller_map; };

struct Walked {
    std::vector<Seen> rungs;
    std::vector<emi_ipm_result_t> results;
    std::vector<double> err;
    std::vector<emi_ipm_refine_result_t> out;
};

Walked walk(const Case& k) {
    Walked w;
    w.results.resize((size_t)k.nrungs * k.B); w.err.resize((size_t)k.nrungs * k.B); w.out.resize(k.B);
    emi::RefineBook book;
    book.begin(k.B, k.nrungs, k.first_check < 0 ? emi::RefineBook::NEVER : k.first_check, w.results.data(), w.err.data(), w.out.data());
    for (int r = 0; r < k.nrungs && !book.done(); ++r) {
        const int n = book.n();
        Seen s;
        s.live = book.live; s.pos = book.pos;
        s.has_row_map = book.row_map() != nullptr; s.has_caller_map = book.caller_map() != nullptr;
        if (s.has_row_map) s.row_map.assign(book.row_map(), book.row_map() + n);
        if (s.has_caller_map) s.caller_map.assign(book.caller_map(), book.caller_map() + n);
        std::vector<emi_ipm_result_t> res(n);
        std::vector<double> herr(n);
        for (int i = 0; i < n; ++i) {
            res[i] = emi_ipm_result_t{};
            res[i].status = k.status[book.live[i]][r];
            res[i].iterations = 10 * r + book.live[i];          // (something to recognise the record by)
            herr[i] = k.err[book.live[i]][r];
        }
        book.record_solve(r, res.data());
        const bool last = r + 1 == k.nrungs;
        if (book.checks(r)) book.decide(r, herr.data(), k.tol, last);
        else if (last) book.return_all(r);
        else book.climb_all();
        s.here_from = book.here.from; s.here_to = book.here.to; s.older_from = book.older.from; s.older_to = book.older.to;
        w.rungs.push_back(s);
    }
    EXPECT(book.done() || (int)w.rungs.size() == k.nrungs);
    return w;
}

void list(const Ints& v) {
    std::printf("[");
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? "," : "", v[i]);
    std::printf("]");
}
void put(const char* key, const Ints& v, bool null = false, const char* end = ",") {
    std::printf("\"%s\":", key);
    if (null) std::printf("null");
    else list(v);
    std::printf("%s", end);
}
void put(double v) {          // (as Python's json reads them)
    if (std::isnan(v)) std::printf("NaN");
    else if (std::isinf(v)) std::printf(v > 0 ? "Infinity" : "-Infinity");
    else std::printf("%.17g", v);
}

void print(const Case& k, const Walked& w) {
    std::printf("{\"case\":\"%s\",\"B\":%d,\"nrungs\":%d,\"first_check\":%d,\"tol\":%.17g,\"status\":[", k.name.c_str(), k.B, k.nrungs, k.first_check, k.tol);
    for (int b = 0; b < k.B; ++b) { std::printf("%s", b ? "," : ""); list(k.status[b]); }
    std::printf("],\"err\":[");
    for (int b = 0; b < k.B; ++b) {
        std::printf("%s[", b ? "," : "");
        for (int r = 0; r < k.nrungs; ++r) { std::printf("%s", r ? "," : ""); put(k.err[b][r]); }
        std::printf("]");
    }
    std::printf("],\"rungs\":[");
    for (size_t r = 0; r < w.rungs.size(); ++r) {
        const Seen& s = w.rungs[r];
        std::printf("%s{", r ? "," : "");
        put("live", s.live); put("pos", s.pos); put("row_map", s.row_map, !s.has_row_map); put("caller_map", s.caller_map, !s.has_caller_map);
        put("here_from", s.here_from); put("here_to", s.here_to); put("older_from", s.older_from); put("older_to", s.older_to, false, "}");
    }
    std::printf("],\"res_status\":[");
    for (size_t i = 0; i < w.results.size(); ++i) std::printf("%s%d", i ? "," : "", w.results[i].status);
    std::printf("],\"res_iterations\":[");
    for (size_t i = 0; i < w.results.size(); ++i) std::printf("%s%d", i ? "," : "", w.results[i].iterations);
    std::printf("],\"res_err\":[");
    for (size_t i = 0; i < w.err.size(); ++i) { std::printf("%s", i ? "," : ""); put(w.err[i]); }
    std::printf("],\"out\":[");
    for (int b = 0; b < k.B; ++b) {
        std::printf("%s[%d,%d,%d,", b ? "," : "", w.out[b].rung, w.out[b].verdict, w.out[b].rungs_solved);
        put(w.out[b].err);
        std::printf("]");
    }
    std::printf("]}\n");
}

}  // namespace

int main() {
    const double tol = 1e-3, hi = 5e-3, lo = 5e-4;
    std::vector<Case> cases;
    // instance 0 meets the tolerance on rung 1, 1 ends unsolved there (nothing good yet), 2 ends unsolved on rung 2 (falls back to rung 1),
    // 3 climbs to the last rung and misses, 4 meets on rung 3
    const Case base{"base", 5, 4, 1, tol,
                    {{OK, OK, OK, OK}, {OK, BAD, OK, OK}, {OK, ACC, BAD, OK}, {ACC, OK, OK, OK}, {OK, OK, ACC, OK}},
                    {{hi, lo, lo, lo}, {hi, lo, lo, lo}, {hi, hi, lo, lo}, {hi, hi, 4e-3, 2e-3}, {hi, hi, 4e-3, 9e-4}}};
    cases.push_back(base);
    cases.push_back({"all retire on rung 1", 3, 4, 1, tol, {{OK, OK, OK, OK}, {OK, BAD, OK, OK}, {BAD, ACC, OK, OK}},
                     {{hi, lo, lo, lo}, {hi, lo, lo, lo}, {hi, tol, lo, lo}}});
    cases.push_back({"first_check 0", 4, 3, 0, tol, {{OK, OK, OK}, {BAD, OK, OK}, {OK, BAD, OK}, {OK, OK, BAD}},
                     {{lo, lo, lo}, {lo, lo, lo}, {hi, lo, lo}, {hi, hi, lo}}});
    cases.push_back({"a NaN estimate", 3, 3, 1, tol, {{OK, OK, OK}, {OK, OK, OK}, {OK, OK, BAD}},
                     {{hi, NaN, lo}, {hi, lo, lo}, {hi, std::numeric_limits<double>::infinity(), NaN}}});
    cases.push_back({"never", 4, 3, -1, tol, {{OK, OK, OK}, {BAD, BAD, BAD}, {OK, BAD, OK}, {ACC, OK, OK}},
                     {{lo, lo, lo}, {lo, lo, lo}, {lo, lo, lo}, {lo, lo, lo}}});
    cases.push_back({"one instance", 1, 3, 1, tol, {{OK, OK, OK}}, {{hi, hi, lo}}});
    cases.push_back({"one instance, one rung, never", 1, 1, -1, tol, {{BAD}}, {{hi}}});

    for (const Case& k : cases) print(k, walk(k));

    // the base case by hand
    const Walked w = walk(base);
    EXPECT(w.rungs.size() == 4);
    if (w.rungs.size() == 4) {
        const Seen &r0 = w.rungs[0], &r1 = w.rungs[1], &r2 = w.rungs[2], &r3 = w.rungs[3];
        const Ints all{0, 1, 2, 3, 4}, none;
        EXPECT(r0.live == all && r0.pos == all && !r0.has_row_map && !r0.has_caller_map);
        EXPECT(r0.here_from == none && r0.here_to == none && r0.older_from == none && r0.older_to == none);
        EXPECT(r1.live == all && r1.pos == all && !r1.has_row_map && !r1.has_caller_map);
        EXPECT((r1.here_from == Ints{0, 1}) && (r1.here_to == Ints{0, 1}) && r1.older_from == none && r1.older_to == none);
        EXPECT((r2.live == Ints{2, 3, 4}) && (r2.pos == Ints{2, 3, 4}) && r2.row_map == r2.pos && r2.caller_map == r2.live);
        EXPECT(r2.here_from == none && r2.here_to == none && (r2.older_from == Ints{2}) && (r2.older_to == Ints{2}));
        EXPECT((r3.live == Ints{3, 4}) && (r3.pos == Ints{1, 2}) && r3.row_map == r3.pos && r3.caller_map == r3.live);
        EXPECT((r3.here_from == Ints{0, 1}) && (r3.here_to == Ints{3, 4}) && r3.older_from == none && r3.older_to == none);
    }
    const int rung[5] = {1, 1, 1, 3, 3}, verdict[5] = {EMI_REFINE_MET, EMI_REFINE_FAILED, EMI_REFINE_FELL_BACK, EMI_REFINE_NOT_MET, EMI_REFINE_MET};
    const int solved[5] = {2, 2, 3, 4, 4};
    for (int b = 0; b < 5; ++b) {
        EXPECT(w.out[b].rung == rung[b] && w.out[b].verdict == verdict[b] && w.out[b].rungs_solved == solved[b]);
        EXPECT(w.out[b].err == base.err[b][rung[b]]);
        for (int r = 0; r < 4; ++r) {
            const emi_ipm_result_t& q = w.results[(size_t)r * 5 + b];
            const double e = w.err[(size_t)r * 5 + b];
            if (r < solved[b]) EXPECT(q.status == base.status[b][r] && q.iterations == 10 * r + b);
            else EXPECT(q.status == -1 && q.iterations == 0 && q.cost == 0.0);
            if (r >= 1 && r < solved[b]) EXPECT(e == base.err[b][r]);
            else EXPECT(std::isnan(e));
        }
    }

    if (failures) {
        std::fprintf(stderr, "refine book: %d check(s) failed\n", failures);
        return EXIT_FAILURE;
    }
    std::puts("refine book: ok");
    return EXIT_SUCCESS;
}
