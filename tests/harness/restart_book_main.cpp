// restart_book_main.cpp -- stand-alone check of the bookkeeping of the ladder restarts (etol_amd/csrc/emi_restart_book.hpp over
// emi_refine_book.hpp), built with the host sanitizers (`make check-restart-book`).  It walks the two books through the calls
// ipm_solve_restart and LadderRun (emi_ipm_ladder.hip) make per attempt and per rung, without a device: the statuses, estimates and
// levels of every instance in every attempt are scripted.  Every case is printed as one JSON line (the script, then per attempt the
// pending list and per rung live / caller map / the two groups of retirees and who of them goes into the caller's arrays, then
// results, err and out), which tests/test_restart_cpu.py holds to the restated rule; the mixed case is also held here, to values
// worked out by hand.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "emi_restart_book.hpp"

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
constexpr int OK = EMI_IPM_CONVERGED, ACC = EMI_IPM_ACCEPTABLE, BAD = EMI_IPM_MAX_ITER, INF = EMI_IPM_INFEASIBLE;
constexpr int FAILED = 1 << EMI_REFINE_FAILED, FELL = 1 << EMI_REFINE_FELL_BACK;

struct Case {
    std::string name;
    int B, nrungs, first_check;                     // first_check < 0: never (the plain ladder)
    double tol;
    int A, retry_mask, drop;
    std::vector<std::vector<Ints>> status;          // [a][b][r]
    std::vector<std::vector<std::vector<double>>> err;
    std::vector<Ints> level;                        // [a][b]
};

struct Seen { Ints live, caller_map, here_from, here_to, older_from, older_to, sent_here, sent_older; bool has_caller_map; };
struct Attempt { Ints pending; std::vector<Seen> rungs; };

struct Walked {
    std::vector<Attempt> attempts;
    std::vector<emi_ipm_result_t> results;
    std::vector<double> err;
    std::vector<emi_ipm_restart_result_t> out;
};

Walked walk(const Case& k) {
    Walked w;
    const size_t all = (size_t)k.A * k.nrungs * k.B;
    w.results.resize(all); w.err.resize(all); w.out.resize(k.B);
    emi::RestartBook rb;
    rb.begin(k.B, k.A, k.nrungs, k.first_check < 0 ? emi::RefineBook::NEVER : k.first_check, k.retry_mask, w.results.data(), w.err.data(),
             w.out.data());
    for (int a = 0; a < k.A && !rb.done(); ++a) {
        emi::RefineBook book;
        rb.open(a, book);
        Attempt at;
        at.pending = rb.pending;
        EXPECT((int)rb.level.size() == rb.n());
        for (int i = 0; i < rb.n(); ++i) rb.level[i] = k.level[a][rb.pending[i]];
        for (int r = 0; r < k.nrungs && !book.done(); ++r) {
            const int n = book.n();
            Seen s;
            s.live = book.live;
            s.has_caller_map = book.caller_map() != nullptr;
            if (s.has_caller_map) s.caller_map.assign(book.caller_map(), book.caller_map() + n);
            EXPECT(r > 0 || book.row_map() == nullptr);         // the first batch of an attempt is placed, not prolonged
            std::vector<emi_ipm_result_t> res(n);
            std::vector<double> herr(n);
            for (int i = 0; i < n; ++i) {
                res[i] = emi_ipm_result_t{};
                res[i].status = k.status[a][book.live[i]][r];
                res[i].iterations = 100 * a + 10 * r + book.live[i];        // (something to recognise the record by)
                herr[i] = k.err[a][book.live[i]][r];
            }
            book.record_solve(r, res.data());
            const bool last = r + 1 == k.nrungs;
            if (book.checks(r)) book.decide(r, herr.data(), k.tol, last);
            else if (k.drop) book.drop_or_climb(r, last);
            else if (last) book.return_all(r);
            else book.climb_all();
            s.here_from = book.here.from; s.here_to = book.here.to; s.older_from = book.older.from; s.older_to = book.older.to;
            for (int b : book.here.to)
                if (rb.writes(a, book.verdict_of(b))) s.sent_here.push_back(b);
            for (int b : book.older.to)
                if (rb.writes(a, book.verdict_of(b))) s.sent_older.push_back(b);
            at.rungs.push_back(s);
        }
        EXPECT(book.done());
        rb.close(a, book);
        w.attempts.push_back(at);
    }
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
    std::printf("{\"case\":\"%s\",\"B\":%d,\"nrungs\":%d,\"first_check\":%d,\"tol\":%.17g,\"A\":%d,\"retry_mask\":%d,\"drop\":%d,\"status\":[",
                k.name.c_str(), k.B, k.nrungs, k.first_check, k.tol, k.A, k.retry_mask, k.drop);
    for (int a = 0; a < k.A; ++a) {
        std::printf("%s[", a ? "," : "");
        for (int b = 0; b < k.B; ++b) { std::printf("%s", b ? "," : ""); list(k.status[a][b]); }
        std::printf("]");
    }
    std::printf("],\"err\":[");
    for (int a = 0; a < k.A; ++a) {
        std::printf("%s[", a ? "," : "");
        for (int b = 0; b < k.B; ++b) {
            std::printf("%s[", b ? "," : "");
            for (int r = 0; r < k.nrungs; ++r) { std::printf("%s", r ? "," : ""); put(k.err[a][b][r]); }
            std::printf("]");
        }
        std::printf("]");
    }
    std::printf("],\"level\":[");
    for (int a = 0; a < k.A; ++a) { std::printf("%s", a ? "," : ""); list(k.level[a]); }
    std::printf("],\"attempts\":[");
    for (size_t a = 0; a < w.attempts.size(); ++a) {
        std::printf("%s{", a ? "," : "");
        put("pending", w.attempts[a].pending);
        std::printf("\"rungs\":[");
        for (size_t r = 0; r < w.attempts[a].rungs.size(); ++r) {
            const Seen& s = w.attempts[a].rungs[r];
            std::printf("%s{", r ? "," : "");
            put("live", s.live); put("caller_map", s.caller_map, !s.has_caller_map);
            put("here_from", s.here_from); put("here_to", s.here_to); put("older_from", s.older_from); put("older_to", s.older_to);
            put("sent_here", s.sent_here); put("sent_older", s.sent_older, false, "}");
        }
        std::printf("]}");
    }
    std::printf("],\"res_status\":[");
    for (size_t i = 0; i < w.results.size(); ++i) std::printf("%s%d", i ? "," : "", w.results[i].status);
    std::printf("],\"res_iterations\":[");
    for (size_t i = 0; i < w.results.size(); ++i) std::printf("%s%d", i ? "," : "", w.results[i].iterations);
    std::printf("],\"res_err\":[");
    for (size_t i = 0; i < w.err.size(); ++i) { std::printf("%s", i ? "," : ""); put(w.err[i]); }
    std::printf("],\"out\":[");
    for (int b = 0; b < k.B; ++b) {
        const emi_ipm_restart_result_t& o = w.out[b];
        std::printf("%s[%d,%d,%d,%d,%d,%d,", b ? "," : "", o.attempt, o.attempts, o.level, o.refine.rung, o.refine.verdict, o.refine.rungs_solved);
        put(o.refine.err);
        std::printf("]");
    }
    std::printf("]}\n");
}

// an attempt in which every instance has the same script
std::vector<Ints> all_run(int B, const Ints& s) { return std::vector<Ints>(B, s); }
std::vector<std::vector<double>> all_see(int B, const std::vector<double>& e) { return std::vector<std::vector<double>>(B, e); }

}  // namespace

int main() {
    const double tol = 1e-3, hi = 5e-3, lo = 5e-4;
    const std::vector<double> met{hi, lo, lo}, missed{hi, hi, hi};
    std::vector<Case> cases;
    cases.push_back({"everybody solved in attempt 0", 3, 3, 1, tol, 3, 0, 1,
                     {all_run(3, {OK, OK, OK}), all_run(3, {OK, OK, OK}), all_run(3, {OK, OK, OK})}, {all_see(3, met), all_see(3, met), all_see(3, met)},
                     {{0, 1, 2}, {-2, -2, -2}, {-2, -2, -2}}});
    cases.push_back({"everybody pending", 3, 3, 1, tol, 2, 0, 1,
                     {all_run(3, {BAD, OK, OK}), {{BAD, OK, OK}, {OK, BAD, OK}, {INF, OK, OK}}}, {all_see(3, met), all_see(3, met)},
                     {{-2, -2, -2}, {0, 0, -1}}});
    // three attempts over (r0, r1, r2) with the check from rung 1 on.  Attempt 0: instance 0 meets on rung 1; 1 drops on rung 0; 2 is
    // solved on rungs 0 and 1 and fails on rung 2 (falls back to rung 1: not retried); 3 fails on rung 1, the first checked rung (FAILED);
    // 4 drops on rung 0; 5 climbs to the end and misses.  Attempt 1 on {1, 3, 4}: 1 meets on rung 1, 3 drops on rung 0, 4 fails on rung 1.
    // Attempt 2 on {3, 4}: 3 meets on rung 2, 4 drops on rung 0 and is pending to the end
    const Case mixed{"mixed over three attempts", 6, 3, 1, tol, 3, 0, 1,
                     {{{OK, OK, OK}, {BAD, OK, OK}, {OK, ACC, BAD}, {OK, INF, OK}, {INF, OK, OK}, {ACC, OK, OK}},
                      {{OK, OK, OK}, {OK, OK, OK}, {OK, OK, OK}, {BAD, OK, OK}, {OK, BAD, OK}, {OK, OK, OK}},
                      {{OK, OK, OK}, {OK, OK, OK}, {OK, OK, OK}, {OK, OK, ACC}, {BAD, OK, OK}, {OK, OK, OK}}},
                     {{met, met, missed, met, met, missed}, all_see(6, met), {met, met, met, {hi, hi, lo}, met, met}},
                     {{-2, -2, -2, -2, -2, -2}, {0, 1, 2, 0, 1, 2}, {-2, -2, -2, -2, -2, -2}}};
    cases.push_back(mixed);
    cases.push_back({"a fall-back that is retried", 2, 3, 1, tol, 2, FAILED | FELL, 1,
                     {{{OK, OK, BAD}, {OK, OK, OK}}, {{OK, OK, OK}, {OK, OK, OK}}}, {{missed, met}, {{hi, hi, lo}, met}}, {{-2, -2}, {1, 1}}});
    cases.push_back({"the plain ladder with the drop", 4, 3, -1, tol, 2, 0, 1,
                     {{{OK, OK, OK}, {BAD, OK, OK}, {OK, BAD, OK}, {OK, OK, BAD}}, {{OK, OK, OK}, {OK, OK, ACC}, {OK, OK, BAD}, {BAD, OK, OK}}},
                     {all_see(4, met), all_see(4, met)}, {{-2, -2, -2, -2}, {0, 0, 0, 0}}});
    cases.push_back({"the plain ladder without the drop", 3, 2, -1, tol, 2, 0, 0,
                     {{{BAD, OK}, {OK, BAD}, {BAD, BAD}}, {{OK, OK}, {OK, OK}, {OK, BAD}}}, {all_see(3, {lo, lo}), all_see(3, {lo, lo})},
                     {{-2, -2, -2}, {0, 0, 0}}});
    cases.push_back({"without the drop below first_check", 3, 3, 1, tol, 2, 0, 0,
                     {{{BAD, OK, OK}, {BAD, BAD, OK}, {OK, OK, BAD}}, {{OK, OK, OK}, {OK, OK, OK}, {OK, OK, OK}}},
                     {{met, met, missed}, all_see(3, met)}, {{-2, -2, -2}, {-2, -2, -2}}});
    cases.push_back({"every verdict retried", 2, 2, 0, tol, 3, 15, 0, {all_run(2, {OK, OK}), all_run(2, {OK, OK}), all_run(2, {OK, OK})},
                     {all_see(2, {lo, lo}), all_see(2, {hi, hi}), all_see(2, {lo, lo})}, {{-2, -2}, {-2, -2}, {-2, -2}}});
    cases.push_back({"one instance", 1, 3, 1, tol, 3, 0, 1, {{{BAD, OK, OK}}, {{OK, INF, OK}}, {{OK, OK, OK}}}, {{met}, {met}, {missed}},
                     {{-2}, {2}, {-1}}});
    cases.push_back({"one instance, one rung, one attempt", 1, 1, -1, tol, 1, 0, 1, {{{BAD}}}, {{{hi}}}, {{-2}}});

    for (const Case& k : cases) print(k, walk(k));

    // the mixed case by hand
    const Walked w = walk(mixed);
    EXPECT(w.attempts.size() == 3);
    if (w.attempts.size() == 3) {
        const Attempt &a0 = w.attempts[0], &a1 = w.attempts[1], &a2 = w.attempts[2];
        const Ints none;
        EXPECT((a0.pending == Ints{0, 1, 2, 3, 4, 5}) && (a1.pending == Ints{1, 3, 4}) && (a2.pending == Ints{3, 4}));
        EXPECT(a0.rungs.size() == 3 && a1.rungs.size() == 2 && a2.rungs.size() == 3);
        if (a0.rungs.size() == 3 && a1.rungs.size() == 2 && a2.rungs.size() == 3) {
            EXPECT(!a0.rungs[0].has_caller_map && (a0.rungs[0].here_to == Ints{1, 4}) && (a0.rungs[0].sent_here == Ints{1, 4}));
            EXPECT((a0.rungs[1].live == Ints{0, 2, 3, 5}) && (a0.rungs[1].here_to == Ints{0, 3}) && (a0.rungs[1].here_from == Ints{0, 2}));
            EXPECT((a0.rungs[2].live == Ints{2, 5}) && (a0.rungs[2].here_to == Ints{5}) && (a0.rungs[2].older_to == Ints{2}) &&
                   (a0.rungs[2].older_from == Ints{1}));
            EXPECT((a1.rungs[0].caller_map == Ints{1, 3, 4}) && (a1.rungs[0].here_to == Ints{3}) && a1.rungs[0].sent_here == none);
            EXPECT((a1.rungs[1].live == Ints{1, 4}) && (a1.rungs[1].here_to == Ints{1, 4}) && (a1.rungs[1].sent_here == Ints{1}));
            EXPECT((a2.rungs[0].caller_map == Ints{3, 4}) && (a2.rungs[0].here_to == Ints{4}) && a2.rungs[0].sent_here == none);
            EXPECT((a2.rungs[2].live == Ints{3}) && (a2.rungs[2].here_to == Ints{3}) && (a2.rungs[2].sent_here == Ints{3}));
        }
    }
    const int attempt[6] = {0, 1, 0, 2, 0, 0}, attempts[6] = {1, 2, 1, 3, 3, 1}, level[6] = {-2, 1, -2, -2, -2, -2};
    const int rung[6] = {1, 1, 1, 2, 0, 2}, solved[6] = {2, 2, 3, 3, 1, 3};
    const int verdict[6] = {EMI_REFINE_MET, EMI_REFINE_MET, EMI_REFINE_FELL_BACK, EMI_REFINE_MET, EMI_REFINE_FAILED, EMI_REFINE_NOT_MET};
    for (int b = 0; b < 6; ++b) {
        const emi_ipm_restart_result_t& o = w.out[b];
        EXPECT(o.attempt == attempt[b] && o.attempts == attempts[b] && o.level == level[b]);
        EXPECT(o.refine.rung == rung[b] && o.refine.verdict == verdict[b] && o.refine.rungs_solved == solved[b]);
    }
    // (instance 4 was solved on rung 0 of every attempt and on rung 1 of attempt 1; instance 0 in attempt 0 only)
    const auto status_of = [&](int a, int r, int b) { return w.results[((size_t)a * 3 + r) * 6 + b].status; };
    EXPECT(status_of(0, 0, 4) == INF && status_of(0, 1, 4) == -1 && status_of(1, 0, 4) == OK && status_of(1, 1, 4) == BAD && status_of(1, 2, 4) == -1 &&
           status_of(2, 0, 4) == BAD && status_of(2, 1, 4) == -1);
    EXPECT(status_of(0, 1, 0) == OK && status_of(0, 2, 0) == -1 && status_of(1, 0, 0) == -1 && status_of(2, 0, 0) == -1);
    EXPECT(w.results[((size_t)1 * 3 + 1) * 6 + 4].iterations == 114);

    if (failures) {
        std::fprintf(stderr, "restart book: %d check(s) failed\n", failures);
        return EXIT_FAILURE;
    }
    std::puts("restart book: ok");
    return EXIT_SUCCESS;
}
