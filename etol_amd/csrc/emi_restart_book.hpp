// emi_restart_book.hpp -- who is still pending while a batch is re-run from one start after another (emi_ipm_solve_restart_*).
//
// The driver (emi_ipm_ladder.hip: ipm_solve_restart) runs the rung loop (LadderRun, with its RefineBook) once per attempt, on the
// instances that no earlier attempt gave a verdict outside retry_mask.  This object keeps the integers of that: who is pending, which
// attempt owns an instance's trajectory in the caller's arrays, and the per-attempt blocks of what the caller reads afterwards
// (results[a][r][b], err[a][r][b], out[b]).  The rule itself is emi_ipm_restart_decide.  Host-only and free of the HIP runtime, so
// that a stand-alone program can walk it under a host sanitizer with scripted statuses and estimates
// (tests/harness/restart_book_main.cpp).
//
//   begin          everybody is pending; every block of the caller's records says "never solved"
//   open           the RefineBook of attempt a: its records are block a, its batch of the first rung is the pending list
//   writes         whether a retiree of attempt a goes into the caller's arrays: everybody in attempt 0 (what a pending instance
//                  keeps to the end), later only who leaves with a verdict outside retry_mask
//   close          after the rung loop of attempt a: out[b] of who was solved in it, and the pending list of the next attempt
#pragma once

#include <limits>
#include <vector>

#include "emi355x.h"
#include "emi_refine_book.hpp"

namespace emi {

struct RestartBook {
    static constexpr int MAX_ATTEMPTS = 8;
    static constexpr int NO_LEVEL = -2;             // emi_plan_route's "nothing to plan": every start but PLANNED, and dX0

    int B = 0, A = 0, nrungs = 0, first_check = 0, retry_mask = 0;
    std::vector<int> pending;                       // the caller's numbers, ascending
    std::vector<int> level;                         // [pending.size()]: emi_start_guess_dev's of the present attempt, in that order
    std::vector<emi_ipm_refine_result_t> refine;    // [B]: the RefineBook's out of the present attempt
    emi_ipm_result_t* results = nullptr;            // [A][nrungs][B]
    double* err = nullptr;                          // [A][nrungs][B]
    emi_ipm_restart_result_t* out = nullptr;        // [B]

    // first_check_: RefineBook::NEVER for the plain ladder
    void begin(int B_, int A_, int nrungs_, int first_check_, int retry_mask_, emi_ipm_result_t* results_, double* err_,
               emi_ipm_restart_result_t* out_) {
        B = B_; A = A_; nrungs = nrungs_; first_check = first_check_; retry_mask = retry_mask_; results = results_; err = err_; out = out_;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (size_t i = 0; i < (size_t)A * nrungs * B; ++i) {
            results[i] = emi_ipm_result_t{};
            results[i].status = -1;
            err[i] = nan;
        }
        pending.resize(B); refine.resize(B);
        for (int b = 0; b < B; ++b) {
            pending[b] = b;
            out[b] = emi_ipm_restart_result_t{0, 0, NO_LEVEL, emi_ipm_refine_result_t{-1, EMI_REFINE_FAILED, 0, nan}};
        }
    }
    int n() const { return (int)pending.size(); }
    bool done() const { return pending.empty(); }
    size_t block(int a) const { return (size_t)a * nrungs * B; }

    void open(int a, RefineBook& book) {
        book.begin(B, nrungs, first_check, results + block(a), err + block(a), refine.data());
        book.keep(pending.data(), n());
        level.assign(n(), NO_LEVEL);
    }
    bool writes(int a, int verdict) const { return a == 0 || !emi_ipm_restart_decide(verdict, retry_mask); }
    void close(int a, const RefineBook& book) {
        std::vector<int> next;
        for (int i = 0; i < n(); ++i) {
            const int b = pending[i];
            const int verdict = book.verdict_of(b);
            const bool again = emi_ipm_restart_decide(verdict, retry_mask) != 0;
            out[b].attempts = a + 1;
            if (a == 0 || !again) {                 // (a == 0: what an instance that stays pending to the end reports)
                out[b].attempt = a;
                out[b].level = level[i];
                out[b].refine = refine[b];
                out[b].refine.verdict = verdict;
            }
            if (again) next.push_back(b);
        }
        pending.swap(next);
    }
};

}  // namespace emi
