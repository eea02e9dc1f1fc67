// emi_refine_book.hpp -- who is where while a batch climbs a mesh ladder (emi_ipm_solve_ladder_*, emi_ipm_solve_refine_*).
//
// The driver (emi_ipm_ladder.hip: LadderRun) solves a compact batch of the live instances on every rung; an instance that retires
// hands its trajectory to the caller's arrays and the rest move up.  This object keeps the integers of that: who is live, where each
// live instance sat in the batch of the rung before, which retirees return which rung's iterate, and what the caller reads afterwards
// (results[r][b], err[r][b], out[b]).  The rule itself is emi_ipm_refine_decide.  Host-only and free of the HIP runtime, so that a
// stand-alone program can walk it under a host sanitizer with scripted statuses and estimates (tests/harness/refine_book_main.cpp).
//
//   begin          everybody is live; the caller's records say "never solved" until a rung writes them
//   keep           ... only the instances of a list are: a run that begins from a subset (a later attempt of emi_ipm_solve_restart_*)
//   record_solve   the results of a rung's solve, compact -> the caller's numbering
//   climb_all      a rung without a check: the next batch is this one
//   decide         a rung with a check: the estimates in, the two groups of retirees and the next batch out
//   return_all     the last rung of a run that never checks (the plain ladder): everybody returns this rung's iterate
//   drop_or_climb  a rung without a check under EMI_RESTART_DROP_FAILED: whoever was not solved leaves here, the rest climb or return
//   verdict_of     the verdict of an instance that has left; in a run that never checks, by the solve on the rung it ended on
//   row_map        where the rows of the next prolongation come from; null while nobody left the batch of the rung before
//   caller_map     the live instances in the caller's numbering; null while the batch is whole
#pragma once

#include <limits>
#include <vector>

#include "emi355x.h"

namespace emi {

struct RefineBook {
    static constexpr int NEVER = std::numeric_limits<int>::max();      // first_check of a run that checks on no rung
    // a group of retirees: entry i is instance from[i] of a compact batch and instance to[i] of the caller
    struct Moves { std::vector<int> from, to; };

    int B = 0, nrungs = 0, first_check = 0;
    int prev_n = 0;                     // the size of the batch pos refers to
    std::vector<int> live, pos;         // live: the caller's numbers, ascending; pos: where each sat in the batch of the rung before
    Moves here, older;                  // of the last decision: who returns that rung's iterate / the one of the rung before (from: its pos)
    emi_ipm_result_t* results = nullptr;            // [nrungs][B]
    double* err = nullptr;                          // [nrungs][B]
    emi_ipm_refine_result_t* out = nullptr;         // [B]

    void begin(int B_, int nrungs_, int first_check_, emi_ipm_result_t* results_, double* err_, emi_ipm_refine_result_t* out_) {
        B = B_; nrungs = nrungs_; first_check = first_check_; results = results_; err = err_; out = out_;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (size_t i = 0; i < (size_t)nrungs * B; ++i) {
            results[i] = emi_ipm_result_t{};
            results[i].status = -1;
            err[i] = nan;
        }
        live.resize(B); pos.resize(B);
        for (int b = 0; b < B; ++b) {
            out[b] = emi_ipm_refine_result_t{-1, EMI_REFINE_FAILED, 0, nan};
            live[b] = pos[b] = b;
        }
        prev_n = B;
        here = older = Moves{};
    }
    // the batch of the first rung is the instances who[0 .. n) (the caller's numbers, ascending) and not everybody
    void keep(const int* who, int n_) {
        live.assign(who, who + n_); pos.resize(n_);
        for (int i = 0; i < n_; ++i) pos[i] = i;
        prev_n = n_;
    }
    static bool solved(int status) { return status == EMI_IPM_CONVERGED || status == EMI_IPM_ACCEPTABLE; }
    int n() const { return (int)live.size(); }
    bool done() const { return live.empty(); }
    bool checks(int r) const { return r >= first_check; }
    // (both lists ascend without repeats: as long as the one they were taken from, they are 0, 1, ..)
    const int* row_map() const { return n() == prev_n ? nullptr : pos.data(); }
    const int* caller_map() const { return n() == B ? nullptr : live.data(); }

    void record_solve(int r, const emi_ipm_result_t* res) {
        for (int i = 0; i < n(); ++i) {
            results[(size_t)r * B + live[i]] = res[i];
            out[live[i]].rungs_solved = r + 1;
        }
    }
    void climb_all() {
        prev_n = n();
        for (int i = 0; i < prev_n; ++i) pos[i] = i;
        here = older = Moves{};
    }
    void return_all(int r) {
        here = older = Moves{};
        for (int i = 0; i < n(); ++i) {
            here.from.push_back(i); here.to.push_back(live[i]);
            out[live[i]].rung = r;
        }
        prev_n = n();
        live.clear(); pos.clear();
    }
    // The drop rule on rung r < first_check (where decide applies, it is that rule's "not ok, no good solution"): an instance whose
    // solve on r is neither converged nor acceptable has nothing good from an earlier rung either, and leaves on r with
    // EMI_REFINE_FAILED and what the solve left.  The rest climb; on the last rung of a run that never checks they return as in return_all
    void drop_or_climb(int r, bool last) {
        std::vector<int> next, next_pos;
        here = older = Moves{};
        for (int i = 0; i < n(); ++i) {
            const int b = live[i];
            if (!last && solved(results[(size_t)r * B + b].status)) {
                next.push_back(b); next_pos.push_back(i);
                continue;
            }
            here.from.push_back(i); here.to.push_back(b);
            out[b].rung = r;
        }
        prev_n = n();
        live.swap(next); pos.swap(next_pos);
    }
    int verdict_of(int b) const {
        if (first_check != NEVER || out[b].rung < 0) return out[b].verdict;
        return solved(results[(size_t)out[b].rung * B + b].status) ? EMI_REFINE_MET : EMI_REFINE_FAILED;
    }
    // herr [n]: the estimates of rung r in the order of the batch (the statuses are those of record_solve); last: r is the last
    // rung, which retires everybody
    void decide(int r, const double* herr, double ode_tol, bool last) {
        const bool has_good = r > first_check;          // whoever climbed from a checked rung was solved there
        std::vector<int> next, next_pos;
        here = older = Moves{};
        for (int i = 0; i < n(); ++i) {
            const int b = live[i];
            err[(size_t)r * B + b] = herr[i];
            int verdict = 0;
            if (!emi_ipm_refine_decide(results[(size_t)r * B + b].status, herr[i], ode_tol, has_good, last, &verdict)) {
                next.push_back(b); next_pos.push_back(i);
                continue;
            }
            const int k = verdict == EMI_REFINE_FELL_BACK ? 1 : 0;
            Moves& m = k ? older : here;
            m.from.push_back(k ? pos[i] : i); m.to.push_back(b);
            out[b].verdict = verdict;
            out[b].rung = r - k;
            out[b].err = err[(size_t)(r - k) * B + b];
        }
        prev_n = n();
        live.swap(next); pos.swap(next_pos);
    }
};

}  // namespace emi
