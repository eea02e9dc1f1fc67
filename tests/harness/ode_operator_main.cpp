// ode_operator_main.cpp -- emi_ode_error_operator (csrc/emi_host.cpp, host-only) as a stand-alone program for the host sanitizers
// (make check-ode-operator): every output array is allocated at its exact size, so a write past 5 (M-1) M or 5 (M-1) is reported;
// the rows of E must sum to 1, those of E' to 0, the points lie inside their intervals, bad arguments are refused.
#include <cmath>
#include <cstdio>
#include <vector>

#include "emi355x.h"

static int fail(const char* what, int M) {
    std::printf("ode_operator_check: %s (M = %d)\n", what, M);
    return 1;
}

int main() {
    for (int M : {2, 3, 4, 9, 41, 130}) {
        std::vector<double> tau(M), w(M);
        if (emi_lgl(M, tau.data(), w.data(), nullptr) != EMI_OK) return fail("emi_lgl", M);
        const int np = 5 * (M - 1);
        std::vector<double> E((size_t)np * M), Ed((size_t)np * M), tq(np);
        if (emi_ode_error_operator(M, tau.data(), w.data(), E.data(), Ed.data(), tq.data()) != EMI_OK) return fail("status", M);
        for (int p = 0; p < np; ++p) {
            const int k = p % (M - 1);
            if (!(tq[p] > tau[k] && tq[p] < tau[k + 1])) return fail("point outside its interval", M);
            double s = 0, sd = 0, ad = 0;
            for (int j = 0; j < M; ++j) { s += E[(size_t)p * M + j]; sd += Ed[(size_t)p * M + j]; ad += std::fabs(Ed[(size_t)p * M + j]); }
            if (std::fabs(s - 1.0) > M * 0x1p-52 || std::fabs(sd) > M * 0x1p-52 * ad) return fail("row sums", M);
        }
        if (emi_ode_error_operator(1, tau.data(), w.data(), E.data(), Ed.data(), tq.data()) != EMI_ERR_ARG) return fail("M < 2 accepted", M);
        if (emi_ode_error_operator(M, tau.data(), nullptr, E.data(), Ed.data(), tq.data()) != EMI_ERR_ARG) return fail("NULL accepted", M);
    }
    std::printf("ode_operator_check: ok\n");
    return 0;
}
