// ode_delay_operator_main.cpp -- emi_ode_error_delay_operator (csrc/emi_host.cpp, host-only) as a stand-alone program for the host
// sanitizers (make check-ode-delay-operator): the output array is allocated at its exact size, so a write past 5 (M-1) M is
// reported; the rows sum to 1 (sums of absolute values stated), a delay of 0 gives emi_ode_error_operator's E, a delay that
// reaches before t0 gives e_0 at those points and a delay longer than the horizon at every point, bad arguments are refused.
#include <cmath>
#include <cstdio>
#include <vector>

#include "emi355x.h"

static int fail(const char* what, int M) {
    std::printf("ode_delay_operator_check: %s (M = %d)\n", what, M);
    return 1;
}

int main() {
    const double t0 = 0.25, tf = 3.0, T = tf - t0, h = T / 2.0;
    for (int M : {2, 3, 4, 9, 41, 130}) {
        std::vector<double> tau(M), w(M);
        if (emi_lgl(M, tau.data(), w.data(), nullptr) != EMI_OK) return fail("emi_lgl", M);
        const int np = 5 * (M - 1);
        std::vector<double> E((size_t)np * M), Ed((size_t)np * M), tq(np), Edel((size_t)np * M);
        if (emi_ode_error_operator(M, tau.data(), w.data(), E.data(), Ed.data(), tq.data()) != EMI_OK) return fail("plain operator", M);
        for (double frac : {0.0, 0.05, 0.3, 1.7}) {
            const double delay = frac * T;
            if (emi_ode_error_delay_operator(M, tau.data(), w.data(), t0, tf, delay, Edel.data()) != EMI_OK) return fail("status", M);
            for (int p = 0; p < np; ++p) {
                const double* row = Edel.data() + (size_t)p * M;
                double s = 0, a = 0;
                for (int j = 0; j < M; ++j) { s += row[j]; a += std::fabs(row[j]); }
                if (std::fabs(s - 1.0) > (M + 2) * 0x1p-52 * a) return fail("row sum", M);
                const double tp = t0 + h * (tq[p] + 1.0);
                if (tp - delay <= t0)
                    for (int j = 0; j < M; ++j)
                        if (row[j] != (j == 0 ? 1.0 : 0.0)) return fail("a time before t0 does not give e_0", M);
                if (frac >= 1.0 && row[0] != 1.0) return fail("a delay longer than the horizon leaves a row that is not e_0", M);
                // no delay: the abscissa goes through t_p and back, which moves it by a few ulp of 1
                if (frac == 0.0)
                    for (int j = 0; j < M; ++j)
                        if (std::fabs(row[j] - E[(size_t)p * M + j]) > 1e-9) return fail("delay 0 is not the interpolation operator", M);
            }
        }
        double* out = Edel.data();
        if (emi_ode_error_delay_operator(1, tau.data(), w.data(), t0, tf, 0.1, out) != EMI_ERR_ARG) return fail("M < 2 accepted", M);
        if (emi_ode_error_delay_operator(M, nullptr, w.data(), t0, tf, 0.1, out) != EMI_ERR_ARG) return fail("NULL accepted", M);
        if (emi_ode_error_delay_operator(M, tau.data(), nullptr, t0, tf, 0.1, out) != EMI_ERR_ARG) return fail("NULL accepted", M);
        if (emi_ode_error_delay_operator(M, tau.data(), w.data(), t0, tf, 0.1, nullptr) != EMI_ERR_ARG) return fail("NULL accepted", M);
        if (emi_ode_error_delay_operator(M, tau.data(), w.data(), tf, t0, 0.1, out) != EMI_ERR_ARG) return fail("tf <= t0 accepted", M);
        if (emi_ode_error_delay_operator(M, tau.data(), w.data(), t0, t0, 0.1, out) != EMI_ERR_ARG) return fail("tf == t0 accepted", M);
        if (emi_ode_error_delay_operator(M, tau.data(), w.data(), t0, tf, -0.1, out) != EMI_ERR_ARG) return fail("delay < 0 accepted", M);
    }
    std::printf("ode_delay_operator_check: ok\n");
    return 0;
}
