// emi_api_start.hip -- the starts of a context's whole batch behind the C ABI: emi_start_guess_dev / _host (kernels and workspace:
// emi_start_guess.hip; the route's host twin emi_plan_route: emi_host.cpp).
#include <hip/hip_runtime.h>

#include <cmath>

#include "emi_ctx.hpp"
#include "emi_plan_route.hpp"

using namespace emi_api;

namespace {

// what both forms refuse before anything is staged or launched
int start_check(emi_ctx_t c, const char* what, const emi_start_t* st, const void* X) {
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: f64 contexts only", what);
    EMI_TRY(ready(c));
    if (!st || !X || !st->xa || !st->xb) return fail(c, EMI_ERR_ARG, "%s: null argument", what);
    if (st->kind != EMI_START_LINE && st->kind != EMI_START_BEND && st->kind != EMI_START_PLANNED)
        return fail(c, EMI_ERR_ARG, "%s: unknown kind %d", what, st->kind);
    if (st->nsets != 1 && st->nsets != c->B) return fail(c, EMI_ERR_ARG, "%s: %d sets of end states (1 or the batch, %d)", what, st->nsets, c->B);
    if (st->grid != 0 && (st->grid < emi_plan::GRID_MIN || st->grid > emi_plan::GRID_MAX))
        return fail(c, EMI_ERR_ARG, "%s: grid %d (0, or %d .. %d)", what, st->grid, emi_plan::GRID_MIN, emi_plan::GRID_MAX);
    if (std::isnan(st->bend) || std::isnan(st->clearance)) return fail(c, EMI_ERR_ARG, "%s: bend or clearance is NaN", what);
    if (c->M < 2) return fail(c, EMI_ERR_ARG, "%s: a mesh of %d nodes", what, c->M);
    if (c->px < 0 || c->py < 0 || c->px >= c->ns || c->py >= c->ns)
        return fail(c, EMI_ERR_ARG, "%s: position states %d, %d of a model with %d states", what, c->px, c->py, c->ns);
    if (c->B > 65535) return fail(c, EMI_ERR_UNSUPPORTED, "%s: up to 65535 instances", what);
    return EMI_OK;
}

}  // namespace

extern "C" {

int emi_start_guess_dev(emi_ctx_t c, const emi_start_t* st, void* dX, void* dLevel) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(start_check(c, "emi_start_guess_dev", st, dX));
    HIP_TRY(c, hipSetDevice(c->device));
    EMI_TRY(emi::start_guess(c, *st, dX, dLevel));
    if (st->repair) EMI_TRY(emi_repair_guess_dev(c, dX));
    return EMI_OK;
}

int emi_start_guess_host(emi_ctx_t c, const emi_start_t* st, double* X, int* level) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(start_check(c, "emi_start_guess_host", st, X));
    HIP_TRY(c, hipSetDevice(c->device));
    HostStager s(c);
    void* dX = s.place(X, (size_t)c->B * c->ns * c->M * 8, false, true);
    void* dL = s.place(level, (size_t)c->B * 4, false, true);
    HOST_STAGED_TRY(s, emi_start_guess_dev(c, st, dX, dL))
    return s.finish();
}

}  // extern "C"
