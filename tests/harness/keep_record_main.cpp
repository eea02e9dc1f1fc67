// keep_record_main.cpp -- stand-alone check of the record behind EMI_EVAL_KEEP_INVARIANT (etol_amd/csrc/emi_keep_record.hpp), built
// with the host sanitizers (`make check-keep-record`).  It replays, without a device, the sequences emi_eval_dev / emi_eval_host
// (emi_api_pass.hip) and the setters of emi_api.hip put the record through; the buffers are host allocations that stand for device addresses.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "emi_keep_record.hpp"

namespace {

int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// one emi_eval_dev call in `pieces` launches, the launch `fail_at` (if any) returning an error: whether it ran as a KEEP pass
bool eval(emi::KeepRecord& r, const void* vals, bool nodes, bool nojac, bool flag, int pieces = 1, int fail_at = -1) {
    const emi::KeepRecord::Pass p = r.begin_pass(nodes && !nojac, flag, vals);
    bool ok = true;
    for (int i = 0; i < pieces && ok; ++i) {
        // a piece of a pass that writes everything runs with the record void: nothing may rely on it half way
        if (p.writes_jac && !p.keep) EXPECT(!r.matches(vals));
        ok = i != fail_at;
    }
    r.end_pass(p, vals, ok);
    return p.keep;
}

}  // namespace

int main() {
    std::vector<double> a(64), b(64);
    emi::KeepRecord r;

    // nothing written yet: the flag is ignored, the pass primes the buffer, the next one keeps
    EXPECT(!eval(r, a.data(), true, false, true));
    EXPECT(eval(r, a.data(), true, false, true));
    EXPECT(!eval(r, a.data(), true, false, false));         // not asked for: writes everything (and stays primed)
    EXPECT(eval(r, a.data(), true, false, true));
    // values-only and defect-only passes leave the record alone, whatever the flag
    EXPECT(!eval(r, a.data(), true, true, true));
    EXPECT(!eval(r, nullptr, true, true, true));
    EXPECT(!eval(r, a.data(), false, false, true));
    EXPECT(eval(r, a.data(), true, false, true));
    // another buffer: full pass there, and the record moves with it
    EXPECT(!eval(r, b.data(), true, false, true));
    EXPECT(!eval(r, a.data(), true, false, true));
    EXPECT(eval(r, a.data(), true, false, true));
    // every setter bumps the generation: the next pass writes everything, once
    for (int i = 0; i < 7; ++i) {
        r.bump();
        EXPECT(!r.matches(a.data()));
        EXPECT(!eval(r, a.data(), true, false, true));
        EXPECT(eval(r, a.data(), true, false, true));
    }
    // a batch in pieces counts only when every piece is out
    r.bump();
    EXPECT(!eval(r, a.data(), true, false, true, 4, 2));
    EXPECT(!r.matches(a.data()));
    EXPECT(!eval(r, a.data(), true, false, true, 4));
    EXPECT(eval(r, a.data(), true, false, true, 4));
    // a KEEP pass that fails does not touch the invariant rows: the record stands
    EXPECT(eval(r, a.data(), true, false, true, 4, 1));
    EXPECT(r.matches(a.data()));
    // the staging buffer of the host forms: overwritten by an upload, or grown (freed and allocated anew, maybe at the same address)
    r.written(b.data());
    EXPECT(r.matches(a.data()));
    r.written(a.data());
    EXPECT(!eval(r, a.data(), true, false, true));
    {
        std::unique_ptr<double[]> s(new double[16]);
        EXPECT(!eval(r, s.get(), true, false, true));
        EXPECT(eval(r, s.get(), true, false, true));
        r.written(s.get());                                  // (ensure_vals_staging tells the record BEFORE the old buffer goes)
    }
    std::unique_ptr<double[]> s2(new double[32]);
    EXPECT(!eval(r, s2.get(), true, false, true));
    r.written(nullptr);
    EXPECT(eval(r, s2.get(), true, false, true));
    // a null VALS never matches and never primes
    emi::KeepRecord z;
    EXPECT(!eval(z, nullptr, true, false, true));
    EXPECT(!z.matches(nullptr));

    if (failures) {
        std::fprintf(stderr, "keep record: %d check(s) failed\n", failures);
        return EXIT_FAILURE;
    }
    std::puts("keep record: ok");
    return EXIT_SUCCESS;
}
