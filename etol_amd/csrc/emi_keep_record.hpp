// emi_keep_record.hpp -- what a context remembers about the VALS buffer it last filled, for EMI_EVAL_KEEP_INVARIANT.
//
// The rows of VALS that the model declares invariant (emi_models.hpp: jac_varies / grad_varies) are functions of the mesh, the
// model parameters and the cost sign.  A pass may skip them only if the buffer it writes into already holds them for exactly the
// problem in force: this record says which buffer that is.  Host-only and free of the HIP runtime, so that its bookkeeping can be
// exercised by a stand-alone program under a host sanitizer (tests/harness/keep_record_main.cpp).
//
//   generation   bumped by every call that changes a value or the layout of VALS (mesh, model and its parameters, batch, path
//                table, tracks, delays, maximize sign): a record made under an older generation no longer matches
//   begin_pass   a pass starts; one that writes every row voids whatever the record said until the pass -- all its pieces -- is out
//   end_pass     ... and every piece was launched without an error: the buffer is primed
//   Passes that do not write the Jacobian (EMI_EVAL_NOJAC, defect only) leave the record alone.
#pragma once

namespace emi {

struct KeepRecord {
    const void* vals = nullptr;         // the buffer the last full Jacobian pass of this context wrote, whole batch; null: none
    unsigned long long vals_generation = 0;
    unsigned long long generation = 1;

    // one emi_eval_* call, all its pieces: whether it writes the Jacobian at all, and whether it may leave the invariant rows alone
    struct Pass { bool writes_jac = false, keep = false; };

    void bump() { ++generation; }
    void forget() { vals = nullptr; }
    bool matches(const void* dVALS) const { return dVALS != nullptr && vals == dVALS && vals_generation == generation; }
    // writes_jac: the pass stores Jacobian rows into dVALS; requested: the caller passed EMI_EVAL_KEEP_INVARIANT.  A pass that writes
    // everything voids the record at once: it is renewed by end_pass, when every piece is out
    Pass begin_pass(bool writes_jac, bool requested, const void* dVALS) {
        Pass p;
        p.writes_jac = writes_jac && dVALS != nullptr;
        p.keep = p.writes_jac && requested && matches(dVALS);
        if (p.writes_jac && !p.keep) forget();
        return p;
    }
    void end_pass(const Pass& p, const void* dVALS, bool ok) {
        if (!p.writes_jac || p.keep || !ok) return;
        vals = dVALS;
        vals_generation = generation;
    }
    // someone else wrote into [p, p + bytes): a record on a buffer that starts there is void (the context's own staging buffer)
    void written(const void* p) {
        if (p != nullptr && p == vals) forget();
    }
};

}  // namespace emi
