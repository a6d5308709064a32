// The life-cycle of a plan's resident factor: is there a factor, does it belong to the current values, and what was
// computed from it.  No HIP and no plan in here -- g++ alone compiles it (tools/factor_state_sanitize.cpp) -- and nothing outside
// this header assigns its members (tests/test_factor_state_host.py): the plan's files call the transitions and ask the predicates.
//
// Generations: factor_gen moves whenever the values or the resident factor change; fact_gen = factor_gen of the last factorization
// started, ok_gen = that of the last one that succeeded or of a replacement that did (-1: none), sel_gen = factor_gen the selected
// inverse was computed from, rf_anorm_gen = factor_gen the stored |A|_1 belongs to.  epoch is the flag value of the running
// factorization's fused steps and the key of the fingerprint cache: it moves with a factorization only, never with the values.
// Invariants: fact_gen <= factor_gen, ok_gen <= factor_gen, current() => usable(), epoch != 0 once a factorization has started;
// broken() => !usable() only while every factorization_enqueued belongs to a factorization_started, which a caller of the phase and
// segment entry points can break -- who must not take a half-rotated factor for one asks broken() as well.
#pragma once
#include <cstdint>

struct SfFactorState {
    bool values_set = false;
    int64_t factor_gen = 0, fact_gen = -1, ok_gen = -1, sel_gen = -1, rf_anorm_gen = -1;
    bool fact_done = false;         // the last factorization started has had all its launches enqueued
    bool upd_failed = false;        // a downdate left the factor half rotated
    int epoch = 0, hash_epoch = -1;
    int last_status = 0;            // what the last collect found (SF_OK = 0)

    // ---- transitions ----
    void values_changed() {         // the resident factor (and a selected inverse from it) no longer belongs to the values
        values_set = true;
        ++factor_gen;
    }
    void factorization_started() {
        epoch = (epoch == 0x7fffffff) ? 1 : epoch + 1;      // never 0: the flags are cleared to it
        fact_gen = ++factor_gen;
        upd_failed = false;
        fact_done = false;
    }
    void factorization_enqueued() { fact_done = true; }
    // the stream has been waited for and the info word read; a run whose launches are not all enqueued yet proves nothing
    int collected(int status) {
        last_status = status;
        if (status == 0 && fact_done) ok_gen = fact_gen;
        return status;
    }
    // the factor was written without a factorization (update, downdate, row modification, import): cached fingerprints and a
    // selected inverse are stale, and nothing is left for a collect to find -- it must not move ok_gen back to fact_gen.
    // !ok: half written, no factor until the next factorization starts or another replacement succeeds
    void factor_replaced(bool ok) {
        hash_epoch = -1;
        ++factor_gen;
        fact_done = false;
        ok_gen = ok ? factor_gen : -1;
        upd_failed = !ok;
    }
    void selinv_started() { sel_gen = -1; }
    void selinv_finished() { sel_gen = factor_gen; }
    void hashes_pending() { hash_epoch = -1; }
    void hashes_arrived() { hash_epoch = epoch; }
    void anorm_forgotten() { rf_anorm_gen = -1; }
    void anorm_computed() { rf_anorm_gen = factor_gen; }

    // ---- predicates (no device call: the two that may need a collect first say so, the driver's wrappers do it) ----
    bool has_values() const { return values_set; }
    // the last factorization started has succeeded, or a replacement since; NOT required: that it is one of the current values
    bool needs_collect_for_usable() const { return fact_done && ok_gen < fact_gen; }
    bool usable() const { return ok_gen >= 0 && ok_gen >= fact_gen; }
    // ... and nothing has changed since: the factor is the one of the current values
    bool needs_collect_for_current() const { return ok_gen != factor_gen && fact_gen == factor_gen; }
    bool current() const { return ok_gen == factor_gen; }
    bool broken() const { return upd_failed; }
    bool selinv_matches() const { return sel_gen == factor_gen; }
    bool hashes_current() const { return hash_epoch == epoch; }
    bool anorm_current() const { return rf_anorm_gen == factor_gen; }
    int64_t factor_generation() const { return factor_gen; }
    int factor_epoch() const { return epoch; }
};
