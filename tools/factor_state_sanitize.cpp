// The life-cycle of a plan's factor (csrc/sf_factor_state.h) without a device, under ASan + UBSan
// (tests/test_factor_state_host.py): named scenarios with every predicate after every step, then every sequence of up to 7
// transitions against the rules as they stood before the header existed -- the loose members of the plan and the assignments that
// were spread over its files, written out again below -- and the invariants over the same sequences.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "sf_factor_state.h"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "factor_state_sanitize: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

namespace {

// ---- the old rules, field by field ----
struct Old {
    bool values_set = false;
    int64_t factor_gen = 0, fact_gen = -1, ok_gen = -1, sel_gen = -1, rf_anorm_gen = -1;
    bool fact_done = false, upd_failed = false;
    int epoch = 0, hash_epoch = -1, last_status = 0;
    void set_values() { values_set = true; ++factor_gen; }                      // the three set_values paths
    void run_launches_first() {                                                 // and the graph replay, which then set fact_done
        epoch = (epoch == 0x7fffffff) ? 1 : epoch + 1;
        fact_gen = ++factor_gen;
        upd_failed = false;
        fact_done = false;
    }
    void run_launches_last() { fact_done = true; }
    void sync(int status) {
        last_status = status;
        if (last_status == 0 && fact_done) ok_gen = fact_gen;
    }
    void updown_commit(bool failed) {       // the import was its success branch (it also cleared upd_failed) without the fact_done line
        hash_epoch = -1;
        ++factor_gen;
        fact_done = false;
        if (failed) { upd_failed = true; ok_gen = -1; return; }
        ok_gen = factor_gen;
        upd_failed = false;
    }
    void selinv_run_begin() { sel_gen = -1; }
    void selinv_run_end() { sel_gen = factor_gen; }
    void hashes_begin() { hash_epoch = -1; }
    void hashes_end() { hash_epoch = epoch; }
    void refine_setup() { rf_anorm_gen = -1; }
    void refine_anorm() { rf_anorm_gen = factor_gen; }
    bool usable_needs_sync() const { return fact_done && ok_gen < fact_gen; }                       // sf_factor_usable
    bool usable() const { return ok_gen >= 0 && ok_gen >= fact_gen; }
    bool current_needs_sync() const { return ok_gen != factor_gen && fact_gen == factor_gen; }      // sf_selinv_factor_current
    bool current() const { return ok_gen == factor_gen; }
};

constexpr int NT = 13;      // transitions with their argument values
void apply(SfFactorState& s, Old& o, int t) {
    switch (t) {
        case 0: s.values_changed(); o.set_values(); break;
        case 1: s.factorization_started(); o.run_launches_first(); break;
        case 2: s.factorization_enqueued(); o.run_launches_last(); break;
        case 3: s.collected(0); o.sync(0); break;
        case 4: s.collected(2); o.sync(2); break;
        case 5: s.factor_replaced(true); o.updown_commit(false); break;
        case 6: s.factor_replaced(false); o.updown_commit(true); break;
        case 7: s.selinv_started(); o.selinv_run_begin(); break;
        case 8: s.selinv_finished(); o.selinv_run_end(); break;
        case 9: s.hashes_pending(); o.hashes_begin(); break;
        case 10: s.hashes_arrived(); o.hashes_end(); break;
        case 11: s.anorm_forgotten(); o.refine_setup(); break;
        case 12: s.anorm_computed(); o.refine_anorm(); break;
    }
}

// what the walk remembers of a sequence: a factorization has started at all; one is open (started, the factor not replaced since);
// factorization_enqueued came without one -- a caller ran the last launches of a factorization it never began
struct Seen { bool started = false, open = false, orphan = false; };

void compare(const SfFactorState& s, const Old& o, const Seen& seen) {
    REQUIRE(s.values_set == o.values_set && s.factor_gen == o.factor_gen && s.fact_gen == o.fact_gen && s.ok_gen == o.ok_gen);
    REQUIRE(s.sel_gen == o.sel_gen && s.rf_anorm_gen == o.rf_anorm_gen && s.fact_done == o.fact_done && s.upd_failed == o.upd_failed);
    REQUIRE(s.epoch == o.epoch && s.hash_epoch == o.hash_epoch && s.last_status == o.last_status);
    REQUIRE(s.has_values() == o.values_set && s.broken() == o.upd_failed && s.factor_generation() == o.factor_gen);
    REQUIRE(s.needs_collect_for_usable() == o.usable_needs_sync() && s.usable() == o.usable());
    REQUIRE(s.needs_collect_for_current() == o.current_needs_sync() && s.current() == o.current());
    REQUIRE(s.selinv_matches() == (o.sel_gen == o.factor_gen) && s.hashes_current() == (o.hash_epoch == o.epoch));
    REQUIRE(s.anorm_current() == (o.rf_anorm_gen == o.factor_gen) && s.factor_epoch() == o.epoch);
    // the invariants
    REQUIRE(s.fact_gen <= s.factor_gen && s.ok_gen <= s.factor_gen);
    REQUIRE(!s.current() || s.usable());
    REQUIRE(!seen.started || s.epoch != 0);
    // broken() => !usable() holds as long as every factorization_enqueued belongs to a factorization_started.  The entry points
    // do not promise that (sf_chol_plan_factorize_phase(p, 1) on its own, scenarios()), so the callers that must not take a
    // half-rotated factor for one keep asking broken() as well
    REQUIRE(seen.orphan || !s.broken() || !s.usable());
}

long walk(const SfFactorState& s, const Old& o, const Seen& seen, int depth) {
    long count = 1;
    compare(s, o, seen);
    if (depth == 0) return count;
    for (int t = 0; t < NT; ++t) {
        SfFactorState s1 = s;
        Old o1 = o;
        apply(s1, o1, t);
        Seen n = seen;
        if (t == 1) n.started = n.open = true;
        if (t == 5 || t == 6) n.open = false;
        if (t == 2 && !n.open) n.orphan = true;
        count += walk(s1, o1, n, depth - 1);
    }
    return count;
}

// usable, current, broken, selinv_matches
void expect(const SfFactorState& s, bool usable, bool current, bool broken, bool sel) {
    REQUIRE(s.usable() == usable && s.current() == current && s.broken() == broken && s.selinv_matches() == sel);
}

void scenarios() {
    SfFactorState s;
    expect(s, false, false, false, false);                  // a fresh plan
    REQUIRE(!s.has_values() && !s.needs_collect_for_usable() && !s.needs_collect_for_current());
    s.values_changed();
    expect(s, false, false, false, false);
    s.factorization_started();
    expect(s, false, false, false, false);
    REQUIRE(!s.needs_collect_for_usable() && s.needs_collect_for_current() && s.factor_epoch() == 1 && !s.hashes_current());
    s.factorization_enqueued();
    REQUIRE(s.needs_collect_for_usable() && s.needs_collect_for_current());
    REQUIRE(s.collected(0) == 0);
    expect(s, true, true, false, false);
    REQUIRE(!s.needs_collect_for_usable() && !s.needs_collect_for_current());
    s.hashes_pending(); REQUIRE(!s.hashes_current());
    s.hashes_arrived(); REQUIRE(s.hashes_current());
    s.anorm_computed(); REQUIRE(s.anorm_current());
    s.selinv_started();
    expect(s, true, true, false, false);
    s.selinv_finished();
    expect(s, true, true, false, true);
    s.values_changed();                                     // the factor stays usable, nothing else belongs to the values any more
    expect(s, true, false, false, false);
    REQUIRE(!s.anorm_current() && s.hashes_current() && !s.needs_collect_for_current());
    s.factorization_started(); s.factorization_enqueued();
    REQUIRE(s.collected(2) == 2);                           // collected with a failure
    expect(s, false, false, false, false);
    REQUIRE(s.last_status == 2 && !s.hashes_current());

    SfFactorState seg;                                      // a segment-driven run collected before its last launch is enqueued
    seg.values_changed(); seg.factorization_started();
    seg.collected(0);
    REQUIRE(seg.ok_gen == -1);
    expect(seg, false, false, false, false);
    seg.factorization_enqueued(); seg.collected(0);
    expect(seg, true, true, false, false);

    SfFactorState u = seg;                                  // a replaced factor is not moved back by a collect
    u.factor_replaced(true);
    const int64_t g = u.ok_gen;
    REQUIRE(g == u.factor_generation() && !u.hashes_current());
    u.collected(0);
    REQUIRE(u.ok_gen == g);
    expect(u, true, true, false, false);
    u.factor_replaced(false);                               // a failed downdate
    expect(u, false, false, true, false);
    u.factorization_started();
    expect(u, false, false, false, false);
    u.factorization_enqueued();
    expect(u, false, false, false, false);
    u.collected(0);
    expect(u, true, true, false, false);

    SfFactorState imp;                                      // an import on a plan whose own factorization nobody collected
    imp.values_changed(); imp.factorization_started(); imp.factorization_enqueued();
    imp.factor_replaced(true);
    expect(imp, true, true, false, false);
    REQUIRE(!imp.needs_collect_for_usable() && !imp.needs_collect_for_current());
    imp.collected(0);                                       // (without the fact_done rule ok_gen would go back to fact_gen here)
    expect(imp, true, true, false, false);

    SfFactorState half = seg;                               // the last launches of a factorization nobody started, after a failed
    half.factor_replaced(false);                            // downdate: the collect takes them for the end of the one before it
    half.factorization_enqueued(); half.collected(0);
    REQUIRE(half.broken() && half.usable());

    SfFactorState w;                                        // the epoch wraps past 0
    w.epoch = 0x7fffffff;
    w.factorization_started();
    REQUIRE(w.factor_epoch() == 1);
}

}  // namespace

int main() {
    scenarios();
    const long states = walk(SfFactorState(), Old(), Seen(), 7);
    SfFactorState top;                                      // the same walk from the last epoch before the wrap
    Old otop;
    top.epoch = otop.epoch = 0x7ffffffe;
    walk(top, otop, Seen{true, false, false}, 4);
    printf("factor_state_sanitize: ok (%ld states)\n", states);
    return 0;
}
