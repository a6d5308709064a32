// The schedule builder (csrc/sf_schedule.cpp) on a CPU: builds the schedules of a list of small plans -- in core, mapped over
// several ranks, out of core, Cholesky and LU -- and checks every index the kernels will follow against bounds computed from the
// input and the panel layout alone; then one malformed input per SF_ERR_ARG exit that an input can reach.  No GPU, no HIP:
// tests/test_schedule_host.py builds this file with sf_schedule.cpp and sf_symbolic.cpp under ASan + UBSan.  Prints
// "schedule_sanitize: ok" and returns 0.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "sf_schedule.h"
#include "sf_symbolic.h"

using sf::Long;

static int g_fail = 0;
static std::string g_case;
#define CHECK(cond)                                                                                           \
    do {                                                                                                      \
        if (!(cond) && ++g_fail <= 20) printf("FAIL %s: %s (line %d)\n", g_case.c_str(), #cond, __LINE__);     \
    } while (0)

// ---- matrices: the 7-point Laplacian on a g^3 grid, lower triangle by column; and a whole matrix with an unsymmetric pattern ----
struct Csc { Long n; std::vector<Long> p, i; std::vector<double> x; };
static Csc stencil(Long g, bool whole_unsymmetric) {
    Csc A;
    A.n = g * g * g;
    A.p.push_back(0);
    for (Long z = 0; z < g; ++z) for (Long y = 0; y < g; ++y) for (Long x = 0; x < g; ++x) {
        const Long j = x + g * (y + g * z);
        auto put = [&](Long i, double v) { A.i.push_back(i); A.x.push_back(v); };
        if (whole_unsymmetric) {        // entries above the diagonal, some dropped: the pattern of U differs from L's
            if (z > 0 && j % 5 != 0) put(j - g * g, -1.0);
            if (y > 0) put(j - g, -1.0);
            if (x > 0 && j % 3 != 0) put(j - 1, -1.0);
        }
        put(j, 6.5);
        if (x + 1 < g) put(j + 1, -1.0);
        if (y + 1 < g) put(j + g, -1.0);
        if (z + 1 < g) put(j + g * g, -1.0);
        A.p.push_back((Long)A.i.size());
    }
    return A;
}

static void analyze(Long g, bool lu, bool unsym, sf::Symbolic& S) {
    const Csc A = stencil(g, unsym);
    std::vector<Long> perm((size_t)A.n);
    int rc = sf::grid_nd_perm(g, g, g, 3, 1, perm.data());
    if (!rc) rc = lu ? sf::analyze_lu(A.n, A.p.data(), A.i.data(), A.x.data(), perm.data(), (size_t)1 << 30, !unsym, S)
                     : sf::analyze_cholesky(A.n, A.p.data(), A.i.data(), A.x.data(), perm.data(), (size_t)1 << 30, S);
    if (rc) { printf("FAIL: analysis of %lld^3 returned %d\n", (long long)g, rc); exit(1); }
}

static PlanInput input_of(const sf::Symbolic& S) {
    PlanInput in;
    in.dry = true;
    in.lu = S.lu; in.n = S.n; in.nsuper = S.nsuper;
    in.Super = S.Super.data(); in.SuperMap = S.SuperMap.data(); in.Lsip = S.Lsip.data(); in.Lsi = S.Lsi.data(); in.Lsxp = S.Lsxp.data();
    in.Lp = S.Lp.data(); in.Li = S.Li.data();
    if (S.lu && !S.symmetric) { in.Up = S.Up.data(); in.Ui = S.Ui.data(); }
    return in;
}

struct Built { SfSchedule s; sf::DlSchedule dl; Layout lay; PlanTables T; int rc = 0, stage = 0; };
// the three steps as plan_create runs them; stage = the one that refused (1 arguments, 2 layout, 3 the rest)
static void build(const PlanInput& in, const PlanKnobs& kn, Built& b) {
    b.stage = 1; if ((b.rc = sf_schedule_check_arguments(in))) return;
    b.stage = 2; if ((b.rc = sf_schedule_layout(in, b.s, b.lay))) return;
    b.stage = 3; if ((b.rc = sf_schedule_build(in, kn, b.s, b.dl, b.lay, b.T))) return;
    b.stage = 0;
}

// ---- the checks of one good schedule.  cover[e] counts how often host entry e of the factor is downloaded (over all ranks) ----
static void check_schedule(const PlanInput& in, const Built& b, std::vector<int>& cover) {
    const SfSchedule& p = b.s;
    const PlanTables& T = b.T;
    const Layout& lay = b.lay;
    const int64_t xC = lay.XP[(size_t)in.nsuper], R = in.sides() * xC, isize = in.Lsip[in.nsuper];
    CHECK(lay.ushift == xC && p.xC == xC && (int64_t)lay.XP.size() == in.nsuper + 1);
    for (sf_long s = 0; s < in.nsuper; ++s) CHECK(lay.XP[s] == -1 || (lay.XP[s] >= 0 && lay.XP[s] + in.nscol(s) * in.nsrow(s) <= xC));
    // a task's panel: the supernode of its first column, stored here, at the L or the U^T place; its extents inside the panel
    auto sn_of = [&](int32_t first_col) -> sf_long { return (first_col >= 0 && first_col < in.n) ? in.SuperMap[first_col] : -1; };
    auto panel_ok = [&](int64_t off, sf_long s, int32_t ld) {
        return s >= 0 && in.Super[s] >= 0 && lay.XP[s] >= 0 && ld == in.nsrow(s) && (off == lay.XP[s] || (in.lu && off == lay.XP[s] + xC));
    };
    auto block_ok = [&](sf_long s, int diag, int b_, int row0, int nrows) {
        return diag >= 0 && b_ >= 1 && diag + b_ <= in.nscol(s) && row0 >= 0 && nrows >= 0 && row0 + nrows <= in.nsrow(s);
    };
    for (const PotrfTask& t : T.potrf) {
        const sf_long s = sn_of(t.first_col);
        CHECK(panel_ok(t.panel, s, t.ld) && t.panel == lay.XP[s] && t.first_col == in.Super[s] && block_ok(s, t.diag, t.b, 0, 0) && t.b <= sf::NB);
    }
    for (const TrsmTask& t : T.trsm) {
        const sf_long s = sn_of(t.first_col);
        CHECK(panel_ok(t.panel, s, t.ld) && panel_ok(t.dpanel, s, t.ld) && t.first_col == in.Super[s]);
        CHECK(s >= 0 && block_ok(s, t.diag, t.b, t.row0, t.nrows) && t.b <= sf::NB && t.row0 >= t.diag + t.b && t.nrows >= 1 && t.nrows <= sf::TRSM_ROWS);
        CHECK(s >= 0 && (in.lu ? (t.panel != t.dpanel && (t.unit == 1) == (t.panel == lay.XP[s] + xC)) : (t.panel == t.dpanel && t.unit == 0)));
    }
    for (const StepTask& t : T.steps) {
        const sf_long s = sn_of(t.first_col);
        CHECK(panel_ok(t.panel, s, t.ld) && panel_ok(t.xpanel, s, t.ld) && t.first_col == in.Super[s]);
        CHECK(s >= 0 && block_ok(s, t.diag, t.b, t.row0, t.nrows) && t.b <= sf::NB && t.J >= 0 && t.J <= t.diag && t.row0 >= t.diag && t.nrows >= 1 &&
              t.nrows <= sf::ST_ROWS);
        CHECK((t.flag == -1 && (t.mode & 2)) || (t.flag >= 0 && t.flag < T.n_flags && t.flag < p.n_flags));
        CHECK(s >= 0 && t.slot >= 0 && t.slot < std::max<int64_t>(T.max_diag_tasks, 1) && t.next_b >= 0 && t.row0 + t.next_b <= in.nsrow(s) &&
              (t.next_b == 0 || t.row0 + t.next_b <= in.nscol(s)));
    }
    // GEMM problems, by the kind of the launch that runs them
    auto prob_ok = [&](const GemmProb& g, bool scatter) {
        bool ok = g.M >= 1 && g.N >= 1 && g.K >= 1 && g.lda >= 1 && g.ldc >= 1 && g.y_off >= 0 && g.x_off >= 0 && g.c_off >= 0;
        ok = ok && g.y_off + (g.M - 1) + (int64_t)(g.K - 1) * g.lda < R && g.x_off + (g.N - 1) + (int64_t)(g.K - 1) * g.lda < R;
        if (!scatter) return ok && g.c_off + (g.M - 1) + (int64_t)(g.N - 1) * g.ldc < R;
        const sf_long a = sn_of(g.tgt_first_col);
        ok = ok && a >= 0 && lay.XP[a] >= 0 && (g.c_off == lay.XP[a] || (in.lu && g.c_off == lay.XP[a] + xC)) && g.ldc == in.nsrow(a);
        ok = ok && g.tgt_nscol == in.nscol(a) && g.tgt_nbelow == in.nsrow(a) - in.nscol(a) && g.tgt_rows == in.Lsip[a] + in.nscol(a);
        ok = ok && g.src_rows >= 0 && g.src_rows + g.M <= isize && g.N <= g.M;
        return ok && g.map_off >= 0 && g.map_off + g.M <= T.relmap_size;
    };
    int64_t tickets_seen = 0;
    for (const Launch& L : p.launches) {
        CHECK(L.first >= 0 && L.count >= 0);
        const int64_t end = L.first + L.count;
        if (L.kind == LAUNCH_POTRF) CHECK(end <= (int64_t)T.potrf.size() && L.count > 0);
        else if (L.kind == LAUNCH_TRSM) CHECK(end <= (int64_t)T.trsm.size() && L.count > 0);
        else if (L.kind == LAUNCH_STEP) { CHECK(end <= (int64_t)T.steps.size() && L.count > 0 && L.ticket >= 0 && L.ticket < p.n_tickets); tickets_seen += 1; }
        else if (L.kind == LAUNCH_OOC_GROUP) CHECK(in.ooc() && L.first < in.ooc_ngroups && L.count == 0);
        else if (L.kind == LAUNCH_UPDATE_SMALL) {
            CHECK(end <= (int64_t)T.stasks.size() && L.count > 0);
            for (int64_t k = L.first; k < end && k < (int64_t)T.stasks.size(); ++k) {
                const GemmTask& t = T.stasks[(size_t)k];
                CHECK(t.prob >= 0 && t.prob < (int32_t)T.probs.size());
                if (t.prob < 0 || t.prob >= (int32_t)T.probs.size()) continue;
                const GemmProb& g = T.probs[(size_t)t.prob];
                CHECK(prob_ok(g, true) && t.tm * sf::SU_TM < g.M && t.tn * sf::SU_TN < g.N);
            }
        } else {
            CHECK(launch_is_gemm(L.kind) && end <= (int64_t)T.gtasks.size() && L.count > 0);
            CHECK(L.ticket >= 0 && L.ticket + 8 <= p.n_tickets);
            tickets_seen += 8;
            // the K-step prefix: count + 1 entries, from 0, never falling, ending at `units`
            CHECK(L.prefix_first >= 0 && L.prefix_first + L.count + 1 <= (int64_t)T.ktprefix.size());
            if (!launch_is_gemm(L.kind) || end > (int64_t)T.gtasks.size() || L.prefix_first + L.count + 1 > (int64_t)T.ktprefix.size()) continue;
            const uint32_t* pre = T.ktprefix.data() + L.prefix_first;
            CHECK(pre[0] == 0 && pre[L.count] == L.units);
            for (int k = 0; k < L.count; ++k) {
                const GemmTask& t = T.gtasks[(size_t)(L.first + k)];
                CHECK(pre[k] <= pre[k + 1] && pre[k + 1] - pre[k] == t.nkt);
                CHECK(t.prob >= 0 && t.prob < (int32_t)T.probs.size());
                if (t.prob < 0 || t.prob >= (int32_t)T.probs.size()) continue;
                const GemmProb& g = T.probs[(size_t)t.prob];
                CHECK(prob_ok(g, L.kind == LAUNCH_GEMM_SCATTER));
                CHECK(t.tm * sf::GEMM_BM < g.M && t.tn * sf::GEMM_BN < g.N && t.nkt >= 1 &&
                      (int64_t)t.kt0 + t.nkt <= (g.K + sf::GEMM_BK - 1) / sf::GEMM_BK);
            }
        }
    }
    CHECK(tickets_seen == p.n_tickets && p.launch_split <= p.launches.size());
    for (const Segment& sg : p.segments) {
        CHECK(sg.l0 <= sg.l1 && sg.l1 <= p.launches.size() && sg.off.size() == sg.cnt.size() && sg.src.size() == sg.off.size());
        int64_t packed = 0;
        for (size_t k = 0; k < sg.off.size(); ++k) {
            CHECK(sg.off[k] >= 0 && sg.cnt[k] >= 1 && sg.off[k] + sg.cnt[k] <= R);
            CHECK(sg.src[k] >= sg.off[k] && sg.src[k] + (sg.cols[k] - 1) * sg.ld[k] + sg.rows[k] <= sg.off[k] + sg.cnt[k]);
            packed += sg.rows[k] * sg.cols[k];
        }
        CHECK(packed == sg.packed);
    }
    // out of core: what a group's first launch zeroes and masks
    for (const auto& zs : p.ooc_zero)
        for (const auto& z : zs) CHECK(z.first >= 0 && z.second >= 1 && z.first + z.second <= xC);
    if (in.ooc()) CHECK((int64_t)T.loadmask.size() == (int64_t)(in.ooc_ngroups + 1) * std::max<sf_long>(in.nsuper, 1));
    else CHECK(T.loadmask.empty() == !p.partial);
    // the solve's tasks and its sync block: [info | n_solve_sync words | 3 ticket words per step]
    const int64_t words = 1 + (int64_t)p.n_solve_sync + 3 * (int64_t)p.solve_steps.size();
    CHECK((int64_t)p.solve_sync_words() == words);
    for (const sf::SolveTask& t : T.solve) {
        const sf_long s = sn_of(t.first_col);
        CHECK(s >= 0 && lay.XP[s] >= 0 && t.panel == lay.XP[s] && t.rows == in.Lsip[s] && t.ld == in.nsrow(s) && t.first_col == in.Super[s]);
        CHECK(s >= 0 && block_ok(s, t.diag, t.b, t.row0, t.nrows) && t.b <= std::max(sf::SV_B, (int)in.nscol(s)) && (t.nrows == 0 || t.row0 >= t.diag + t.b));
        CHECK(t.flag >= 0 && t.flag < p.n_solve_sync && 1 + t.flag < words && t.expect >= 0);
        CHECK(t.tdiag == 0 || (t.tdiag >= 1 && t.tdiag - 1 + (int64_t)t.b * t.b <= T.solveT_size));
    }
    for (int64_t k : T.solveT_list) CHECK(k >= 0 && k < (int64_t)T.solve.size());
    for (size_t k = 0; k < p.solve_steps.size(); ++k) {
        const auto& st = p.solve_steps[k];
        CHECK(st.fwd_first >= 0 && st.fwd_first + st.fwd_count <= (int64_t)T.solve.size() && st.bwd_first >= 0 && st.bwd_first + st.count <= (int64_t)T.solve.size());
        CHECK(st.ndiag >= 0 && st.ndiag <= st.count && st.ndiag <= st.fwd_count && st.nrows_tasks >= 0 && st.nrows_tasks + st.ndiag <= st.count);
        CHECK(st.red_first >= 0 && st.red_count >= 0 && st.red_first + st.red_count <= (int)p.solve_reduces.size());
        CHECK(1 + (int64_t)p.n_solve_sync + 3 * (int64_t)k + 2 < words);
    }
    for (const auto& r : p.solve_reduces) CHECK(r.off >= 0 && r.cnt >= 1 && r.off + r.cnt <= in.n);
    // the download: every piece inside the panels on the device, its events and fill tiles in range; its host entries counted
    CHECK(b.dl.lu_direct ? b.dl.fill_first.size() == b.dl.ev_ready.size() + 1 : T.fill_tiles.empty());
    if (!b.dl.fill_first.empty()) CHECK(b.dl.fill_first.front() == 0 && b.dl.fill_first.back() == (int64_t)T.fill_tiles.size());
    for (const sf::FillTile& f : T.fill_tiles) CHECK(f.xp >= 0 && f.xp + (int64_t)f.nsrow * f.ce <= xC && f.r0 >= 0 && f.r0 <= f.c0 && f.cb <= f.ce && f.c0 < f.ce && f.ce <= f.nsrow);
    auto mark = [&](int64_t lo, int64_t len) {
        CHECK(lo >= 0 && len >= 0 && lo + len <= (int64_t)cover.size());
        for (int64_t e = std::max<int64_t>(lo, 0); e < std::min<int64_t>(lo + len, (int64_t)cover.size()); ++e) ++cover[(size_t)e];
    };
    size_t last_ready = 0;
    for (const DlPiece& pc : b.dl.pieces) {
        CHECK(pc.ev >= 0 && (size_t)pc.ev < b.dl.ev_ready.size() && pc.ready >= last_ready && pc.ready <= p.launches.size() && pc.count >= 1);
        if (pc.ev >= 0 && (size_t)pc.ev < b.dl.ev_ready.size()) CHECK(b.dl.ev_ready[(size_t)pc.ev] == pc.ready);
        last_ready = pc.ready;
        CHECK(in.ooc() ? (pc.group >= -1 && pc.group < in.ooc_ngroups) : pc.group == -1);
        if (pc.s0 >= 0) {                   // LU, direct form: both panels' runs
            CHECK(in.lu && pc.s1 > pc.s0 && pc.s1 <= in.nsuper && pc.dev_off >= 0 && pc.dev_count >= 1 && pc.dev_off + pc.dev_count <= xC);
            if (pc.ld > 0) {
                const int64_t hld = 2 * in.nsrow(pc.s0) - in.nscol(pc.s0);
                CHECK(pc.s1 == pc.s0 + 1 && pc.ld == in.nsrow(pc.s0) && pc.j0 >= 0 && pc.j0 + pc.ncols <= in.nscol(pc.s0) && pc.dev_off == lay.XP[pc.s0] + pc.j0 * pc.ld &&
                      pc.dev_count == pc.ncols * pc.ld && pc.count == pc.ncols * hld);
                mark(in.Lsxp[pc.s0] + pc.j0 * hld, pc.ncols * hld);
            } else {
                CHECK(pc.dev_off == lay.XP[pc.s0] && pc.count == in.Lsxp[pc.s1] - in.Lsxp[pc.s0]);
                mark(in.Lsxp[pc.s0], in.Lsxp[pc.s1] - in.Lsxp[pc.s0]);
            }
        } else if (pc.ld > 0) {             // Cholesky block column right of the first: rows [skip, ld) cross, the rest is zero-filled
            CHECK(!in.lu && pc.skip >= 0 && pc.skip < pc.ld && pc.ncols >= 1 && pc.count == pc.ncols * (pc.ld - pc.skip));
            CHECK(pc.dev_off >= 0 && pc.dev_off + pc.ncols * pc.ld <= xC);
            mark(pc.host_off, pc.ncols * pc.ld);
        } else {
            if (!in.lu) CHECK(pc.dev_off >= 0 && pc.dev_off + pc.count <= xC);
            mark(pc.host_off, pc.count);
        }
    }
    for (int64_t c : b.dl.group_pieces) CHECK(c >= 0);
}

// every host entry of the supernodes `stored` marks must have been downloaded exactly once
static void check_cover(const PlanInput& in, const std::vector<int>& cover, const std::vector<char>& stored) {
    for (sf_long s = 0; s < in.nsuper; ++s)
        for (int64_t e = in.Lsxp[s]; e < in.Lsxp[s + 1]; ++e) CHECK(cover[(size_t)e] == (stored[(size_t)s] ? 1 : 0));
}

static void good_whole(const std::string& name, const sf::Symbolic& S, const PlanKnobs& kn) {
    g_case = name;
    const PlanInput in = input_of(S);
    Built b;
    build(in, kn, b);
    CHECK(b.rc == SF_OK);
    if (b.rc) return;
    CHECK(b.s.u_alias == (S.lu && S.symmetric));
    std::vector<int> cover((size_t)S.Lsxp[(size_t)S.nsuper], 0);
    check_schedule(in, b, cover);
    check_cover(in, cover, std::vector<char>((size_t)S.nsuper, 1));
    printf("%-40s %zu launches, %zu solve steps, %zu pieces\n", name.c_str(), b.s.launches.size(), b.s.solve_steps.size(), b.dl.pieces.size());
}

static void good_mapped(const std::string& name, const sf::Symbolic& S, int W, const PlanKnobs& kn) {
    std::vector<int32_t> owner((size_t)std::max<Long>(S.nsuper, 1));
    double tf = 0, ml = 0;
    g_case = name;
    CHECK(sf::subtree_partition(S.nsuper, S.Super.data(), S.SuperMap.data(), S.Lsip.data(), S.Lsi.data(), W, owner.data(), &tf, &ml, 1.0 / W + 0.25) == 0);
    std::vector<int> cover((size_t)S.Lsxp[(size_t)S.nsuper], 0);
    size_t launches = 0;
    for (int r = 0; r < W; ++r) {
        g_case = name + " rank " + std::to_string(r);
        PlanInput in = input_of(S);
        MappedInput m;
        CHECK(sf_schedule_map_input(in, owner.data(), r, W, m) == SF_OK);
        Built b;
        build(in, kn, b);
        CHECK(b.rc == SF_OK);
        if (b.rc) return;
        check_schedule(in, b, cover);
        launches += b.s.launches.size();
    }
    g_case = name;
    check_cover(input_of(S), cover, std::vector<char>((size_t)S.nsuper, 1));     // the ranks together download the factor once
    printf("%-40s %d ranks, %zu launches in all\n", name.c_str(), W, launches);
}

// out of core at a budget of num / den of the factor; returns the top mode the partition chose
static int good_ooc(const sf::Symbolic& S, int num, int den, const PlanKnobs& kn) {
    g_case = "chol 12^3 out of core, budget " + std::to_string(num) + "/" + std::to_string(den);
    int64_t total = 0;
    for (Long s = 0; s < S.nsuper; ++s) total += (S.Super[s + 1] - S.Super[s]) * (S.Lsip[s + 1] - S.Lsip[s]);
    std::vector<int32_t> group((size_t)std::max<Long>(S.nsuper, 1), 0);
    int ngroups = 0, mode = 0;
    int64_t ge = 0, te = 0, need = 0;
    const int prc = sf::ooc_partition(S.nsuper, S.Super.data(), S.SuperMap.data(), S.Lsip.data(), S.Lsi.data(), total * num / den, group.data(), &ngroups, &ge, &te,
                                      &need, &mode);
    CHECK(prc == 0 || prc == 2);        // (2: no cut fits the budget, the cheapest one is returned)
    PlanInput in = input_of(S);
    in.ooc_group = group.data(); in.ooc_ngroups = ngroups; in.ooc_top_mode = mode;
    Built b;
    build(in, kn, b);
    CHECK(b.rc == SF_OK);
    if (b.rc) return -1;
    CHECK(ngroups > 1 && b.s.partial && b.s.ooc_groups == ngroups && b.s.ooc_top_mode == mode);
    std::vector<int> cover((size_t)S.Lsxp[(size_t)S.nsuper], 0);
    check_schedule(in, b, cover);
    check_cover(in, cover, std::vector<char>((size_t)S.nsuper, 1));
    printf("%-40s %d groups, top mode %d, %zu launches\n", g_case.c_str(), ngroups, mode, b.s.launches.size());
    return mode;
}

// ---- malformed inputs: SF_ERR_ARG from the stage named, and nothing for the sanitizers to report ----
static void expect_refused(const std::string& name, const PlanInput& in, int stage) {
    g_case = name;
    Built b;
    build(in, read_knobs(), b);
    CHECK(b.rc == SF_ERR_ARG && b.stage == stage);
    if (b.rc != SF_ERR_ARG || b.stage != stage) printf("  %s: rc %d at stage %d, expected SF_ERR_ARG at stage %d\n", name.c_str(), b.rc, b.stage, stage);
}

static void malformed(const sf::Symbolic& S) {
    const PlanInput good = input_of(S);
    const Long ns = S.nsuper;
    Long leaf = -1;                 // a supernode with rows below its columns, and its parent
    for (Long s = 0; s < ns && leaf < 0; ++s) if (good.nsrow(s) > good.nscol(s)) leaf = s;
    const Long par = S.SuperMap[(size_t)S.Lsi[(size_t)(S.Lsip[(size_t)leaf] + good.nscol(leaf))]];
    std::vector<int32_t> i32((size_t)ns, -1);
    std::vector<uint32_t> masks((size_t)ns, 0);
    {   // layout: a group number out of range
        PlanInput in = good; i32.assign((size_t)ns, -1); i32[0] = 0; i32[1] = 5;
        in.ooc_group = i32.data(); in.ooc_ngroups = 2;
        expect_refused("ooc_group out of range", in, 2);
    }
    {   // layout: a phase out of range
        PlanInput in = good; i32.assign((size_t)ns, 0); i32[0] = 2;
        in.phase_in = i32.data();
        expect_refused("phase out of range", in, 2);
    }
    {   // layout: a stored top supernode whose mask does not list this rank
        PlanInput in = good; i32.assign((size_t)ns, 0); i32[(size_t)ns - 1] = 1; masks.assign((size_t)ns, 0); masks[(size_t)ns - 1] = 2u;
        in.phase_in = i32.data(); in.top_mask = masks.data(); in.nranks = 2; in.rank = 0; in.load_top = 2;
        expect_refused("top mask without this rank", in, 2);
    }
    {   // layout: a top mode that does not exist
        PlanInput in = good; i32.assign((size_t)ns, -1); i32[0] = 0; i32[1] = 1;
        in.ooc_group = i32.data(); in.ooc_ngroups = 2; in.ooc_top_mode = 3;
        expect_refused("top mode 3", in, 2);
    }
    {   // layout: no layout of the top arena -- the layout runs before the validation, and with a top mode it walks the tree itself
        // (sf::ooc_top_layout): a first row below that maps to an earlier supernode is refused there
        PlanInput in = good; i32.assign((size_t)ns, -1); i32[0] = 0; i32[1] = 1;
        std::vector<Long> SuperMap = S.SuperMap;
        SuperMap[(size_t)S.Lsi[(size_t)(S.Lsip[(size_t)leaf] + good.nscol(leaf))]] = 0; in.SuperMap = SuperMap.data();
        in.ooc_group = i32.data(); in.ooc_ngroups = 2; in.ooc_top_mode = 1;
        expect_refused("no layout of the top arena", in, 2);
    }
    {   // validate: a panel size that does not match the supernode's shape
        PlanInput in = good; std::vector<Long> Lsxp = S.Lsxp; Lsxp[1] += 1; in.Lsxp = Lsxp.data();
        expect_refused("Lsxp against the shapes", in, 3);
    }
    {   // validate: Super does not end at n
        PlanInput in = good; std::vector<Long> Super = S.Super; Super[(size_t)ns] -= 1; in.Super = Super.data();
        expect_refused("Super[nsuper] != n", in, 3);
    }
    {   // validate: column pointers that fall
        PlanInput in = good; std::vector<Long> Lp = S.Lp; Lp[5] = Lp[6] + 1; in.Lp = Lp.data();
        expect_refused("falling column pointers", in, 3);
    }
    {   // validate: a row list that is not ascending
        PlanInput in = good; std::vector<Long> Lsi(S.Lsi.begin(), S.Lsi.end());
        Lsi[(size_t)(S.Lsip[(size_t)leaf] + good.nscol(leaf))] = S.n + 7; in.Lsi = Lsi.data();
        expect_refused("row index out of range", in, 3);
    }
    {   // validate: SuperMap is not the inverse of Super
        PlanInput in = good; std::vector<Long> SuperMap = S.SuperMap; SuperMap[(size_t)S.Super[1]] = 0; in.SuperMap = SuperMap.data();
        expect_refused("SuperMap against Super", in, 3);
    }
    {   // validate: a matrix entry without a place in its supernode's panel
        PlanInput in = good; std::vector<Long> Li(S.Li.begin(), S.Li.end());
        const Long j = S.Super[(size_t)ns - 1];        // first column of the last supernode: row 0 lies above it
        Li[(size_t)S.Lp[(size_t)j]] = 0; in.Li = Li.data();
        expect_refused("entry without a place", in, 3);
    }
    {   // levels: a stored supernode whose parent is not stored
        PlanInput in = good; i32.assign((size_t)ns, 0); i32[(size_t)par] = -1;
        in.phase_in = i32.data();
        expect_refused("row without a stored target", in, 3);
    }
    {   // levels: a streamed supernode that updates another group
        PlanInput in = good; i32.assign((size_t)ns, -1); i32[(size_t)leaf] = 0; i32[(size_t)par] = 1;
        in.ooc_group = i32.data(); in.ooc_ngroups = 2;
        expect_refused("update into another group", in, 3);
    }
    // (tree_levels' "not postordered" cannot be reached: validate_structure runs before it, a row below a supernode's columns is
    // larger than all of them, and SuperMap has been checked to be Super's inverse, so the parent's number is larger too.)
}

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const PlanKnobs kn = read_knobs();
    PlanKnobs unfused = kn;
    unfused.fuse_max = 0;           // SF_FUSE_MAX=0: the three-launch form everywhere
    sf::Symbolic c12, c6, lus8, luu8;
    analyze(12, false, false, c12);
    analyze(6, false, false, c6);
    analyze(8, true, false, lus8);
    analyze(8, true, true, luu8);

    good_whole("chol 12^3 in core", c12, kn);
    good_whole("chol 6^3 in core, SF_FUSE_MAX=0", c6, unfused);
    good_whole("lu 8^3 symmetric pattern", lus8, kn);
    good_whole("lu 8^3 unsymmetric pattern", luu8, kn);
    good_whole("lu 8^3 unsymmetric, SF_FUSE_MAX=0", luu8, unfused);
    good_mapped("chol 12^3 mapped over 4", c12, 4, kn);
    good_mapped("chol 12^3 mapped over 7", c12, 7, kn);
    good_mapped("lu 8^3 unsymmetric mapped over 2", luu8, 2, kn);
    // (budgets of 1/2 and 1/3 of the factor both give top mode 2 at 12^3; 3/4 gives mode 0, the resident top)
    std::set<int> modes;
    for (auto nd : {std::pair<int, int>{1, 2}, {1, 3}, {3, 4}}) modes.insert(good_ooc(c12, nd.first, nd.second, kn));
    g_case = "out of core";
    CHECK(modes.size() >= 2 && !modes.count(-1));
    malformed(c12);
    if (g_fail) { printf("schedule_sanitize: %d checks FAILED\n", g_fail); return 1; }
    printf("schedule_sanitize: ok\n");
    return 0;
}
