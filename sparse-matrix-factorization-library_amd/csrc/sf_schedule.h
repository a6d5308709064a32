// The schedule of a device plan: everything plan creation decides from the symbolic structure alone -- the panel layout, the launch
// list with its task tables, the segments of the distributed top, the out-of-core groups, the solve and download schedules.  No HIP
// here: sf_schedule.cpp builds all of it with the host compiler, tools/schedule_sanitize.cpp bounds-checks every table on a CPU, and
// sf_plan_build.hip adds the device resources that hold it.
#pragma once
#include <sparseframe_hip.h>

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "sf_download.h"
#include "sf_tasks.h"

using sf::GemmProb;
using sf::GemmTask;
using sf::PotrfTask;
using sf::TrsmTask;
using sf::StepTask;

// Launch::kind.  The numbers are part of the inspection ABI (sf_chol_plan_launch_info, tools/dump_schedules.py) and index last_kind_ms.
enum : int {
    LAUNCH_POTRF = 0,           // one-wave POTRF / GETRF of the diagonal blocks of a step
    LAUNCH_TRSM = 1,            // the rows below them
    LAUNCH_GEMM_INNER = 2,      // panel GEMM inside an outer block (K = the block's columns left of the step)
    LAUNCH_GEMM_SCATTER = 3,    // Schur updates into the ancestors, scatter fused
    LAUNCH_GEMM_OUTER = 4,      // left-looking update of an outer block (large K)
    LAUNCH_STEP = 5,            // fused step k_step (steps of at most fuse_max workgroups; otherwise GEMM_INNER, POTRF, TRSM)
    LAUNCH_UPDATE_SMALL = 6,    // Schur updates with K <= SU_MAXK (k_update_small, tasks in stasks)
    LAUNCH_OOC_GROUP = 7,       // out of core: group `first` takes over its buffer (zero + assemble); no tasks
};
static inline bool launch_is_gemm(int kind) { return kind >= LAUNCH_GEMM_INNER && kind <= LAUNCH_GEMM_OUTER; }

struct Launch {
    int kind;       // LAUNCH_*
    int64_t first;  // first task
    int count;
    int64_t prefix_first = 0;   // GEMM launches: first entry of this launch's K-step prefix (count + 1 entries)
    uint32_t units = 0;         // GEMM launches: total number of (tile, K step) units
    double flops = 0;           // GEMM launches: algorithmic flops of the problems in this launch
    bool split = false;         // distributed top: this rank executes the units [share_lo, share_hi) x units of this launch
    int share_idx = 0, share_cnt = 1;
    bool whole_tiles = false;   // GEMM launch executed in full by every rank of a group: no K-splitting, bit-identical results (see k_gemm)
    double share_lo = 0.0, share_hi = 1.0;      // = share_idx / share_cnt, (share_idx + 1) / share_cnt unless the set's shares are weighted
    int ticket = 0;             // index of the launch's claim counters in d_info[1 + ticket ..]: one (k_step) or eight (GEMMs, one per XCD)
};

// Distributed top phase (sf_chol_plan_create_distributed): phase 1 is cut into segments.  Before a segment runs, the
// regions it lists (the 512-column block of every top panel of the level whose 64-column chain is about to start) are
// summed over the ranks; until then a block only ever received additive updates (subtree Schur updates, split top
// Schur updates, split outer GEMMs), so its true value is the sum of the ranks' copies.
struct Segment {
    uint32_t mask = 0;                     // the ranks that hold (and sum) these block columns
    size_t l0 = 0, l1 = 0;                 // launches [l0, l1)
    std::vector<int64_t> off, cnt;         // whole block columns: doubles, relative to the factor base pointer
    // the part of each region that can be non-zero (rows >= the block's first column): `cols` pieces of `rows` doubles,
    // `ld` apart, starting at `src` -- what sf_chol_plan_segment_pack gathers into one contiguous buffer
    std::vector<int64_t> src, rows, cols, ld;
    int64_t packed = 0;                    // doubles in the packed buffer
    // look-ahead schedule: every additive contribution to these block columns except the one of the block column just before
    // them (which the segment's own first launch adds, replicated) is enqueued before the PREVIOUS segment starts, so the sum
    // over the ranks may run beside the previous segment's chain
    bool early = false;
    // OWNER-COMPUTES prototype (SF_TOP_OWNER=1): the near GEMM and the 64-column chain of this block column,
    // launches [l0, lc), run on ONE rank of the group only (group index owner_gi = block number mod group size); the finished block
    // column is then broadcast to the group before the launches [lc, l1) (the split far GEMMs, which read it).  -1: everybody runs
    // everything (the default: replicate and all-reduce).
    int owner_gi = -1;
    size_t lc = 0;
};

// ---------------- what plan creation is given ----------------
// lu == false: Cholesky, one nsrow x nscol panel per supernode at Lsxp[s] (the reference layout).
// lu == true: no-pivot LU kept on the device as a PAIR of nsrow x nscol panels per supernode,
//     PL(i,j) = L(i,j) for i > j (unit diagonal implied), PU(i,j) = U(j,i) for i >= j  (i.e. U^T),
// all PL panels first, then all PU panels (shift xC).  With that pairing every LU operation is the Cholesky one
// with the two operand roles taken from different panels:
//     L-panel update   C(ci,cj) -= sum_k PL(ci,k) PU(cj,k), ci >  cj      U-panel update  C -= sum_k PU(ci,k) PL(cj,k), ci >= cj
//     L21 <- L21 U11^{-1}  = k_trsm_block with D = PU's diagonal block    U12^T <- U12^T L11^{-T} = same kernel, D = PL's, unit
// which are exactly the reference's two GEMMs per update (L:2570-2577), its two-target scatter (L:2583-2604) and its
// two triangular solves (L:2653-2662), and the factor is gathered into the reference's (2*nsrow-nscol) x nscol panels
// (L:2514-2517) only when it is downloaded.
//
// ooc_group (one device, nranks == 1, no phase array): OUT-OF-CORE plan -- the factor does not stay on the device.  ooc_group[s] in
// [0, ooc_ngroups) = the streamed group of supernode s (sf::ooc_partition: whole subtrees, consecutive in the postorder), -1 = top.
// The top panels are resident; the groups' panels alias TWO buffers of the largest group's size (group g lives in buffer g & 1)
// and are factorized group by group, group g while group g - 1 is copied to the host; a group's buffer is zeroed and assembled
// again (LAUNCH_OOC_GROUP) once the copy of group g - 2 has left the device.  Such a plan only runs through the overlapped download
// (sf_chol_plan_factorize_to_host); it cannot solve or hand out its factor (partial).
// ooc_top_mode 1 (sf::ooc_partition decides): the top panels are not resident throughout either -- a top supernode is assembled
// with the first group below it, factorized right after the last one, and its place in the top arena (sf::ooc_top_layout) is
// given to another two groups later.  For factors that mode 0's resident top does not fit.
// dry: build the SCHEDULE only (launch list, segments, solve reduces, storage map, byte counts) -- no device is touched, nothing is
// allocated or uploaded, and the resulting plan can only be inspected (sf_chol_plan_launch_info & co.) and destroyed.  The schedule
// does not know the difference; sf_plan_build.hip walks the same list of device resources and only counts their bytes: what a rank
// WOULD do at a size or rank count this box cannot run (tests/test_config4_schedules.py walks all eight plans of 256^3 / 8 and
// checks them against each other).
// root_cum (optional, nranks + 1 values from 0 to 1): the shares of the split launches of the sets that ALL ranks take part in
// are [root_cum[r], root_cum[r + 1]) instead of equal ones -- create_mapped uses them to even out ranks whose other groups
// differ in weight (an elimination tree the amalgamation made lopsided)
// top_mask[s] (phase-1 supernodes, optional): bit r set = rank r takes part in supernode s (proportional mapping: the
// ranks whose subtrees lie below s).  Its panel exists only on those ranks, their GEMM shares and the all-reduce run
// inside that group.  Without it every rank takes part in every top supernode.
struct PlanInput {
    sf_long n = 0, nsuper = 0;
    const sf_long *Super = nullptr, *SuperMap = nullptr, *Lsip = nullptr, *Lsi = nullptr, *Lsxp = nullptr;
    const sf_long *Lp = nullptr, *Li = nullptr, *Up = nullptr, *Ui = nullptr;
    bool lu = false;
    int device = 0;
    bool dry = false;
    const int32_t* phase_in = nullptr;
    int load_top = 1, rank = 0, nranks = 1;
    const uint32_t* top_mask = nullptr;
    const double* root_cum = nullptr;
    const int32_t* ooc_group = nullptr;
    int ooc_ngroups = 0, ooc_top_mode = 0;

    sf_long nscol(sf_long s) const { return Super[s + 1] - Super[s]; }
    sf_long nsrow(sf_long s) const { return Lsip[s + 1] - Lsip[s]; }
    bool ooc() const { return ooc_group != nullptr && ooc_ngroups > 1; }
    int sides() const { return lu ? 2 : 1; }        // panels per supernode: L, and for LU the U^T panel
};

// ---------------- every environment knob of plan creation ----------------
struct PlanKnobs {
    bool trace = false;                 // SF_TRACE: the four phase times of plan_create on stderr
    int su_maxk = sf::SU_MAXK;          // SF_SU_MAXK: experiment knob
    // steps of up to this many workgroups run as ONE k_step launch; beyond it (swarms of tiny panels at the bottom levels)
    // the three-launch form -- stream-K GEMM, one-wave POTRF, 256-row TRSM workgroups -- has the better throughput.
    // Measured: 128^3 608 ms at 2048, 603 at 8192, 600 at 16384, 602 unlimited; 2-D 1000^2 (config 3) 12.0 ms up to 16384,
    // 12.3 at 32768, 13.3 unlimited
    // (LU config 5: 91.7 ms at 2048, 91.2 at 16384)
    // SF_FUSE_MAX (debug knob, read at plan creation): 0 forces the three-launch form everywhere, so that both forms
    // stay covered by the tests
    int64_t fuse_max = 32 * sf::GEMM_GRID;
    // (The ranks of a group must keep bit-identical copies of a shared panel: an LU threshold pivot decision may not depend on a
    // rank's own rounding.  Everything a chain reads is either an all-reduced sum or computed in a fixed order -- the step kernels,
    // and the look-ahead schedule's replicated near parts, which run k_gemm with whole_tiles: one addition per target element.)
    bool lookahead = true;              // SF_LOOKAHEAD=0: the round-1 schedule (tests cover both)
    bool use_graph = false;             // SF_GRAPH: resident factorizations replayed as one hipGraph
    bool top_owner = false;             // SF_TOP_OWNER: prototype schedule (Cholesky only), see Segment::owner_gi
    // device solve.  default: fused (35.3 ms at 128^3); SF_SOLVE_BWD_FUSED=0: two launches per backward step (38.2 ms)
    bool solve_diagT = true, solve_bwd_ahead = true, solve_bwd_fused = true, solve_fwd_ahead = true, solve_fwd_far_first = true;
    int solve_far_wgs = 512, solve_far_groups = 8;
    // overlapped download
    int dl_workers = DL_WORKERS_DEFAULT, dl_workers_fresh = DL_WORKERS_FRESH;      // SF_DL_WORKERS sets both
    bool dl_host_wait = true;
    int64_t dl_slot = DL_SLOT_DEFAULT;  // SF_DL_SLOT_MB
    bool dl_2d = true;                  // SF_DL_2D=0: copy the structurally zero rows of the Cholesky block columns like everything else
    bool dl_lu_pack = false;            // SF_DL_LU_PACK=1: the gather-kernel form of the LU download (schedule_download)
    bool stream_priority = true;        // SF_STREAM_PRIORITY=0: ordinary streams (create_device_resources)
    bool gemm_dynamic = true;           // SF_GEMM_DYNAMIC=0: static deal of k_gemm's whole-tile rounds
    double piv_tol = 0.0, piv_perturb = 0.0;    // SF_LU_PIVOT_TOL / SF_LU_PERTURB: the pivoting policy an LU plan starts with
};
PlanKnobs read_knobs();

// ---------------- what the stages hand to each other ----------------
// where the panels live, and which ranks share them
struct Layout {
    std::vector<int64_t> XP;        // device offset of every panel (doubles), -1: not stored on this rank; XP[nsuper] = the end
    std::vector<uint32_t> gmask;    // top supernodes stored here: the group of ranks that takes part in them
    int64_t ushift = 0;             // LU: PU(s) = PL(s) + ushift
    uint32_t all_ranks = 1;
    int rank = 0;
    int group_idx(uint32_t m) const { return __builtin_popcount(m & ((1u << rank) - 1u)); }     // this rank's index in group m
};

// host-side tables the scheduling stages fill and create_device_resources uploads; dropped when creation returns
struct PlanTables {
    std::vector<PotrfTask> potrf;
    std::vector<TrsmTask> trsm;
    std::vector<StepTask> steps;
    std::vector<GemmProb> probs;
    std::vector<GemmTask> gtasks;
    std::vector<GemmTask> stasks;           // 64 x 32 tiles of the Schur updates with K <= SU_MAXK (k_update_small)
    std::vector<uint32_t> ktprefix;         // K-step prefix of every GEMM launch (stream-K work distribution, see k_gemm)
    std::vector<int64_t> scatter_probs;     // index of the first problem of every (s, a) pair
    int64_t relmap_size = 0;
    std::vector<sf::SolveTask> solve;
    std::vector<int64_t> solveT_list;       // backward diagonal tasks that read a row-major copy of their block (indices into `solve`)
    int64_t solveT_size = 0;
    std::vector<sf::FillTile> fill_tiles;
    int32_t n_flags = 0;
    int64_t max_diag_tasks = 0;             // k_step launches: scratch for the 16 x 16 inverses, 1024 doubles per diagonal task
    // download schedule: launch count after which block column jo of supernode s is final (its 64-column chain is done)
    std::vector<int64_t> blk_first;
    std::vector<size_t> blk_ready;
    // assembly masks (empty: a whole plan, which has none).  Out of core: one per group, then the top's, nsuper entries each
    // (d_loadmask + g * nsuper, g = ooc_ngroups: the top); other partial plans: one
    std::vector<int8_t> loadmask;
};

// One set of independent supernodes of the sweep -- phase 0: a level of the owned subtrees; phase 1: the top
// supernodes of one level that share one group of ranks (ascending mask: every rank meets the sets it shares with
// another rank in the same order, so the groups' collectives cannot wait for each other in a circle).
struct LevelSet { int ph; std::vector<sf_long> sn; uint32_t mask; int share_idx, share_cnt; double lo = 0.0, hi = 1.0; int group = -1; };

// ---------------- what the schedule leaves in the plan ----------------
// Every host-only member of sf_chol_plan that the scheduling stages write and the rest of the library reads: containers and
// scalars, no device memory and no HIP handle.  sf_chol_plan derives from it.
struct SfSchedule {
    bool dry = false;           // schedule-only plan (plan_create's dry mode): no device resources, inspection only
    bool lu = false;            // no-pivot LU: every supernode has an L panel and a U^T panel (see PlanInput)
    bool u_alias = false;       // LU with a symmetric input: U aliases L (reference L:2718-2729)
    int64_t n = 0, nsuper = 0, nnz = 0, isize = 0, xsize = 0;
    int64_t unz = 0;            // LU: entries of U (by row)
    int64_t xC = 0;             // doubles in one set of nsrow x nscol panels (Cholesky: == xsize)
    int rank = 0, nranks = 1;   // distributed top: this rank's share of the split launches
    // multi-GPU sharding: phase[s] = 0 owned subtree supernode, 1 top supernode (replicated), -1 not on this rank
    std::vector<int8_t> phase;
    std::vector<int64_t> h_XP;  // device panel offsets (doubles), -1 when the panel is not stored on this rank
    bool partial = false;       // some supernodes are absent or the top panels are not loaded here
    int64_t top_off = 0, top_size = 0;   // contiguous region of the top panels inside one panel set
    size_t launch_split = 0;    // launches [0, launch_split) belong to phase 0, the rest to phase 1
    std::vector<Launch> launches;
    int nlevels = 0;
    std::vector<int> level_of;
    std::vector<Segment> segments;
    std::vector<uint32_t> all_masks;    // every group of the factorization (all ranks build the same sorted list)
    bool lookahead = true;         // shared top panels: outer GEMM split into a far part (ahead of the previous chain) and the last block's
    bool top_owner = false;        // SF_TOP_OWNER=1: owner-computes chains for the sets every rank takes part in (prototype, see Segment)
    bool use_graph = false;        // SF_GRAPH=1 (sf_chol_plan_factorize): the resident factorization as one hipGraph
    // out-of-core plan (PlanInput::ooc_group): number of streamed groups (0: in core), entries of one of the two group buffers
    // (the pieces per group, and how many of them are still on the device during a download: dl.group_pieces and the gate)
    int ooc_groups = 0;
    int64_t ooc_buf = 0;
    // top mode 1 (active top panels only): first / last group below every top supernode, and per group the (offset, length) ranges its
    // first launch zeroes for the top panels that start with it
    int ooc_top_mode = 0;
    std::vector<int32_t> ooc_first, ooc_last, ooc_wait;     // ooc_wait[g]: the last group whose copies group g's first launch waits for
    std::vector<std::vector<std::pair<int64_t, int64_t>>> ooc_zero;
    // device solve: task lists per (level, 64-column step).  The forward launch of a step has fwd_count tasks, the backward one
    // `count` (equal unless the plan is one rank's part of a distributed factor: the forward tiles that update ancestors' rows are
    // dealt out over the group, the backward ones are not); big: a panel of the step is wider than 64 columns; red_first /
    // red_count: sums over a group that precede the forward launch
    struct SolveStep { int64_t fwd_first, bwd_first; int count; int big; int nrows_tasks; int small; int ndiag; int fwd_count; int red_first, red_count; };
    static constexpr int SOLVE_TICKETS = 3;     // ticket words per step: forward, backward, the backward sweep's second launch (two-launch form)
    struct SolveReduce { int64_t off, cnt; uint32_t mask; };        // x[off .. off + cnt) summed over the ranks of `mask`
    std::vector<SolveStep> solve_steps;
    std::vector<SolveReduce> solve_reduces;
    std::vector<std::pair<int64_t, int64_t>> solve_own;           // column ranges whose solution this rank reports (distributed solve)
    std::vector<std::pair<int64_t, int64_t>> solve_load;          // column ranges whose right-hand side this rank loads
    bool solve_bwd_fused = false;
    int n_solve_sync = 0;
    // words of the solve's sync block: [info | n_solve_sync sync words | SOLVE_TICKETS tickets per step]
    size_t solve_sync_words() const { return 1 + (size_t)n_solve_sync + SOLVE_TICKETS * solve_steps.size(); }
    std::vector<int32_t> sel_pair_J, sel_pair_i;    // every scatter problem (J, a) as the schedule enumerated it: J, first panel row,
    std::vector<int64_t> sel_pair_off;              // relative-map offset (host only)
    std::vector<int64_t> load_dropL, load_dropU;   // entries given again later in their column (the last one is loaded): -1 in the load map
    int n_tickets = 0;          // claim counters behind d_info[0]
    int32_t n_flags = 1;        // k_step: flags, one per (panel, fused step)
    int64_t n_gemm_tasks = 0, n_pairs = 0;
    double flops_tiles = 0, flops_tiles_update = 0;   // MFMA flops the GEMM tiles issue (full 128 x 128 x 16 steps): all launches / Schur updates
    double flops_update_small = 0;      // part of flops_update done by k_update_small (K <= SU_MAXK)
    double flops_exec = 0, flops_update = 0, scatter_elems = 0, flops_panel_gemm = 0, flops_outer_gemm = 0;
    // host copies of the structure's pointers (the device solve, the download's unpacking)
    std::vector<int64_t> h_Lsip, h_Lsxp;
    std::vector<int32_t> h_Super;
    std::vector<int32_t> h_Lsi;     // Cholesky plans: the row lists, what sf_chol_plan_update_path walks (sf_updown_path.h)
};

// One rank's input of a mapped plan (sf_*_plan_create_mapped / _schedule_mapped) from the owner map of sf_subtree_partition:
// sf_schedule_map_input sets in's phase array, top masks, root shares, rank and nranks; `store` owns the arrays.  SF_OK or SF_ERR_ARG.
struct MappedInput { std::vector<uint32_t> mask; std::vector<int32_t> phase; std::vector<double> cum; };
int sf_schedule_map_input(PlanInput& in, const int32_t* owner, int rank, int nranks, MappedInput& store);

// The schedule in three steps, because plan_create has work of its own between them (the ways out, in order: the comment above
// sf_schedule_build in sf_schedule.cpp): the argument checks; then -- the device chosen and the plan allocated -- the panel layout,
// which sizes the factor; then -- the factor's allocation started on the helper thread -- everything else, into s, dl and T.
// Each returns SF_OK or SF_ERR_ARG.  stamps: optional, four times in ms -- before the validation, after the levels, after the
// task tables, at the end.
int sf_schedule_check_arguments(const PlanInput& in);
int sf_schedule_layout(const PlanInput& in, SfSchedule& s, Layout& lay);
int sf_schedule_build(const PlanInput& in, const PlanKnobs& kn, SfSchedule& s, sf::DlSchedule& dl, Layout& lay, PlanTables& T,
                      double* stamps = nullptr);
