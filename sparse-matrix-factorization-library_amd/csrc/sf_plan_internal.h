// Private view of the device plan shared by the translation units of libsparseframe_hip.so (not part of the C ABI).
#pragma once
#include <sparseframe_hip.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <utility>
#include <vector>

#include "sf_device_mem.h"
#include "sf_download.h"
#include "sf_factor_state.h"
#include "sf_kernels.h"
#include "sf_schedule.h"
#include "sf_updown_path.h"

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            fprintf(stderr, "[sparseframe-hip] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return SF_ERR_HIP;                                                              \
        }                                                                                   \
    } while (0)

// h on the device (one element at least); bytes_total grows by its size.  A failed allocation is SF_ERR_HIP
template <class T>
static inline int upload(sf::DevMem<T>& d, const std::vector<T>& h, size_t* bytes_total) {
    const size_t count = std::max<size_t>(h.size(), 1);
    if (d.alloc(count)) return SF_ERR_HIP;
    if (!h.empty()) HIP_TRY(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *bytes_total += count * sizeof(T);
    return SF_OK;
}

// struct path's device pool (sf_handlers.hip): the next plan_create of this thread may use `ptr` for its factor
extern "C" void sf_plan_offer_factor_buffer(double* ptr, size_t bytes);
extern "C" int sf_plan_factor_borrowed(const sf_chol_plan* p);
// blocks that came through the seam of sf_device_mem.h and are still live in this process: 0 device, 1 pinned host
extern "C" long sf_debug_live_blocks(int which);

// hipEventElapsedTime whose failure (an event that was never recorded) is expected and must not stay behind as the thread's
// "last error": callers that poll hipGetLastError after their own launches (PyTorch does) would report it as theirs
static inline bool elapsed_ms(float* ms, hipEvent_t a, hipEvent_t b) {
    if (hipEventElapsedTime(ms, a, b) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

struct sf_comm;      // one rank's end of a multi-GPU group (sf_multi.hip)
struct sf_chol_plan;
// ---- the device solve's host side (sf_solve.hip; shared by sf_chol_plan_solve[_many] and sf_chol_plan_solve_distributed) ----
// the plan's sync block d_solve_sync: the info word, n_solve_sync sync words, SOLVE_TICKETS ticket words per step; bytes: all of it
struct SolveSync { int *info, *sync, *tickets; size_t bytes; };
SolveSync sf_solve_sync(const sf_chol_plan* p);
// one step of a sweep on x (width 1: x[n]; sf::SVM_W: the row-major block), base = the panels the sweep reads
void sf_solve_step_fwd(sf_chol_plan* p, size_t k, const double* base, double* x, int width, const SolveSync& y, hipStream_t st);
void sf_solve_step_bwd(sf_chol_plan* p, size_t k, const double* base, double* x, int width, const SolveSync& y, hipStream_t st);
// the backward half: the row-major copies of the top steps' diagonal blocks (transpose_diag), then every step from the last
void sf_solve_sweep_bwd(sf_chol_plan* p, double* x, int width, bool transpose_diag, const SolveSync& y, hipStream_t st);
// both sweeps on x (the caller has zeroed the sync block on the stream)
void sf_solve_sweeps(sf_chol_plan* p, double* x, int width, bool transpose_diag, hipStream_t st);
// the end of a solve: read the info word, synchronize; SF_ERR_HIP if a bounded in-launch wait ran out
int sf_solve_finish(sf_chol_plan* p, hipStream_t st);
// ---- the factor's state (sf_factor_state.h) behind the one call that may wait for the device (sf_factorize.hip) ----
// the last factorization that was started has succeeded (a finished but unsynchronised one is collected here); an imported factor
// counts.  NOT required: that it is a factorization of the current values.
bool sf_factor_usable(sf_chol_plan* p);
// ... and it is the factor of the current values (a finished but unsynchronised factorization of them is collected here)
bool sf_factor_current(sf_chol_plan* p);
// ---- shared with the condition estimate and the transposed solves (sf_refine.hip) ----
// *d_anorm = device address of |A|_1 of the plan's CURRENT values, up to date on `st` (the residual's row / column form is set up by
// the first call, the norm recomputed when the values have changed); the plans sf_chol_plan_residual accepts
int sf_refine_anorm(sf_chol_plan* p, const double** d_anorm, hipStream_t st);
// ---- shared with the device-pointer solves (sf_device_io.hip) ----
// x <- A^{-T} x for an LU plan (sf_solve_t.hip; the caller has zeroed the sync block on the stream)
void tsolve_sweeps(sf_chol_plan* p, double* x, int width, bool transpose_diag, hipStream_t st);
// its two halves (shared with the LU half solves and C^T A^{-1} B, sf_gram_lu.hip): x <- U^{-T} x, the forward sweep over the U^T
// panels, and x <- F^T x, the backward sweep over the L panels with the interchanges undone (transpose_diag: its row-major
// diagonal copies, made from the L panels)
void tsolve_sweep_fwd(sf_chol_plan* p, double* x, int width, const SolveSync& y, hipStream_t st);
void tsolve_sweep_bwd(sf_chol_plan* p, double* x, int width, bool transpose_diag, const SolveSync& y, hipStream_t st);
// ---- shared by the update / downdate and the row modifications (sf_updown.hip, sf_rowmod.hip) ----
// the refusals of sf_chol_plan_update that do not depend on W: LU, an unknown flag, a plan that is not whole and resident,
// SF_DEV_PERM_IN without an ordering, no usable factor.  SF_OK: the plan's device is current.
int sf_updown_accepts(sf_chol_plan* p, int flags);
sf::UpdownStruct sf_updown_struct(const sf_chol_plan* p);
// the inverse of the ordering of sf_chol_plan_set_ordering: iperm[old] = new
int sf_updown_inverse_ordering(const sf_chol_plan* p, std::vector<int32_t>& iperm);
// the plan's update block d_upd (allocated by the first call of sf_updown_block): the n x UPD_W block of W, the pairs of one
// diagonal block, the info word
struct SfUpdownBlock { double *W, *rot; int* info; };
int sf_updown_block(sf_chol_plan* p);
SfUpdownBlock sf_updown_parts(sf_chol_plan* p);
// zero W on the plan's stream unless the last chunk left it zero; W counts as dirty from here until the caller says otherwise
int sf_updown_clear_w(sf_chol_plan* p);
// Rotate the block of W that is already on the device along `supers` (ascending): the pair of launches of every 64-column block,
// on the plan's stream, nothing waited for.  Returns the number of launches.
int64_t sf_updown_rotate(sf_chol_plan* p, const std::vector<int64_t>& supers, int sign, int kw);
// record ev_s1, read the info word, wait for the stream
int sf_updown_collect(sf_chol_plan* p, int* h_info);
// after the factor was written (rrc: what the launches and sf_updown_collect returned): the stats and the state's factor_replaced;
// a failure (rrc or h_info) leaves the factor broken.  Returns the call's status.
int sf_updown_commit(sf_chol_plan* p, int rrc, int h_info, const std::vector<int64_t>& supers, int64_t launches);
// ---- the host protocol of every entry point that takes columns through the resident factor (sf_apply.hip) ----
// the plan is whole and resident: one rank's, in core, with the solve's task lists
bool sf_plan_whole_resident(const sf_chol_plan* p);
// `ptr` is device (or managed) memory of the plan's device with room for `doubles` doubles from there on
bool sf_device_ptr_ok(const sf_chol_plan* p, const void* ptr, size_t doubles);
// doubles a column-major block of `cols` columns of `rows` rows spans; two such ranges of device memory share a byte (an empty one:
// it starts strictly inside the other)
size_t sf_block_span(int64_t rows, sf_long cols, sf_long ld);
bool sf_blocks_overlap(const void* a, size_t na, const void* b, size_t nb);
// the n x SVM_W block d_xm with its staging half / the parts and results of launch_quadform, d_qf: allocated by whichever call
// needs them first
int sf_solve_many_block(sf_chol_plan* p);
int sf_quadform_scratch(sf_chol_plan* p);
// One operator on x (width 1: x[n]; sf::SVM_W: a row-major block) on the plan's stream, the sync block cleared first.  SOLVE and
// TRANS are both sweeps of A^{-1} and (LU) A^{-T}; FWD_L the forward steps over the L panels; BWD sf_solve_sweep_bwd (L^{-T}, LU:
// U^{-1}); FWD_UT and BWD_LT the halves of TRANS.  copies: the backward sweep first makes its row-major diagonal copies.
enum SfSweep { SF_SWEEP_SOLVE, SF_SWEEP_TRANS, SF_SWEEP_FWD_L, SF_SWEEP_BWD, SF_SWEEP_FWD_UT, SF_SWEEP_BWD_LT };
int sf_apply_sweep(sf_chol_plan* p, SfSweep op, double* x, int width, bool copies);
// The timed stretch between the plan's solve events: open() records ev_s0; mark() records ev_s1 and polls the runtime's last
// error; close() waits for the stream -- through sf_solve_finish when sweeps ran, so that the info word is read -- and adds the
// stretch to total_ms (where the events' time can be read).  Copies enqueued between mark() and close() are waited for and not timed.
struct SfStretch {
    sf_chol_plan* p;
    double total_ms = 0;
    bool timed = false;     // some stretch's time could be read
    int open();
    int mark();
    int close(bool sweeps);
};
// A column-major block of the caller's, in host memory or (dev) in device memory, there optionally in the caller's ordering
struct SfCols { double* ptr; sf_long ld; bool dev; const int32_t* perm; };
// The two phases of a chunk of cw columns from column j0 on.  stage_in / stage_out: a host block to / from `stage` (column-major,
// leading dimension n), outside the timed stretch; a device block: nothing.  load / store: `stage` or the device block to / from
// x, inside it; width 1 works on x where it is staged (stage == x).
int sf_cols_stage_in(sf_chol_plan* p, const SfCols& s, sf_long j0, int cw, double* stage);
void sf_cols_load(sf_chol_plan* p, const SfCols& s, sf_long j0, int cw, int width, const double* stage, double* x);
void sf_cols_store(sf_chol_plan* p, const SfCols& d, sf_long j0, int cw, int width, const double* x, double* stage);
int sf_cols_stage_out(sf_chol_plan* p, const SfCols& d, sf_long j0, int cw, const double* stage);
// The chunk loop.  For every chunk of at most `width` columns of ncols: stage in, open the stretch, load, body(x, j0, cw), store,
// mark, tail(x, j0, cw), stage out, close.  src == null: the body makes the columns; dst == null: the body or the tail disposes
// of them.  width 1 (ncols == 1) is the one-column family on x[n]; width SVM_W works on the row-major block x + chunk * xstride,
// and a host block then goes through the staging half of d_xm (the caller has called sf_solve_many_block).
struct SfApply {
    const SfCols* src;
    const SfCols* dst;
    sf_long ncols;
    int width;
    double* x;
    size_t xstride;
    bool sweeps;        // the body runs sweeps (what close() is told)
};
// (the loop itself, a template on its two callables int(double* x, sf_long j0, int cw), follows the plan below)

// The overlapped download of a plan (sf_download.hip).  Its HIP handles -- dl_events, dl_streams, dl_done, h_ring,
// d_ring -- are NOT here: they stay in sf_plan_handles below, where the release order of DESIGN 8l is written; d_fill is device
// memory and goes with the plan's members, before every handle.
struct SfDownload : sf::DlSchedule {             // the schedule and the knobs (schedule_download, built once): sf_download.h
    sf::DevMem<sf::FillTile> d_fill;            // the LU direct download's sf::FillTile[], grouped by download event (fill_first)
    // ---- a running download ----
    sf::DlGate gate;                            // where the enqueue thread and the copy workers meet (sf_download.h)
    bool active = false;                        // sf_run_launches records the events and publishes them
    size_t next_ev = 0;                         // enqueue thread only: the first event not yet recorded
    double* host = nullptr;                     // destination (reference layout)
    std::vector<std::thread> threads;
    std::vector<double> trace;                  // SF_DL_TRACE: 3 times per piece
    double t0 = 0;
    int cpus_known = 0;                         // 0 not looked up yet, 1 cpus holds the CPUs of the device's NUMA node, -1 none / disabled
    std::vector<int> cpus;
    int last_cpu[DL_WORKERS_MAX] = {};          // CPU each copy worker finished its last download on (SF_TRACE)
    int workers_last = 0;                       // workers of the last download
};

// What a plan gives back AFTER its device memory, in this order: the graph, the events, stream2, the download's events, streams and
// rings, the main stream last.  Members go in reverse order of declaration and a base after the members of the class derived
// from it, so the order is written here once, backwards, and sf_chol_plan needs no list of what it holds.  The
// download's handles stay in this list, not in SfDownload: moving them would move their release before the device memory's.
struct sf_plan_handles {
    sf::Stream stream;                          // ours, or the caller's (own_stream, sf_chol_plan_set_stream)
    sf::DevMem<double> d_ring;                  // LU: device staging of packed pieces, same shape as h_ring
    sf::PinnedMem h_ring;                       // pinned staging ring: dl.workers x 2 slots of dl.slot doubles
    sf::Event dl_done[DL_WORKERS_MAX][2];
    sf::Stream dl_streams[DL_WORKERS_MAX];
    std::vector<sf::Event> dl_events;
    sf::Stream stream2;                         // the collectives of look-ahead segments and their pack copies
    sf::Event ev_unpacked[2], ev_reduced[2], ev_contrib[2];
    sf::Event ev_s1, ev_s0, ev1, ev0;
    sf::GraphExec graph_exec;
};

// The schedule -- every host-only member that plan creation decides from the structure -- is the base SfSchedule (sf_schedule.h);
// a base goes after the members and sf_plan_handles, declared first, goes last, so the release order above stands.
struct sf_chol_plan : sf_plan_handles, SfSchedule {
    ~sf_chol_plan() { if (!dry) (void)hipSetDevice(device); }       // (the owners free on the plan's device)
    SfDownload dl;                              // the overlapped download: schedule, knobs, running state (above)
    double last_to_host_ms = 0;                 // wall time of the last sf_chol_plan_factorize_to_host
    // LU pivoting (sf_kernels.h, PivotCtl): threshold inside the 64 x 64 diagonal blocks, perturbation = piv_perturb * max|a_ij|
    // Defaults = the reference's behaviour: no pivoting, no perturbation (magma_dgetrf_nopiv, L:2653); opt-in by sf_lu_plan_set_pivoting,
    // SparseFrame_set_pivoting (struct path) or SF_LU_PIVOT_TOL / SF_LU_PERTURB at plan creation
    double piv_tol = 0.0, piv_perturb = 0.0, amax = 0;
    double piv_tol0 = 0.0, piv_perturb0 = 0.0;      // the policy the plan was created with (environment or none): what a struct call without a policy of its own gets
    sf::DevMem<int32_t> d_piv;   // pivpos[n] | pivinv[n] | perturbation counter
    int last_perturbed = 0;
    sf::DevMem<int64_t> d_Up;    // LU, unsymmetric input: U by row
    sf::DevMem<int32_t> d_Ui;
    sf::DevMem<double> d_Ux;
    sf::DevMem<int64_t> d_Xp;    // LU: offsets of the nsrow x nscol panels (the reference's Lsxp has the packed sizes)
    sf::DevMem<double> d_pack;   // LU: staging buffer in the reference layout for the download
    // SF_GRAPH=1 (use_graph, sf_chol_plan_factorize): the resident factorization as one hipGraph
    bool capturing = false;
    int graph_epoch = 0;
    double graph_tol = 0, graph_eps = 0;
    hipStream_t graph_stream = nullptr;
    bool factor_borrowed = false;       // d_Lsx holds a buffer the creator lent (sf_plan_offer_factor_buffer, DevMem::lend)
    sf::DevMem<double> d_status;    // one word: the ranks' status agreement before the first data collective (sf_multi.hip)
    sf::DevMem<double> d_scratch;   // packed segment buffers (2 x max over the segments: segment k uses half k & 1)
    int64_t scratch_elems = 0;
    bool unpacked_recorded[2] = {false, false};
    int64_t packed_pending = -1;   // segment whose packed buffer has to be scattered back before it runs
    bool own_stream = true;
    sf::DevMem<int8_t> d_loadmask;
    sf::DevMem<int64_t> d_loadmapL, d_loadmapU;      // whole plans: offset into d_Lsx of every entry of L (/ U), -1 = not loaded
    // device solve (Cholesky, whole matrix on one device): task lists per (level, 64-column step)
    sf::DevMem<sf::SolveTask> d_solve;
    // backward sweep: row-major copies of the diagonal blocks of the top levels' steps (made at the start of every solve)
    sf::DevMem<double> d_solveT;
    sf::DevMem<int64_t> d_solveT_list;
    int64_t n_solveT = 0;
    sf::DevMem<double> d_x;
    sf::DevMem<double> d_resid;  // sf_chol_plan_validate: r | column sums | b | 4 norms
    sf::DevMem<int> d_solve_sync;
    double last_solve_ms = 0;
    // sf_chol_plan_solve_many: the n x SVM_W row-major block and an n x SVM_W column-major staging buffer for the copies, one
    // allocation made by the first call (not in bytes_device)
    sf::DevMem<double> d_xm;
    size_t bytes_solve_many = 0;
    double last_solve_many_ms = 0;
    // sf_chol_plan_solve_half / _quadform / _sample (sf_sample.hip): d_x or d_xm as above; d_qf = the parts and the results of the
    // per-column sums of squares, a fixed size allocated by the first quadform call (in no byte count)
    sf::DevMem<double> d_qf;
    double last_half_ms = 0, last_quadform_ms = 0, last_sample_ms = 0;
    // sf_chol_plan_gram / _gram_device (sf_gram.hip): the Y store -- gram_chunks row-major n x SVM_W blocks, the parts of one chunk
    // row, the result block of the host-array call -- allocated or grown by the first call that needs it (bytes_gram, not in
    // bytes_device); last_gram_parts: slabs per tile of the last call (0: the one-column path)
    // sf_lu_plan_gram / _gram_device (sf_gram_lu.hip): the same store holds gram_chunks Z blocks, gram_chunks_y Y blocks, the parts of
    // one chunk column and the padded result block
    sf::DevMem<double> d_gram;
    int64_t gram_chunks = 0, gram_chunks_y = 0;
    size_t bytes_gram = 0;
    double last_gram_ms = 0;
    int last_gram_parts = 0;
    // sf_*_plan_set_ordering / _set_value_map (sf_device_io.hip): perm[new] = old as 32-bit indices (as d_Lsi), the value map
    // (nnz entries for Lx, then unz for Ux) and the parts of the LU plans' max |a_ij|; bytes_ordering is not in bytes_device
    sf::DevMem<int32_t> d_perm;
    sf::DevMem<int64_t> d_vmap;
    int64_t vmap_nsrc = 0;
    sf::DevMem<double> d_dio_part;
    size_t bytes_ordering = 0;
    SfFactorState fs;               // values, factor, selected inverse, fingerprints: which belongs to which (sf_factor_state.h)
    // sf_chol_plan_selinv (sf_selinv.hip)
    struct SelBig { sf::SelUnit u; int zslabs, sslabs; };
    struct SelStep { int64_t small_first, small_count, big_first, big_count; };   // one level: big units, then narrow supernodes
    bool sel_scheduled = false;
    std::vector<sf::SelUnit> sel_small;
    std::vector<SelBig> sel_big;
    std::vector<SelStep> sel_steps;
    std::vector<sf::SelPair> sel_pairs_h;
    int64_t sel_linv_elems = 0, sel_y_elems = 0, sel_z_elems = 0, sel_s_elems = 0;
    sf::DevMem<double> d_sel;            // the arena (xsize doubles), allocated with the scratch by the first call (not in bytes_device)
    sf::DevMem<double> d_sel_diag;
    sf::DevMem<sf::SelUnit> d_sel_units;
    sf::DevMem<sf::SelPair> d_sel_pairs;
    sf::DevMem<double> d_sel_scratch;
    size_t bytes_selinv = 0;
    double last_selinv_ms = 0, flops_selinv = 0;
    // sf_*_plan_selinv_values / _trace / _entries (sf_selinv_pattern.hip): the position of every entry of the structure in one panel
    // set (posL, then posU of an LU plan with its own U structure) with the off-diagonal marks of a Cholesky plan, the parts and
    // results of a trace, the staging buffer of the (row, column) pairs -- each allocated by the first call that needs it
    // (bytes_selinv_pattern, not in bytes_device)
    sf::DevMem<int64_t> d_sp_pos;
    sf::DevMem<uint8_t> d_sp_offd;
    sf::DevMem<double> d_sp_part;
    sf::DevMem<char> d_sp_stage;
    size_t bytes_selinv_pattern = 0;
    double last_selinv_pattern_ms = 0;
    int64_t last_selinv_outside = 0;
    // sf_*_plan_adjoint_values / _logdet_grad_values (sf_adjoint.hip): the column and the term marks of every position (L's,
    // then U's of an LU plan with its own U structure), the unmapped result of a mapped or host-array call, and the value map by source
    // entry (adj_vmap_gen: vmap_gen it was built from) -- each allocated by the first call that needs it (bytes_adjoint, not in
    // bytes_device)
    sf::DevMem<int32_t> d_adj_col;
    sf::DevMem<uint8_t> d_adj_mark;
    sf::DevMem<double> d_adj_tmp;
    sf::DevMem<int64_t> d_adj_src;              // sptr[nsrc + 1] | the positions by source entry, ascending within one
    int64_t vmap_gen = 0, adj_vmap_gen = -1, adj_src_entries = 0;
    size_t bytes_adjoint = 0;
    double last_adjoint_ms = 0;
    // sf_chol_plan_residual / sf_chol_plan_refine (sf_refine.hip): A by rows as positions into d_Lx / d_Ux (unsymmetric LU: also by
    // columns, for |A|_1), the vectors b | x | best x | r | w and the scalars; one set of allocations made by the first call
    // (not in bytes_device)
    sf::DevMem<int64_t> d_rf_ptr, d_rf_pos, d_rf_cptr, d_rf_cpos;
    sf::DevMem<int32_t> d_rf_col, d_rf_ccol;
    sf::DevMem<double> d_rf_vec;
    int64_t rf_entries = 0;
    size_t bytes_refine = 0;
    int last_refine_iters = 0;
    double last_refine_berr0 = 0, last_refine_berr = 0, last_refine_ms = 0, last_residual_ms = 0;
    // sf_*_plan_condest (sf_solve_t.hip): x | the sign vector | the iteration's scalars, allocated by the first call (not in
    // bytes_device)
    // sf_chol_plan_update (sf_updown.hip): the row-major n x UPD_W block of W, the rotation pairs of one 64-column block
    // and the info word, one allocation made by the first call (bytes_update, not in bytes_device)
    sf::DevMem<double> d_upd;
    size_t bytes_update = 0;
    bool upd_w_dirty = true;        // the block of W may hold something: zero it before the next chunk (a finished chunk leaves zeros)
    double last_updown_ms = 0;
    int64_t upd_path_supers = 0, upd_path_cols = 0, upd_launches = 0, upd_bad_column = -1;
    // sf_chol_plan_rowdel / _rowadd (sf_rowmod.hip) work in the same block; what the last call did
    int64_t rowmod_row_tasks = 0, rowmod_sweep_supers = 0, rowmod_launches = 0, rowmod_bad_index = -1, rowmod_not_deleted = 0;
    sf::DevMem<double> d_cond;
    size_t bytes_condest = 0;
    int last_condest_solves = 0;
    double last_condest_ms = 0;
    int device = 0;

    // device copies of the structure
    sf::DevMem<int64_t> d_Lp;
    sf::DevMem<int32_t> d_Li;
    sf::DevMem<double> d_Lx;
    sf::DevMem<int32_t> d_Super;
    sf::DevMem<int32_t> d_SuperMap;
    sf::DevMem<int64_t> d_Lsip;
    sf::DevMem<int32_t> d_Lsi;
    sf::DevMem<int64_t> d_Lsxp;
    sf::DevMem<double> d_Lsx;
    sf::DevMem<int> d_info;      // [0]: status bits of the running factorization; [1 ..]: task-claim counters of the k_step launches
    bool gemm_dynamic = true;   // k_gemm: whole-tile rounds claimed from per-XCD counters (SF_GEMM_DYNAMIC=0: static deal)

    sf::DevMem<PotrfTask> d_potrf;
    sf::DevMem<TrsmTask> d_trsm;
    sf::DevMem<StepTask> d_steps;
    sf::DevMem<int> d_flags;     // k_step: one flag per (panel, fused step); == the factorization's epoch once its diagonal block is factored
    sf::DevMem<double> d_tinv;   // k_step: inverses of the 16 x 16 diagonal sub-blocks, per diagonal task of the running launch
    std::vector<uint64_t> h_hash;    // per-supernode fingerprints of the factor (sf_plan_panel_hashes; fs.hashes_current())
    sf::DevMem<GemmProb> d_probs;
    sf::DevMem<GemmTask> d_gtasks;
    sf::DevMem<GemmTask> d_stasks;   // tiles of k_update_small
    sf::DevMem<uint32_t> d_ktprefix;
    sf::DevMem<int32_t> d_relmap;

    size_t bytes_device = 0;
    bool profiling = false;
    double last_ms = 0, last_load_ms = 0, last_panel_ms = 0, last_update_ms = 0;
    double last_kind_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

template <class Body, class Tail>
int sf_apply_chunks(sf_chol_plan* p, const SfApply& a, SfStretch& t, Body&& body, Tail&& tail) {
    for (sf_long j0 = 0; j0 < a.ncols; j0 += a.width) {
        const int cw = (int)std::min<sf_long>(a.width, a.ncols - j0);
        double* x = a.x + (size_t)(j0 / a.width) * a.xstride;
        double* stage = a.width == 1 ? x : p->d_xm ? p->d_xm + (size_t)p->n * a.width : nullptr;
        if (a.src)
            if (int rc = sf_cols_stage_in(p, *a.src, j0, cw, stage)) return rc;
        if (int rc = t.open()) return rc;
        if (a.src) sf_cols_load(p, *a.src, j0, cw, a.width, stage, x);
        if (int rc = body(x, j0, cw)) return rc;
        if (a.dst) sf_cols_store(p, *a.dst, j0, cw, a.width, x, stage);
        if (int rc = t.mark()) return rc;
        if (int rc = tail(x, j0, cw)) return rc;
        if (a.dst)
            if (int rc = sf_cols_stage_out(p, *a.dst, j0, cw, stage)) return rc;
        if (int rc = t.close(a.sweeps)) return rc;
    }
    return SF_OK;
}
template <class Body>
int sf_apply_chunks(sf_chol_plan* p, const SfApply& a, SfStretch& t, Body&& body) {
    return sf_apply_chunks(p, a, t, body, [](double*, sf_long, int) { return SF_OK; });
}

// The factorization driver (sf_factorize.hip): launches [l0, l1) of the plan on its stream; first: the start of a factorization
// (timer, memsets, assembly); last: its end (timer, and with sync the status)
int sf_run_launches(sf_chol_plan* p, size_t l0, size_t l1, bool first, bool last, int sync);
// This rank's window [lo, hi) of a launch's `total` divisible items (GEMM launches: stream-K units; k_update_small: tiles); all of
// them unless the launch is split over a group.  The boundaries are the same doubles on the two ranks they separate, so the windows
// of a group's members tile [0, total) exactly (checked for every launch of 256^3 / 8 by tests/test_config4_schedules.py).
static inline void launch_window(const Launch& L, int64_t total, int64_t* lo, int64_t* hi) {
    *lo = 0; *hi = total;
    if (!L.split) return;
    *lo = (int64_t)((double)total * L.share_lo);
    *hi = L.share_hi >= 1.0 ? total : (int64_t)((double)total * L.share_hi);
}
// Overlapped download (sf_download.hip).  sf_dl_begin starts the copy workers of a factorization whose launches are
// about to be enqueued with sf_run_launches (which records and publishes the piece events while dl.active is set);
// sf_dl_end publishes what is left, waits for the workers and returns SF_OK or the first error.
int sf_dl_begin(sf_chol_plan* p, double* host_out);
// sf_run_launches' two calls: record the events of everything that is final once `done` launches have been enqueued and tell the
// copy workers; out of core, before group g takes over its buffer: wait until the pieces of the groups that held it (and, top mode
// 2, the top panels whose places it takes) have left the device -- SF_ERR_HIP when the download was aborted meanwhile
hipError_t sf_dl_publish(sf_chol_plan* p, size_t done);
int sf_dl_wait_groups(sf_chol_plan* p, int g);
// the constants of sf_selinv_pattern.hip for sf_chol_plan_stat: 0 the column chunk, 1 entries per part, 2 pairs per staging trip, 3 max m
double sf_selpat_constant(int which);
// per-supernode fingerprints (k_factor_hash) of the factor the plan holds, in the reference layout's index space; 0 for panels this
// rank does not store.  Computed once per factorization (about one read of the factor), then cached.
extern "C" int sf_plan_panel_hashes(sf_chol_plan* p, const uint64_t** out);
int sf_dl_end(sf_chol_plan* p);
// gathers the panels of the parts (plans of several ranks, one pattern) into the whole plan dst (sf_segments.hip)
int sf_plan_import_from(sf_chol_plan* dst, sf_chol_plan* const* parts, int nparts);
// pipelined segment sums (sf_segments.hip), used by sf_chol_plan_factorize_distributed
int sf_seg_begin(sf_chol_plan* p, sf_long k, void** dptr, sf_long* count);
void* sf_plan_stream2(sf_chol_plan* p);
int sf_seg_reduced(sf_chol_plan* p, sf_long k);
int sf_seg_finish(sf_chol_plan* p, sf_long k);
// owner-computes segments (Segment::owner_gi >= 0): sf_seg_finish runs only the owner's part [l0, lc); then the broadcast --
// sf_seg_bcast_begin packs the finished block column on the owner / zeroes the buffer elsewhere (main stream), the caller sums the
// buffer over the group (x + 0 + ... + 0: every rank gets the owner's values), sf_seg_bcast_finish scatters it back and runs [lc, l1)
int sf_seg_is_owner_segment(const sf_chol_plan* p, sf_long k);
int sf_seg_bcast_begin(sf_chol_plan* p, sf_long k, void** dptr, sf_long* count);
int sf_seg_bcast_finish(sf_chol_plan* p, sf_long k);
int sf_seg_early(const sf_chol_plan* p, sf_long k);
