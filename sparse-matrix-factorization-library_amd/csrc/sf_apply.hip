// The host protocol of the entry points that take a block of columns through the resident factor: solves, half solves, quadratic
// forms, sampling, the device-pointer forms, B^T A^{-1} B and C^T A^{-1} B.  DESIGN 8j.
//
// The kernels, task lists, sync words and tickets are sf_solve.hip's and sf_solve_t.hip's, the layout kernels sf_solve.hip's and
// sf_device_io.hip's.  What is here, once: which plans qualify, the lazily allocated blocks, the clear-and-sweep of one operator,
// the timed stretch, a chunk's way in and out, and the chunk loop.  An entry point keeps its own argument checks and then reads
// as source, body, sink.
#include <sparseframe_hip.h>

#include <algorithm>

#include "sf_plan_internal.h"

bool sf_plan_whole_resident(const sf_chol_plan* p) {
    return !(p->dry || p->partial || p->nranks > 1 || p->ooc_groups > 1 || (p->nsuper > 0 && !p->d_solve));
}

// Decided on the host, before anything is enqueued: a host pointer never reaches a kernel.  (hipPointerGetAttributes fails for
// ordinary host memory on some runtimes and reports it as unregistered on others; either way it is refused and no error is left
// behind.)
bool sf_device_ptr_ok(const sf_chol_plan* p, const void* ptr, size_t doubles) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged) return false;
    if (a.device != p->device) return false;
    void* base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)ptr) != hipSuccess) {
        (void)hipGetLastError();
        return true;        // (no range to be had for this kind of memory: the attributes have spoken)
    }
    const char* end = (const char*)base + size;
    return (const char*)ptr >= (const char*)base && (size_t)(end - (const char*)ptr) >= doubles * sizeof(double);
}

size_t sf_block_span(int64_t rows, sf_long cols, sf_long ld) {
    return (rows > 0 && cols > 0) ? (size_t)(cols - 1) * (size_t)ld + (size_t)rows : 0;
}

bool sf_blocks_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb * sizeof(double) && b0 < a0 + na * sizeof(double);
}

// ---- the seam of sf_device_mem.h: the only calls of the runtime's allocator outside the struct path's pool ----
static std::atomic<long> g_live_blocks[2];      // 0 device, 1 pinned host

static int seam_took(hipError_t e, void** ptr, int which) {
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *ptr = nullptr;
        return 1;
    }
    if (*ptr) ++g_live_blocks[which];       // (an empty block is null and is never given back)
    return 0;
}
int sf_dev_malloc(void** ptr, size_t bytes) { return seam_took(hipMalloc(ptr, bytes), ptr, 0); }
int sf_host_malloc(void** ptr, size_t bytes) { return seam_took(hipHostMalloc(ptr, bytes, hipHostMallocDefault), ptr, 1); }
void sf_dev_free(void* ptr) {
    (void)hipFree(ptr);
    --g_live_blocks[0];
}
void sf_host_free(void* ptr) {
    (void)hipHostFree(ptr);
    --g_live_blocks[1];
}
extern "C" long sf_debug_live_blocks(int which) { return (which == 0 || which == 1) ? g_live_blocks[which].load() : -1; }

int sf_solve_many_block(sf_chol_plan* p) {
    if (p->d_xm) return SF_OK;
    const size_t count = 2 * (size_t)p->n * sf::SVM_W;
    if (int rc = p->d_xm.alloc(count)) return rc;
    p->bytes_solve_many = count * sizeof(double);
    return SF_OK;
}

int sf_quadform_scratch(sf_chol_plan* p) { return p->d_qf ? SF_OK : p->d_qf.alloc((size_t)(sf::QF_MAXB + 1) * sf::SVM_W); }

// The row-major copies of the top steps' diagonal blocks (d_solveT) are made from the U^T panels (Cholesky: the L panels) by BWD
// and SOLVE and from the L panels by BWD_LT and TRANS, and neither may see the other's: a caller that alternates the two asks
// BOTH for their copies every time, every other caller on the first chunk of every call (the factor may have changed since).
int sf_apply_sweep(sf_chol_plan* p, SfSweep op, double* x, int width, bool copies) {
    hipStream_t st = p->stream;
    const SolveSync y = sf_solve_sync(p);
    HIP_TRY(hipMemsetAsync(p->d_solve_sync, 0, y.bytes, st));
    switch (op) {
        case SF_SWEEP_SOLVE: sf_solve_sweeps(p, x, width, copies, st); break;
        case SF_SWEEP_TRANS: tsolve_sweeps(p, x, width, copies, st); break;
        case SF_SWEEP_FWD_L:
            for (size_t k = 0; k < p->solve_steps.size(); ++k) sf_solve_step_fwd(p, k, p->d_Lsx, x, width, y, st);
            break;
        case SF_SWEEP_BWD: sf_solve_sweep_bwd(p, x, width, copies, y, st); break;
        case SF_SWEEP_FWD_UT: tsolve_sweep_fwd(p, x, width, y, st); break;
        case SF_SWEEP_BWD_LT: tsolve_sweep_bwd(p, x, width, copies, y, st); break;
    }
    return SF_OK;
}

// the plan's own event pair (ev0/ev1 time the factorization; sf_chol_plan_sync has read them by now): nothing is created here, so
// an error return leaks nothing
int SfStretch::open() {
    HIP_TRY(hipEventRecord(p->ev_s0, p->stream));
    return SF_OK;
}
int SfStretch::mark() {
    HIP_TRY(hipEventRecord(p->ev_s1, p->stream));
    HIP_TRY(hipGetLastError());
    return SF_OK;
}
int SfStretch::close(bool sweeps) {
    if (sweeps) {
        if (int rc = sf_solve_finish(p, p->stream)) return rc;
    } else {
        HIP_TRY(hipStreamSynchronize(p->stream));
    }
    float ms = 0;
    if (elapsed_ms(&ms, p->ev_s0, p->ev_s1)) {
        total_ms += ms;
        timed = true;
    }
    return SF_OK;
}

// one copy either way: 2-D when the caller's leading dimension is padded
int sf_cols_stage_in(sf_chol_plan* p, const SfCols& s, sf_long j0, int cw, double* stage) {
    if (s.dev) return SF_OK;
    const size_t col = (size_t)p->n * sizeof(double);
    const double* B = s.ptr + j0 * s.ld;
    if (s.ld == p->n) HIP_TRY(hipMemcpyAsync(stage, B, col * cw, hipMemcpyHostToDevice, p->stream));
    else HIP_TRY(hipMemcpy2DAsync(stage, col, B, (size_t)s.ld * sizeof(double), col, cw, hipMemcpyHostToDevice, p->stream));
    return SF_OK;
}

int sf_cols_stage_out(sf_chol_plan* p, const SfCols& d, sf_long j0, int cw, const double* stage) {
    if (d.dev) return SF_OK;
    const size_t col = (size_t)p->n * sizeof(double);
    double* X = d.ptr + j0 * d.ld;
    if (d.ld == p->n) HIP_TRY(hipMemcpyAsync(X, stage, col * cw, hipMemcpyDeviceToHost, p->stream));
    else HIP_TRY(hipMemcpy2DAsync(X, (size_t)d.ld * sizeof(double), stage, col, col, cw, hipMemcpyDeviceToHost, p->stream));
    return SF_OK;
}

// (both packs write zeros into the columns [cw, SVM_W) of the block: the padding of a last chunk)
void sf_cols_load(sf_chol_plan* p, const SfCols& s, sf_long j0, int cw, int width, const double* stage, double* x) {
    if (s.dev && width == 1) sf::launch_dev_load1(s.ptr, s.perm, p->n, x, p->stream);
    else if (s.dev) sf::launch_dev_pack(s.ptr + j0 * s.ld, s.ld, s.perm, p->n, cw, x, p->stream);
    else if (width > 1) sf::launch_solve_many_pack(stage, p->n, cw, x, p->stream);
}

void sf_cols_store(sf_chol_plan* p, const SfCols& d, sf_long j0, int cw, int width, const double* x, double* stage) {
    if (d.dev && width == 1) sf::launch_dev_store1(x, d.perm, p->n, d.ptr, p->stream);
    else if (d.dev) sf::launch_dev_unpack(x, d.perm, p->n, cw, d.ptr + j0 * d.ld, d.ld, p->stream);
    else if (width > 1) sf::launch_solve_many_unpack(x, p->n, cw, stage, p->stream);
}
