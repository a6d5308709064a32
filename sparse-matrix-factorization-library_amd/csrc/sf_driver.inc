// The reference's top-level driver -- int SparseFrame(int argc, char **argv), the ONE symbol its public header declares
// (Cholesky/Include/SparseFrame.h:43, LU/Include/SparseFrame.h) and what Demo/demo.c calls -- over this library's stage functions,
// so that the reference's demo links against libsparseframe_hip.so / libsparseframe_lu_hip.so unchanged.  Behaviour follows
// Cholesky/Source/SparseFrame.c:3323-3467 (LU: the same function in LU/Source/SparseFrame.c): argv[1..] are MatrixMarket files;
// up to MATRIX_THREAD_NUM = 2 (parameter.h:10) matrix threads take them from a shared counter and run
// initialize -> read -> analyze -> factorize -> validate -> cleanup on their own matrix_info, sharing one gpu_info_list; the same
// lines are printed (PRINT_INFO is on in the reference's parameter.h:8).  Differences: host threads are std::thread (no OpenMP /
// omp_set_nested), a stage that fails is reported on stderr and the matrix is skipped (the reference ignores every return code),
// and the return value is the number of matrices that failed.
// Included by sf_chol_host.cpp and sf_lu_host.cpp: each library has its own struct layout behind the same names.

int SparseFrame_allocate_matrix(struct common_info_struct* common, struct matrix_info_struct** list) {     // C:368-383
    if (!common || !list) return 1;
    const int nt = common->matrixThreadNum > 0 ? common->matrixThreadNum : 1;
    *list = (struct matrix_info_struct*)calloc((size_t)nt, sizeof(struct matrix_info_struct));
    return *list ? 0 : 1;
}

int SparseFrame_free_matrix(struct common_info_struct* common, struct matrix_info_struct** list) {         // C:385-398
    if (!list || !*list) return 1;
    free(*list);
    *list = nullptr;
    if (common) common->numSparseMatrix = 0;
    return 0;
}

int SparseFrame(int argc, char** argv) {
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    struct common_info_struct common_obj;
    memset(&common_obj, 0, sizeof common_obj);
    struct common_info_struct* common = &common_obj;
    struct gpu_info_struct* gpu_list = nullptr;
    struct matrix_info_struct* matrices = nullptr;

    double t0 = now();
    const int rc_gpu = SparseFrame_allocate_gpu(common, &gpu_list);
    const int nmat = argc > 1 ? argc - 1 : 0;
    common->numSparseMatrix = nmat;
    const int nthreads = std::min(2 /* MATRIX_THREAD_NUM */, nmat);
    common->matrixThreadNum = nthreads;
    printf("Num of matrices = %d\n\n", nmat);
    if (rc_gpu) {
        fprintf(stderr, "SparseFrame: SparseFrame_allocate_gpu failed (%d): no HIP device, and this library has no CPU path\n", rc_gpu);
        return nmat > 0 ? nmat : 1;
    }
    if (SparseFrame_allocate_matrix(common, &matrices)) { SparseFrame_free_gpu(common, &gpu_list); return nmat > 0 ? nmat : 1; }
    common->allocateTime = now() - t0;
    printf("Allocate time:        %lf\n\n", common->allocateTime);

    t0 = now();
    std::atomic<int> next{0}, failed{0};
    std::mutex print_mu;
    auto worker = [&](int thread_index) {
        struct matrix_info_struct* mi = matrices + thread_index;
        for (int k = next.fetch_add(1); k < nmat; k = next.fetch_add(1)) {
            mi->serial = k;
            SparseFrame_initialize_matrix(mi);
            const char* path = argv[1 + k];
            mi->path = path;
            const char* stage = nullptr;
            int rc = SparseFrame_read_matrix(mi);
            if (rc) stage = "read_matrix";
            if (!rc && (rc = SparseFrame_analyze(common, mi))) stage = "analyze";
            if (!rc && (rc = SparseFrame_factorize(common, gpu_list, mi))) stage = "factorize";
            const double tv0 = now();
            if (!rc && (rc = SparseFrame_validate(mi))) stage = "validate";
            const double tv1 = now();
            const double tr = mi->readTime, ta = mi->analyzeTime, tf = mi->factorizeTime, ts = mi->solveTime;
            const double res = (double)mi->residual;
            SparseFrame_cleanup_matrix(mi);
            if (getenv("SF_TRACE"))
                fprintf(stderr, "[sparseframe-hip] driver: validate %.1f ms (solve %.1f ms inside), cleanup %.1f ms\n",
                        (tv1 - tv0) * 1e3, ts * 1e3, (now() - tv1) * 1e3);
            const char* base = strrchr(path, '/');
            base = base ? base + 1 : path;
            std::lock_guard<std::mutex> g(print_mu);
            if (rc) {
                ++failed;
                fprintf(stderr, "SparseFrame: %s: SparseFrame_%s failed with code %d\n", base, stage, rc);
                continue;
            }
            printf("Matrix name:    %s\n", base);
            printf("Read time:      %lf\n", tr);
            printf("Analyze time:   %lf\n", ta);
            printf("Factorize time: %lf\n", tf);
            printf("Solve time:     %lf\n", ts);
            printf("residual (|Ax-b|)/(|A||x|+|b|): %le\n\n", res);
        }
    };
    {
        std::vector<std::thread> th;
        for (int t = 1; t < nthreads; ++t) th.emplace_back(worker, t);
        if (nthreads > 0) worker(0);
        for (auto& x : th) x.join();
    }
    common->computeTime = now() - t0;
    printf("Total computing time: %lf\n\n", common->computeTime);

    t0 = now();
    SparseFrame_free_gpu(common, &gpu_list);
    SparseFrame_free_matrix(common, &matrices);
    common->freeTime = now() - t0;
    printf("Free time:            %lf\n\n", common->freeTime);
    fflush(stdout);
    return failed.load();
}
