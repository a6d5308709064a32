// Test-only probe of the row-modification launchers (csrc/sf_rowmod.hip; built by tests/test_kernels_rowmod.py with the hipcc
// line of tests/kernels/Makefile): ONE launch on a host image of a double arena that holds every double operand -- the panel, the
// block of W, the sweep's y.  The image goes to the device, the launcher runs once, the image comes back.  No numerical logic
// lives here; tests/rowmod_ref.py and the test module do the rest.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "sf_kernels.h"

namespace {

struct Image {
    double* d = nullptr;
    int* info = nullptr;
    int32_t* rows = nullptr;
    int64_t* tasks = nullptr;
    hipError_t rc = hipSuccess;
    Image(const double* h, int64_t count) {
        rc = hipMalloc((void**)&d, (size_t)count * sizeof(double));
        if (rc == hipSuccess) rc = hipMemcpy(d, h, (size_t)count * sizeof(double), hipMemcpyHostToDevice);
    }
    ~Image() {
        (void)hipFree(d);
        (void)hipFree(info);
        (void)hipFree(rows);
        (void)hipFree(tasks);
    }
    void put_rows(const int32_t* h, int64_t nrows) {
        const int64_t nr = nrows > 0 ? nrows : 1;
        if (rc == hipSuccess) rc = hipMalloc((void**)&rows, (size_t)nr * sizeof(int32_t));
        if (rc == hipSuccess && nrows > 0) rc = hipMemcpy(rows, h, (size_t)nrows * sizeof(int32_t), hipMemcpyHostToDevice);
    }
    void put_info(const int* h) {
        if (rc == hipSuccess) rc = hipMalloc((void**)&info, sizeof(int));
        if (rc == hipSuccess) rc = hipMemcpy(info, h, sizeof(int), hipMemcpyHostToDevice);
    }
    int finish(double* h, int64_t count, int* h_info = nullptr) {
        if (rc == hipSuccess) rc = hipGetLastError();
        if (rc == hipSuccess) rc = hipDeviceSynchronize();
        if (rc == hipSuccess) rc = hipMemcpy(h, d, (size_t)count * sizeof(double), hipMemcpyDeviceToHost);
        if (rc == hipSuccess && h_info) rc = hipMemcpy(h_info, info, sizeof(int), hipMemcpyDeviceToHost);
        return (int)rc;
    }
};

}  // namespace

// offsets in doubles into the image; *flag / *info go in and come back
extern "C" int kp_rowmod_zero_rows(double* img, int64_t count, const int64_t* tasks, int64_t ntasks, int64_t one_off, int check, int* flag) {
    Image m(img, count);
    const int64_t nt = ntasks > 0 ? ntasks : 1;
    if (m.rc == hipSuccess) m.rc = hipMalloc((void**)&m.tasks, (size_t)nt * 3 * sizeof(int64_t));
    if (m.rc == hipSuccess && ntasks > 0) m.rc = hipMemcpy(m.tasks, tasks, (size_t)ntasks * 3 * sizeof(int64_t), hipMemcpyHostToDevice);
    m.put_info(flag);
    if (m.rc != hipSuccess) return (int)m.rc;
    sf::launch_rowmod_zero_rows(m.d, m.tasks, ntasks, one_off, check, m.info, nullptr);
    return m.finish(img, count, flag);
}

extern "C" int kp_rowdel_column(double* img, int64_t count, int64_t offCol, int64_t nbelow, const int32_t* rows, int64_t offW) {
    Image m(img, count);
    m.put_rows(rows, nbelow);
    if (m.rc != hipSuccess) return (int)m.rc;
    sf::launch_rowdel_column(m.d + offCol, nbelow, m.rows, m.d + offW, nullptr);
    return m.finish(img, count);
}

extern "C" int kp_rowadd_sweep_diag(double* img, int64_t count, int64_t offD, int64_t ld, int b, int64_t offW, int64_t col0, int64_t offY) {
    Image m(img, count);
    if (m.rc != hipSuccess) return (int)m.rc;
    sf::launch_rowadd_sweep_diag(m.d + offD, ld, b, m.d + offW, col0, m.d + offY, nullptr);
    return m.finish(img, count);
}

extern "C" int kp_rowadd_sweep_rows(double* img, int64_t count, int64_t offP, int64_t ld, int b, int64_t nrows, const int32_t* rows,
                                    int32_t target, int64_t offW, int64_t offY) {
    Image m(img, count);
    m.put_rows(rows, nrows);
    if (m.rc != hipSuccess) return (int)m.rc;
    sf::launch_rowadd_sweep_rows(m.d + offP, ld, b, nrows, m.rows, target, m.d + offW, m.d + offY, nullptr);
    return m.finish(img, count);
}

extern "C" int kp_rowadd_column(double* img, int64_t count, int64_t offCol, int64_t nbelow, const int32_t* rows, int64_t offW, int64_t jrow,
                                int* info) {
    Image m(img, count);
    m.put_rows(rows, nbelow);
    m.put_info(info);
    if (m.rc != hipSuccess) return (int)m.rc;
    sf::launch_rowadd_column(m.d + offCol, nbelow, m.rows, m.d + offW, jrow, m.info, nullptr);
    return m.finish(img, count, info);
}
