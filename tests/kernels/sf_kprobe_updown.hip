// Test-only probe of the update / downdate launchers (csrc/sf_updown.hip; built by tests/test_kernels_updown.py with the hipcc
// line of tests/kernels/Makefile): ONE launch on a host image of a double arena that holds every double operand -- the panel, the
// block of W, the rotation pairs.  The image goes to the device, the launcher runs once, the image comes back.  No numerical logic
// lives here; tests/updown_ref.py and the test module do the rest.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "sf_kernels.h"

namespace {

struct Image {
    double* d = nullptr;
    int* info = nullptr;
    int32_t* rows = nullptr;
    hipError_t rc = hipSuccess;
    Image(const double* h, int64_t count) {
        rc = hipMalloc((void**)&d, (size_t)count * sizeof(double));
        if (rc == hipSuccess) rc = hipMemcpy(d, h, (size_t)count * sizeof(double), hipMemcpyHostToDevice);
    }
    ~Image() {
        (void)hipFree(d);
        (void)hipFree(info);
        (void)hipFree(rows);
    }
    int finish(double* h, int64_t count) {
        if (rc == hipSuccess) rc = hipGetLastError();
        if (rc == hipSuccess) rc = hipDeviceSynchronize();
        if (rc == hipSuccess) rc = hipMemcpy(h, d, (size_t)count * sizeof(double), hipMemcpyDeviceToHost);
        return (int)rc;
    }
};

}  // namespace

// offsets in doubles into the image; *info goes in and comes back
extern "C" int kp_updown_diag(double* img, int64_t count, int64_t offD, int64_t ld, int b, int kw, int sign, int64_t offW, int64_t col0,
                              int64_t offRot, int* info) {
    Image m(img, count);
    if (m.rc == hipSuccess) m.rc = hipMalloc((void**)&m.info, sizeof(int));
    if (m.rc == hipSuccess) m.rc = hipMemcpy(m.info, info, sizeof(int), hipMemcpyHostToDevice);
    if (m.rc != hipSuccess) return (int)m.rc;
    sf::launch_updown_diag(m.d + offD, ld, b, kw, sign, m.d + offW, col0, m.d + offRot, m.info, nullptr);
    const int rc = m.finish(img, count);
    if (rc) return rc;
    return (int)hipMemcpy(info, m.info, sizeof(int), hipMemcpyDeviceToHost);
}

extern "C" int kp_updown_rows(double* img, int64_t count, int64_t offP, int64_t ld, int b, int64_t nrows, const int32_t* rows, int kw,
                              int sign, int64_t offW, int64_t offRot) {
    Image m(img, count);
    const int64_t nr = nrows > 0 ? nrows : 1;
    if (m.rc == hipSuccess) m.rc = hipMalloc((void**)&m.rows, (size_t)nr * sizeof(int32_t));
    if (m.rc == hipSuccess && nrows > 0) m.rc = hipMemcpy(m.rows, rows, (size_t)nrows * sizeof(int32_t), hipMemcpyHostToDevice);
    if (m.rc != hipSuccess) return (int)m.rc;
    sf::launch_updown_rows(m.d + offP, ld, b, nrows, m.rows, kw, sign, m.d + offW, m.d + offRot, nullptr);
    return m.finish(img, count);
}
