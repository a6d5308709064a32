// Test-only probe of the adjoint launchers (csrc/sf_adjoint.hip; built by tests/test_kernels_adjoint.py with the hipcc line of
// tests/kernels/Makefile): ONE launch on a host image of a double arena that holds every double operand -- the blocks Y and X, the
// arena of Sigma, the unmapped result, the output.  The image and the index arrays go to the device, the launcher runs once, the
// image (kp_adj_index: the two index outputs) comes back.  No numerical logic lives here; tests/adjoint_ref.py and the test module
// do the rest.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "sf_kernels.h"

namespace {

// device copies of the host arrays of one call, freed together
struct Dev {
    void* ptrs[12];
    int used = 0;
    hipError_t rc = hipSuccess;
    ~Dev() {
        for (int k = 0; k < used; ++k) (void)hipFree(ptrs[k]);
    }
    // `count` elements of h on the device (one at least); h == nullptr: a null pointer
    template <class T>
    T* put(const T* h, int64_t count) {
        if (!h || rc != hipSuccess) return nullptr;
        T* d = nullptr;
        rc = hipMalloc((void**)&d, (size_t)(count > 0 ? count : 1) * sizeof(T));
        if (rc != hipSuccess) return nullptr;
        ptrs[used++] = d;
        if (count > 0) rc = hipMemcpy(d, h, (size_t)count * sizeof(T), hipMemcpyHostToDevice);
        return d;
    }
    template <class T>
    void get(T* h, const T* d, int64_t count) {
        if (rc == hipSuccess && count > 0) rc = hipMemcpy(h, d, (size_t)count * sizeof(T), hipMemcpyDeviceToHost);
    }
    void ran() {
        if (rc == hipSuccess) rc = hipGetLastError();
        if (rc == hipSuccess) rc = hipDeviceSynchronize();
    }
};

}  // namespace

// col / mark: `room` >= count elements each, pre-filled by the caller; they go up and come back whole
extern "C" int kp_adj_index(const int64_t* ptr, const int32_t* idx, int32_t n, int64_t count, int side, const int64_t* mapA,
                            const int64_t* mapB, int32_t* col, uint8_t* mark, int64_t room) {
    Dev v;
    const int64_t* d_ptr = v.put(ptr, (int64_t)n + 1);
    const int32_t* d_idx = v.put(idx, count);
    const int64_t* d_a = v.put(mapA, count);
    const int64_t* d_b = v.put(mapB, count);
    int32_t* d_col = v.put(col, room);
    uint8_t* d_mark = v.put(mark, room);
    if (v.rc != hipSuccess) return (int)v.rc;
    sf::launch_adj_index(d_ptr, d_idx, n, count, side, d_a, d_b, d_col, d_mark, nullptr);
    v.ran();
    v.get(col, d_col, room);
    v.get(mark, d_mark, room);
    return (int)v.rc;
}

// offsets in doubles into the image; perm: nperm entries or null
extern "C" int kp_adj_values(double* img, int64_t total, const int32_t* idx, const int32_t* col, const uint8_t* mark, int64_t count,
                             const int32_t* perm, int64_t nperm, int k, int64_t offY, int64_t ldy, int64_t offX, int64_t ldx, double alpha,
                             int64_t offOut) {
    Dev v;
    double* d = v.put(img, total);
    const int32_t* d_idx = v.put(idx, count);
    const int32_t* d_col = v.put(col, count);
    const uint8_t* d_mark = v.put(mark, count);
    const int32_t* d_perm = v.put(perm, nperm);
    if (v.rc != hipSuccess) return (int)v.rc;
    sf::launch_adj_values(d_idx, d_col, d_mark, count, d_perm, k, d + offY, ldy, d + offX, ldx, alpha, d + offOut, nullptr);
    v.ran();
    v.get(img, d, total);
    return (int)v.rc;
}

extern "C" int kp_adj_logdet(double* img, int64_t total, const int64_t* mapA, int64_t shiftA, const int64_t* mapB, int64_t shiftB,
                             const uint8_t* mark, int twice, int64_t count, int64_t offS, double alpha, int64_t offOut) {
    Dev v;
    double* d = v.put(img, total);
    const int64_t* d_a = v.put(mapA, count);
    const int64_t* d_b = v.put(mapB, count);
    const uint8_t* d_mark = v.put(mark, count);
    if (v.rc != hipSuccess) return (int)v.rc;
    sf::launch_adj_logdet(d_a, shiftA, d_b, shiftB, d_mark, twice, count, d + offS, alpha, d + offOut, nullptr);
    v.ran();
    v.get(img, d, total);
    return (int)v.rc;
}

extern "C" int kp_adj_scatter(double* img, int64_t total, const int64_t* sptr, const int64_t* list, int64_t nsrc, int64_t nlist,
                              int64_t offTmp, int64_t offOut) {
    Dev v;
    double* d = v.put(img, total);
    const int64_t* d_sptr = v.put(sptr, nsrc + 1);
    const int64_t* d_list = v.put(list, nlist);
    if (v.rc != hipSuccess) return (int)v.rc;
    sf::launch_adj_scatter(d_sptr, d_list, nsrc, d + offTmp, d + offOut, nullptr);
    v.ran();
    v.get(img, d, total);
    return (int)v.rc;
}
