// Owners of what a plan takes from the HIP runtime: a device block, the pinned ring, an event, a stream, a graph executable.
// Each is move-only, empty by default and gives back what it holds when it is destroyed or assigned to, so that a plan, a set-up
// that fails half way and a temporary all release through the same path.  An owner converts to the raw handle: code
// that reads p->d_x in a launch or in pointer arithmetic is written as for a raw pointer.
#pragma once
#include <hip/hip_runtime_api.h>
#include <sparseframe_hip.h>

#include <cstddef>

// The seam to the runtime's allocator (defined once, in sf_apply.hip; a host-only test program links its own).  The two mallocs
// return 0 or, with *ptr null and no error left behind in the runtime, non-zero.  They count the live blocks of each kind.
int sf_dev_malloc(void** ptr, size_t bytes);
void sf_dev_free(void* ptr);
int sf_host_malloc(void** ptr, size_t bytes);
void sf_host_free(void* ptr);

namespace sf {

template <class T>
class DevMem {
    T* ptr_ = nullptr;
    bool lent_ = false;     // the block is somebody else's: never freed here

public:
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : ptr_(o.ptr_), lent_(o.lent_) { o.release(); }
    DevMem& operator=(DevMem&& o) noexcept {        // frees what the target held
        if (this != &o) {
            reset();
            lent_ = o.lent_;
            ptr_ = o.release();
        }
        return *this;
    }
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { reset(); }

    operator T*() const { return ptr_; }
    T* get() const { return ptr_; }
    // `count` elements in place of what was held; SF_ERR_ALLOC leaves the owner empty and no error behind in the runtime
    int alloc(size_t count) {
        reset();
        return sf_dev_malloc((void**)&ptr_, count * sizeof(T)) ? SF_ERR_ALLOC : SF_OK;
    }
    void reset() {
        if (ptr_ && !lent_) sf_dev_free(ptr_);
        release();
    }
    T* release() {
        T* q = ptr_;
        ptr_ = nullptr, lent_ = false;
        return q;
    }
    void adopt(T* q) { reset(); ptr_ = q; }                 // q came from sf_dev_malloc and is freed here
    void lend(T* q) { reset(); ptr_ = q; lent_ = true; }    // q stays its lender's
};

// pinned host memory (the download ring)
class PinnedMem {
    double* ptr_ = nullptr;

public:
    PinnedMem() = default;
    PinnedMem(const PinnedMem&) = delete;
    PinnedMem& operator=(const PinnedMem&) = delete;
    ~PinnedMem() { reset(); }
    operator double*() const { return ptr_; }
    int alloc(size_t count) {
        reset();
        return sf_host_malloc((void**)&ptr_, count * sizeof(double)) ? SF_ERR_ALLOC : SF_OK;
    }
    void reset() {
        if (ptr_) sf_host_free(ptr_);
        ptr_ = nullptr;
    }
};

// An event, a stream or a graph executable.  hipEventCreate(e.put()) fills an owner; reset(h, false) holds a handle that is the
// caller's (the stream a plan was created on) and never destroys it.
template <class H, hipError_t (*Destroy)(H)>
class Handle {
    H h_ = nullptr;
    bool owned_ = true;

public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(o.h_), owned_(o.owned_) { o.h_ = nullptr; }
    Handle& operator=(Handle&& o) noexcept {
        if (this != &o) {
            reset(o.h_, o.owned_);
            o.h_ = nullptr;
        }
        return *this;
    }
    Handle(const Handle&) = delete;
    Handle& operator=(const Handle&) = delete;
    ~Handle() { reset(); }

    operator H() const { return h_; }
    void reset(H h = nullptr, bool owned = true) {
        if (h_ && owned_) (void)Destroy(h_);
        h_ = h, owned_ = owned;
    }
    H* put() { reset(); return &h_; }
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;

}   // namespace sf
