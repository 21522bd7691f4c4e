// device_mem.h -- the one place that owns device memory and reports HIP errors: HIP_TRY, DevBuf<T>, check_device.
// Host-only (the runtime API header, no device code); library-internal, not part of the C ABI.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mmc.h"

// sets the thread-local message mmc_last_error() returns and hands back `code` (defined in mmc_api.cpp)
int mmc_fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                                 \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return mmc_fail(MMC_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

struct HipAlloc {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void release(void* p) { (void)hipFree(p); }
};

// An owned device buffer of `cap` elements.  Every allocation carries kSlack bytes past the last element (vector tail reads stay in
// bounds, and a request for zero elements is never zero bytes).  Growing frees first -- hipFree blocks until whatever still reads
// the old block has finished, and the old and the new block are never held at once -- so the contents do not survive growth; after
// a failed allocation the buffer is empty.  To replace a block that must survive a failure, or whose rows move into the new one,
// build a local DevBuf, fill it, and swap or move-assign it into the member: an early return frees the new block and leaves the old
// one in place, success frees the old one once.
template <class T, class A = HipAlloc>
struct DevBuf {
    static constexpr size_t kSlack = 256;
    T* p = nullptr;
    int64_t cap = 0;   // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { reset(); swap(o); }
        return *this;
    }
    ~DevBuf() { reset(); }
    operator T*() const { return p; }
    void swap(DevBuf& o) noexcept
    {
        T* tp = p; p = o.p; o.p = tp;
        const int64_t tc = cap; cap = o.cap; o.cap = tc;
    }
    void reset()
    {
        if (p) A::release(p);
        p = nullptr; cap = 0;
    }
    // frees what is held, then allocates room for `count` elements; false (buffer empty, HIP's sticky error cleared, nothing
    // reported) when the allocation fails: for the callers that word their own MMC_ERR_NOMEM message
    bool alloc(int64_t count)
    {
        reset();
        void* q = nullptr;
        if (A::alloc(&q, (size_t)count * sizeof(T) + kSlack) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        p = static_cast<T*>(q); cap = count;
        return true;
    }
    // room for at least `count` elements: nothing happens when there is already, else free first and allocate
    int reserve(int64_t count)
    {
        if (count <= cap) return 0;
        reset();
        void* q = nullptr;
        HIP_TRY(A::alloc(&q, (size_t)count * sizeof(T) + kSlack));
        p = static_cast<T*>(q); cap = count;
        return 0;
    }
};

// the device ordinal of a create call: 0, or the error a creator returns
inline int check_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return mmc_fail(MMC_ERR_HIP, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return mmc_fail(MMC_ERR_ARG, "device %d out of range (%d visible)", device, ndev);
    return 0;
}
