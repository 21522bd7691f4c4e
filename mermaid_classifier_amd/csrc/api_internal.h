// api_internal.h -- what the two host units of the C ABI (mmc_api.cpp: backbone, schedule, crop; mmc_head.cpp: calibrated head) share:
// the error plumbing, and the one thing the head asks of a backbone beyond include/mmc.h.
// (The host-only half of the backbone -- architecture tables, blob reader, weight layouts -- is backbone_pack.h: no HIP, and it
// reports through its own BlobError, so it needs nothing from here.)
// Library-internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mmc.h"
#include "device_mem.h"   // mmc_fail, HIP_TRY

template <class... A>
static inline int fail(int code, const char* fmt, A... args)
{
    return mmc_fail(code, fmt, args...);
}
#define KTRY(expr)                                                                                 \
    do {                                                                                           \
        int r_ = (expr);                                                                           \
        if (r_ != 0) return fail(MMC_ERR_HIP, "%s failed (%d: %s)", #expr, r_,                     \
                                 r_ > 0 ? hipGetErrorString((hipError_t)r_) : "unsupported shape"); \
    } while (0)

// the device a backbone lives on (mmc_classify_patches checks it against the head's)
int mmc_backbone_device(const mmc_backbone* bb);
