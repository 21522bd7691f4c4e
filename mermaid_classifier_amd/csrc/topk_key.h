// topk_key.h -- the ordering key of every per-row class selection on the device (calibrate_topk_kernel and its relatives in
// k_generic.hip, cover_adapt_topk_kernel in cover.hip).  A probability is >= 0, so its fp32 bit pattern orders like its value;
// the 64-bit key (bits << 32) | (0xFFFFFFFF - class) therefore orders a row as the reference's stable descending sort does
// (score descending, equal scores in class order), and the keys of a row are distinct for every bit pattern, NaN included.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned long long topk_key(float v, int cls)
{
    return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)cls);
}
