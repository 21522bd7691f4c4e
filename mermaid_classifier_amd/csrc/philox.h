// philox.h -- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the dropout masks made from
// it, for the device and the host alike.  A mask is a pure function of (seed, step, site, element): no state, no stored mask, no
// dependence on the grid, the tile, the chunking or the group (include/mmc.h, "regularisers").
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MMC_PHILOX_HD __host__ __device__ __forceinline__
#else
#define MMC_PHILOX_HD inline
#endif

// out = Philox4x32-10(counter c, key k): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85; a round is
// c' = [hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)], the key bumped after each of the ten rounds.
MMC_PHILOX_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// what a launch needs to make the masks of one site of one member at one step
struct DropMask {
    uint32_t thresh;   // (uint32)floor(p 2^32), made in double on the host; 0 = nothing is dropped
    uint32_t k0, k1;   // lo32(seed), hi32(seed)
    uint32_t step;     // lo32 of the trainer's Adam step count before this step
    uint32_t site;     // 0: the input; l: the output of layer l - 1
    float scale;       // (float)(1.0 / (1.0 - p))
};

// element e = m N + n (64 bit; N the unpadded width of the site) is kept iff word 0 of Philox(counter (lo e, hi e, step, site)) >= thresh
MMC_PHILOX_HD bool dropout_keep(const DropMask& d, uint64_t e)
{
    uint32_t x[4];
    philox4x32_10((uint32_t)e, (uint32_t)(e >> 32), d.step, d.site, d.k0, d.k1, x);
    return x[0] >= d.thresh;
}
