// How v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 operands, unit scales) sums its 128 products and adds them to C, on gfx950:
// crafted operands for output (0, 0) against the exact sum (every product and sum below is exact in double).
//   E1  one product 448 x 448 and one product 2^e: which e survive next to the large product
//   E2  the same with 64 products 2^e: are small products dropped one by one or after being summed
//   E3  448 x 448 - 448 x 448 + 2^e: does cancellation bring the small product back
//   E4  C = 2^24 and one product 2^e: how the sum meets the accumulator
//   E5  128 random products per output, 256 outputs: error against the exact sum in units of 2^-24 sum|p|
// Build: hipcc -O3 --offload-arch=gfx950 -o mfma_f8_sum mfma_f8_sum.hip
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

__global__ void mfma_k(const uint8_t* A, const uint8_t* B, const float* C, float* D)   // A[16][128], B[128][16], C, D [16][16]
{
    const int l = threadIdx.x, r = l & 15, kb = l >> 4;
    union { uint8_t b[32]; v8i v; } a, bb;
    for (int e = 0; e < 32; ++e) {
        a.b[e] = A[r * 128 + 32 * kb + e];
        bb.b[e] = B[(32 * kb + e) * 16 + r];
    }
    f4 c;
    for (int i = 0; i < 4; ++i) c[i] = C[(4 * kb + i) * 16 + r];
    c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a.v, bb.v, c, 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
    for (int i = 0; i < 4; ++i) D[(4 * kb + i) * 16 + r] = c[i];
}

static double dec(uint8_t c)
{
    const int e = (c >> 3) & 15, m = c & 7;
    const double v = e == 0 ? ldexp((double)m, -9) : ldexp(8.0 + m, e - 10);
    return (c & 0x80) ? -v : v;
}
static uint8_t pow2(int x) { return x >= -6 ? (uint8_t)((x + 7) << 3) : (uint8_t)(1 << (x + 9)); }   // 2^x, -9 <= x <= 8

static uint8_t hA[16 * 128], hB[128 * 16], *dA, *dB;
static float hC[256], hD[256], *dC, *dD;
static void clear() { memset(hA, 0, sizeof hA); memset(hB, 0, sizeof hB); memset(hC, 0, sizeof hC); }
static void put(int i, int j, int k, uint8_t a, uint8_t b) { hA[i * 128 + k] = a; hB[k * 16 + j] = b; }
// the product 2^e at position k of output (0, 0), -18 <= e <= 16
static void put_pow(int k, int e, bool neg = false)
{
    const int x = e < -9 ? -9 : (e > 8 ? 8 : e), y = e - x;
    put(0, 0, k, pow2(x) | (neg ? 0x80 : 0), pow2(y));
}
static void go()
{
    hipMemcpy(dA, hA, sizeof hA, hipMemcpyHostToDevice); hipMemcpy(dB, hB, sizeof hB, hipMemcpyHostToDevice);
    hipMemcpy(dC, hC, sizeof hC, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(mfma_k, dim3(1), dim3(64), 0, 0, dA, dB, dC, dD);
    hipMemcpy(hD, dD, sizeof hD, hipMemcpyDeviceToHost);
}
static double exact(int i, int j)
{
    double s = hC[i * 16 + j];
    for (int k = 0; k < 128; ++k) s += dec(hA[i * 128 + k]) * dec(hB[k * 16 + j]);
    return s;
}

int main()
{
    hipMalloc(&dA, sizeof hA); hipMalloc(&dB, sizeof hB); hipMalloc(&dC, sizeof hC); hipMalloc(&dD, sizeof hD);
    const double P = 448.0 * 448.0;
    for (int pos = 0; pos < 2; ++pos) {
        printf("E1 448*448 at k = 0, 2^e at k = %d: D - 448*448 in units of 2^e, e = 16 .. -18\n  ", pos ? 127 : 1);
        for (int e = 16; e >= -18; --e) {
            clear(); put(0, 0, 0, 0x7E, 0x7E); put_pow(pos ? 127 : 1, e); go();
            printf(" %g", ((double)hD[0] - P) / ldexp(1.0, e));
        }
        printf("\n");
    }
    printf("E2 448*448 and 64 products 2^e (k = 1 .. 64): (D - 448*448) / (64 2^e), e = 10 .. -18\n  ");
    for (int e = 10; e >= -18; --e) {
        clear(); put(0, 0, 0, 0x7E, 0x7E);
        for (int k = 1; k <= 64; ++k) put_pow(k, e);
        go();
        printf(" %g", ((double)hD[0] - P) / ldexp(64.0, e));
    }
    printf("\nE3 448*448 - 448*448 + 2^e (k = 0, 1, 2): D / 2^e, e = 16 .. -18\n  ");
    for (int e = 16; e >= -18; --e) {
        clear(); put(0, 0, 0, 0x7E, 0x7E); put(0, 0, 1, 0xFE, 0x7E); put_pow(2, e); go();
        printf(" %g", (double)hD[0] / ldexp(1.0, e));
    }
    printf("\nE4 C = 2^24 and one product 2^e: (D - 2^24) / 2^e, e = 8 .. -8; then 3 products 2^e\n  ");
    for (int e = 8; e >= -8; --e) {
        clear(); hC[0] = 16777216.f; put_pow(0, e); go();
        printf(" %g", ((double)hD[0] - 16777216.0) / ldexp(1.0, e));
    }
    printf("\n  ");
    for (int e = 8; e >= -8; --e) {
        clear(); hC[0] = 16777216.f; put_pow(0, e); put_pow(1, e); put_pow(2, e); go();
        printf(" %g", ((double)hD[0] - 16777216.0) / ldexp(1.0, e));
    }
    printf("\nE5 random codes (all finite e4m3 values, both signs), C = 0: error vs the exact sum\n");
    srand(5);
    for (int trial = 0; trial < 4; ++trial) {
        clear();
        // trial 0, 1: full range; 2, 3: |codes| drawn the way a scaled row looks (one 448 per row, the rest mostly small)
        for (int i = 0; i < 16 * 128; ++i) {
            uint8_t a = (uint8_t)(rand() % 127), b = (uint8_t)(rand() % 127);
            if (trial >= 2) { a = (uint8_t)(rand() % 96); b = (uint8_t)(rand() % 110); }
            hA[i] = a | (rand() & 1 ? 0x80 : 0); hB[i] = b | (rand() & 1 ? 0x80 : 0);
        }
        if (trial >= 2) for (int i = 0; i < 16; ++i) { hA[i * 128 + rand() % 128] = 0x7E; hB[(rand() % 128) * 16 + i] = 0x7E; }
        go();
        double worst_rel = 0, worst_abs = 0, worst_ulp = 0, rms = 0, mean = 0;
        int inexact = 0;
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) {
                double s = 0, m = 0, pmax = 0;
                for (int k = 0; k < 128; ++k) {
                    const double p = dec(hA[i * 128 + k]) * dec(hB[k * 16 + j]);
                    s += p; m += fabs(p); if (fabs(p) > pmax) pmax = fabs(p);
                }
                const double err = (double)hD[i * 16 + j] - s;
                inexact += (float)s != hD[i * 16 + j];
                if (fabs(err) / m > worst_rel) worst_rel = fabs(err) / m;
                if (fabs(err) > worst_abs) worst_abs = fabs(err);
                int ex; frexp(pmax, &ex);
                const double u = fabs(err) / ldexp(1.0, ex - 1);          // in units of 2^floor(log2 max|p|)
                if (u > worst_ulp) worst_ulp = u;
                rms += err * err; mean += err;
            }
        printf("  trial %d: %3d of 256 differ from fp32(exact); max |err| %.4g, max |err| / sum|p| = %.1f x 2^-24, max |err| / 2^floor(log2 max|p|) = 2^%.1f, rms %.3g, mean %+.3g\n",
               trial, inexact, worst_abs, worst_rel / ldexp(1.0, -24), worst_ulp > 0 ? log2(worst_ulp) : -99.0, sqrt(rms / 256), mean / 256);
    }
    return 0;
}
