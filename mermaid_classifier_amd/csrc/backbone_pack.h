// backbone_pack.h -- the host-only half of the backbone: the architecture tables, the weights blob reader and every device weight
// layout as a pure function from natural fp32 tensors to a std::vector of the device image.  Nothing of HIP in here: mmc_api.cpp
// uploads the images and writes the pointers into the launch structs of kernels.h (one bind function per kernel family), and
// tests/host/pack_check.cpp walks every image in the order its kernel reads it, on the CPU.
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mmc.h"

// ------------------------------------------------------------------------------------------
// EfficientNet-B0 stage table (the published architecture; mirrors oracle/efficientnet_b0_ref.py)
// ------------------------------------------------------------------------------------------
struct BlockDef { int k, s, e, cin, cout; };
static const BlockDef B0_BLOCKS[16] = {
    {3, 1, 1, 32, 16},  {3, 2, 6, 16, 24},  {3, 1, 6, 24, 24},   {5, 2, 6, 24, 40},
    {5, 1, 6, 40, 40},  {3, 2, 6, 40, 80},  {3, 1, 6, 80, 80},   {3, 1, 6, 80, 80},
    {5, 1, 6, 80, 112}, {5, 1, 6, 112, 112}, {5, 1, 6, 112, 112}, {5, 2, 6, 112, 192},
    {5, 1, 6, 192, 192}, {5, 1, 6, 192, 192}, {5, 1, 6, 192, 192}, {3, 1, 6, 192, 320}};
// The published family: B0's stage table under compound scaling (widths to multiples of 8, never below 90 % of the scaled
// value; repeats rounded up).  B0 is the network the reference path runs; B4 (width 1.4, depth 1.8, BASELINE.json
// configs[4]) does not exist in the reference and runs on the generic per-layer kernels.
struct ArchDef { int stem = 32, head_in = 320, feat = 1280; std::vector<BlockDef> blocks; };
static inline int round_filters(int c, double width)
{
    const double v = c * width;
    int n = (int)(v + 4) / 8 * 8;
    if (n < 8) n = 8;
    if (n < 0.9 * v) n += 8;
    return n;
}
static inline ArchDef make_arch(int arch)
{
    ArchDef A;
    if (arch == MMC_ARCH_B0) {
        A.blocks.assign(B0_BLOCKS, B0_BLOCKS + 16);
        return A;
    }
    const double width = 1.4, depth = 1.8;   // MMC_ARCH_B4
    static const int STAGES[7][6] = {{1, 3, 1, 1, 32, 16},  {2, 3, 2, 6, 16, 24},   {2, 5, 2, 6, 24, 40}, {3, 3, 2, 6, 40, 80},
                                     {3, 5, 1, 6, 80, 112}, {4, 5, 2, 6, 112, 192}, {1, 3, 1, 6, 192, 320}};
    A.stem = round_filters(32, width);
    for (auto& st : STAGES) {
        const int cin = round_filters(st[4], width), cout = round_filters(st[5], width);
        const int reps = (int)std::ceil(depth * st[0] - 1e-9);
        for (int r = 0; r < reps; ++r) A.blocks.push_back({st[1], r == 0 ? st[2] : 1, st[3], r == 0 ? cin : cout, cout});
    }
    A.head_in = A.blocks.back().cout;
    A.feat = round_filters(1280, width);
    return A;
}
// Scaled activation domain (device_common.h, silu_scaled): every SiLU output is stored times log2(e).
// Producers (stem, expand, depthwise, head) get weights/bias times LOG2E, consumers times 1/LOG2E;
// for the depthwise taps the two cancel, so only its bias is scaled.
static const double LOG2E = 1.4426950408889634;

static inline void same_pad(int size, int k, int s, int* before, int* out)
{
    *out = (size + s - 1) / s;
    int pad = (*out - 1) * s + k - size;
    if (pad < 0) pad = 0;
    *before = pad / 2;
}

// fp32 -> OCP e4m3fn (4 exponent bits, bias 7, 3 mantissa bits, no infinities, largest finite 448), round to nearest even,
// saturating.  The device side uses v_cvt_pk_fp8_f32; the host needs the same encoding for the weights.
static inline uint8_t e4m3_encode(float x)
{
    if (x != x) return 0x7F;
    const uint8_t sign = std::signbit(x) ? 0x80 : 0x00;
    float a = std::fabs(x);
    if (a >= 448.0f) return sign | 0x7E;
    if (a < 0.0009765625f) return sign;                        // below half of the smallest subnormal (2^-9): zero (a tie goes to even = 0)
    int e;
    (void)std::frexp(a, &e);                                   // a = f * 2^e, f in [0.5, 1)
    int ex = e - 1;                                            // a in [2^ex, 2^(ex+1))
    if (ex < -6) ex = -6;                                      // subnormals share the exponent of the smallest normal
    const float quantum = std::ldexp(1.0f, ex - 3);
    float qf = std::nearbyint(a / quantum);                    // round to nearest even (default rounding mode)
    int qi = (int)qf;
    if (qi >= 16) { qi = 8; ++ex; }
    if (ex > 8) return sign | 0x7E;
    if (ex == 8 && qi > 14) return sign | 0x7E;                // 448 = 1.75 * 2^8 is the largest finite value
    if (qi < 8) return sign | (uint8_t)qi;                     // subnormal (only with ex == -6)
    return sign | (uint8_t)(((ex + 7) << 3) | (qi - 8));
}

// ------------------------------------------------------------------------------------------
// blob parsing: header{magic,version,arch,n_tensors} + table{offset,nbytes} + fp32 tensors
// ------------------------------------------------------------------------------------------
// why a blob was refused: an MMC_ERR_* code and the message for mmc_last_error()
struct BlobError {
    int code = MMC_OK;
    char msg[256] = "";
};
__attribute__((format(printf, 3, 4))) static inline int blob_fail(BlobError* err, int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    err->code = code;
    vsnprintf(err->msg, sizeof err->msg, fmt, ap);
    va_end(ap);
    return code;
}

struct BlobReader {
    const uint8_t* base = nullptr;
    size_t nbytes = 0;
    uint32_t n_tensors = 0;
    std::vector<uint64_t> table;   // {offset, nbytes} per tensor (copied out: the blob need not be 8-byte aligned)
    uint32_t next = 0;
    // header checks; copies the table
    int open(const void* packed, size_t bytes, int arch, BlobError* err)
    {
        if (!packed || bytes < 16) return blob_fail(err, MMC_ERR_WEIGHTS, "weights blob is empty");
        base = static_cast<const uint8_t*>(packed);
        nbytes = bytes;
        uint32_t hdr[4];
        memcpy(hdr, base, 16);
        if (memcmp(base, "MMCW", 4) != 0) return blob_fail(err, MMC_ERR_WEIGHTS, "bad magic in weights blob");
        if (hdr[1] != 1) return blob_fail(err, MMC_ERR_WEIGHTS, "weights blob version %u, expected 1", hdr[1]);
        if ((int)hdr[2] != arch) return blob_fail(err, MMC_ERR_WEIGHTS, "weights blob arch %u != requested %d", hdr[2], arch);
        n_tensors = hdr[3];
        if (16 + (size_t)n_tensors * 16 > nbytes) return blob_fail(err, MMC_ERR_WEIGHTS, "weights blob truncated (table)");
        table.resize(2 * (size_t)n_tensors);
        memcpy(table.data(), base + 16, (size_t)n_tensors * 16);
        next = 0;
        return MMC_OK;
    }
    const float* take(size_t n_floats, const char* what, BlobError* err)
    {
        if (next >= n_tensors) { blob_fail(err, MMC_ERR_WEIGHTS, "weights blob ended before %s", what); return nullptr; }
        const uint64_t off = table[2 * next], nb = table[2 * next + 1];
        if (off > nbytes || nb > nbytes - off || nb != n_floats * sizeof(float)) {   // (no off + nb: a hostile offset would wrap it)
            blob_fail(err, MMC_ERR_WEIGHTS, "tensor %u (%s): expected %zu bytes, blob has %llu", next, what, n_floats * sizeof(float),
                      (unsigned long long)nb);
            return nullptr;
        }
        ++next;
        return reinterpret_cast<const float*>(base + off);
    }
};

// The tensors of a blob in their natural shapes: views into the caller's blob, nothing copied
struct RawBlock {
    const float *exp_w = nullptr, *exp_b = nullptr;   // [ce][cin], [ce]; null when the block has no expand conv (e == 1)
    const float *dw_w = nullptr, *dw_b = nullptr;     // [ce][k][k], [ce]
    const float *se_wr = nullptr, *se_br = nullptr;   // [cs][ce], [cs]
    const float *se_we = nullptr, *se_be = nullptr;   // [ce][cs], [ce]
    const float *proj_w = nullptr, *proj_b = nullptr; // [cout][ce], [cout]
};
struct RawNet {
    const float *stem_w = nullptr, *stem_b = nullptr, *stem_pad = nullptr;   // [stem][27] folded (ky,kx,c), [stem], [3]
    std::vector<RawBlock> blk;
    const float *head_w = nullptr, *head_b = nullptr;                        // [feat][head_in], [feat]
};
static inline int se_width(const BlockDef& d) { return d.cin / 4 > 1 ? d.cin / 4 : 1; }

// Walks the fixed tensor order of architecture A: stem w / b / padval; per block expand w / b (when e != 1), dw w / b,
// se wr / br / we / be, project w / b; head w / b.  `rd`: a reader whose open() passed.
static inline int read_blob(BlobReader& rd, const ArchDef& A, RawNet* net, BlobError* err)
{
    // the next tensor of the table, which must hold n floats; false (err filled) when it does not
    auto take = [&](const float*& dst, size_t n, const char* what) { return (dst = rd.take(n, what, err)) != nullptr; };
    if (!take(net->stem_w, (size_t)A.stem * 27, "stem.weight") || !take(net->stem_b, (size_t)A.stem, "stem.bias") ||
        !take(net->stem_pad, 3, "stem.padval"))
        return err->code;
    net->blk.assign(A.blocks.size(), RawBlock{});
    for (size_t i = 0; i < A.blocks.size(); ++i) {
        const BlockDef& d = A.blocks[i];
        RawBlock& R = net->blk[i];
        const size_t ce = (size_t)d.cin * d.e, cs = (size_t)se_width(d);
        char nm[64];
        snprintf(nm, sizeof nm, "b%d.expand", (int)i);
        if (d.e != 1 && (!take(R.exp_w, ce * d.cin, nm) || !take(R.exp_b, ce, nm))) return err->code;
        snprintf(nm, sizeof nm, "b%d.dw", (int)i);
        if (!take(R.dw_w, ce * d.k * d.k, nm) || !take(R.dw_b, ce, nm)) return err->code;
        snprintf(nm, sizeof nm, "b%d.se", (int)i);
        if (!take(R.se_wr, cs * ce, nm) || !take(R.se_br, cs, nm) || !take(R.se_we, ce * cs, nm) || !take(R.se_be, ce, nm)) return err->code;
        snprintf(nm, sizeof nm, "b%d.project", (int)i);
        if (!take(R.proj_w, (size_t)d.cout * ce, nm) || !take(R.proj_b, (size_t)d.cout, nm)) return err->code;
    }
    if (!take(net->head_w, (size_t)A.feat * A.head_in, "head.weight") || !take(net->head_b, (size_t)A.feat, "head.bias")) return err->code;
    if (rd.next != rd.n_tensors)
        return blob_fail(err, MMC_ERR_WEIGHTS, "weights blob has %u tensors, expected %u", rd.n_tensors, rd.next);
    return MMC_OK;
}

// ------------------------------------------------------------------------------------------
// layouts: natural fp32 tensors -> the device image
// ------------------------------------------------------------------------------------------
// b[0 .. n) times `scale`, zero padded to `padded` floats
static inline std::vector<float> pack_bias(const float* b, int n, int padded, double scale)
{
    std::vector<float> v((size_t)padded, 0.f);
    for (int c = 0; c < n; ++c) v[c] = (float)(b[c] * scale);
    return v;
}

// A 1x1 convolution packed for pw_gemm_kernel
struct PwImage {
    int N = 0, K = 0, Kp = 0, nt = 0, n_chunks = 0;
    std::vector<_Float16> w;   // [n_chunks*16*nt][Kp]
    std::vector<float> b;      // [n_chunks*16*nt]
};
// Pack a natural [N][K] fp32 1x1-conv weight into the fragment-ordered fp16 layout of pw_gemm_kernel:
// fragment (chunk, kstep, t) = 1 KB at ((chunk*KS32 + kstep)*nt + t)*512 halves; inside it lane
// (q*16 + m) holds W[channel(chunk, t, m)][kstep*32 + q*8 .. +8], with the row permutation
// fragment row (t*16 + 4qr + jr) <- channel (chunk*16nt + qr*4nt + 4t + jr).
static inline PwImage pack_pw(const float* w, const float* b, int N, int K, int nt, double wscale, double bscale)
{
    PwImage L;
    L.N = N;
    L.K = K;
    L.Kp = (K + 31) / 32 * 32;
    L.nt = nt;
    const int cw = 16 * L.nt;
    L.n_chunks = (N + cw - 1) / cw;
    const int Np = L.n_chunks * cw;
    const int ks32 = L.Kp / 32;
    L.w.assign((size_t)Np * L.Kp, (_Float16)0.0f);
    for (int ch = 0; ch < L.n_chunks; ++ch)
        for (int ks = 0; ks < ks32; ++ks)
            for (int t = 0; t < L.nt; ++t)
                for (int m = 0; m < 16; ++m) {
                    const int c = ch * cw + (m >> 2) * 4 * L.nt + 4 * t + (m & 3);
                    if (c >= N) continue;
                    for (int q = 0; q < 4; ++q)
                        for (int j = 0; j < 8; ++j) {
                            const int k = ks * 32 + q * 8 + j;
                            if (k >= K) continue;
                            const size_t off = ((((size_t)ch * ks32 + ks) * L.nt + t) * 64 + (q * 16 + m)) * 8 + j;
                            L.w[off] = (_Float16)(float)(w[(size_t)c * K + k] * wscale);
                        }
                }
    L.b = pack_bias(b, N, Np, bscale);
    return L;
}

// W[n][k] (rows of ld elements, n < N, k < K) times `scale` as fp16 in MFMA fragment order [nf][ks][64 lanes][8]: element (n, k)
// at ((n/16 * ks + k/32) * 64 + (k%32)/8 * 16 + n%16) * 8 + k%8 -- lane (q*16 + m) of fragment (f, kstep) holds
// W[16f + m][32 kstep + 8q .. +8].  Fragments and k-steps beyond the tensor stay zero.  (A source already in fp16 is only
// permuted: the expand weights keep the rounding of their natural fp16 rows.)
template <typename T>
static inline std::vector<_Float16> pack_frag(const T* w, int N, int K, int ld, int nf, int ks, double scale)
{
    std::vector<_Float16> wf((size_t)nf * ks * 512, (_Float16)0.0f);
    for (int c = 0; c < N; ++c)
        for (int k = 0; k < K; ++k)
            wf[((((size_t)(c / 16) * ks + k / 32) * 64) + ((k % 32) / 8) * 16 + (c % 16)) * 8 + (k % 8)] =
                (_Float16)(float)(w[(size_t)c * ld + k] * scale);
    return wf;
}

// The stem conv, [C][27] folded (ky,kx,c), as C/16 MFMA A fragments of K = 32: row (t*16 + 4q + j) <- channel q*4*(C/16) + 4t + j
// (lane quarter q owns channels q*4*snt + 4t + j); in a row, kernel row qq's first 8 of its 9 values at [8 qq .. +8], the three
// ninth values at [24 .. 27), the rest zero.
static inline std::vector<_Float16> pack_stem(const float* w, int C)
{
    const int snt = C / 16;   // output fragments
    std::vector<_Float16> wp((size_t)C * 32, (_Float16)0.0f);
    for (int t = 0; t < snt; ++t)
        for (int q = 0; q < 4; ++q)
            for (int j = 0; j < 4; ++j) {
                const int prow = t * 16 + 4 * q + j;
                const int c = q * 4 * snt + 4 * t + j;
                const float* wc = w + (size_t)c * 27;
                for (int qq = 0; qq < 3; ++qq)           // kernel row qq, bytes 0..7 of its 9-byte run
                    for (int jj = 0; jj < 8; ++jj) wp[prow * 32 + qq * 8 + jj] = (_Float16)(float)(wc[qq * 9 + jj] * LOG2E);
                for (int jj = 0; jj < 3; ++jj) wp[prow * 32 + 24 + jj] = (_Float16)(float)(wc[jj * 9 + 8] * LOG2E);
            }
    return wp;
}

// Expand weights [ce][cin] times log2(e) as natural fp16 rows of kp >= cin elements, K zero padded (mbconv_a / mbconv_d; the source of
// the fragment-ordered and K-permuted copies, which keep this rounding)
static inline std::vector<_Float16> pack_expand_rows(const float* w, int ce, int cin, int kp)
{
    std::vector<_Float16> wn((size_t)ce * kp, (_Float16)0.0f);
    for (int c = 0; c < ce; ++c)
        for (int k = 0; k < cin; ++k) wn[(size_t)c * kp + k] = (_Float16)(float)(w[(size_t)c * cin + k] * LOG2E);
    return wn;
}

// K-permuted copy of block 1's expand rows `wn` ([ce][kp], 16 input channels) for block 0's folded project: MFMA slot 8q+j holds
// input channel 4q+j (j < 4), the rest zero -- the layout block 0's in-kernel project leaves in the lanes
static inline std::vector<_Float16> pack_expand_kperm(const _Float16* wn, int ce, int kp)
{
    std::vector<_Float16> wq((size_t)ce * 32, (_Float16)0.0f);
    for (int c = 0; c < ce; ++c)
        for (int qq = 0; qq < 4; ++qq)
            for (int j = 0; j < 4; ++j) wq[(size_t)c * 32 + 8 * qq + j] = wn[(size_t)c * kp + 4 * qq + j];
    return wq;
}

// Depthwise taps [ce][k][k] times `tsc`, tap-major fp32 [k*k][ce].
// The taps see a log2(e)-scaled input (stem or expand output) and produce a scaled output: the factors cancel (tsc 1) --
// except for an expand-less block fed by a project conv (B4's block 1), whose input is in the plain domain (tsc log2 e)
static inline std::vector<float> pack_dw_taps(const float* w, int ce, int k, double tsc)
{
    const int kk = k * k;
    std::vector<float> wt((size_t)kk * ce);
    for (int c = 0; c < ce; ++c)
        for (int t = 0; t < kk; ++t) wt[(size_t)t * ce + c] = (float)(w[(size_t)c * kk + t] * tsc);
    return wt;
}

// taps of tail7_kernel / mid14_kernel / mbt_kernel as fp16 pairs [15][ce]: kernel row ky = (k0,k1), (k2,k3), (k4,0); the kernel derives the
// odd-output pairs by shifts, giving the same values as mbconv_d_kernel's wl2 table
static inline std::vector<uint32_t> pack_dw_pairs(const float* w, int ce, int k)
{
    const int kk = k * k;
    std::vector<uint32_t> dp((size_t)15 * ce, 0u);
    auto tap = [&](int c, int ky, int kx) -> _Float16 {
        return kx < k ? (_Float16)w[(size_t)c * kk + ky * k + kx] : (_Float16)0.0f;
    };
    for (int c = 0; c < ce; ++c)
        for (int ky = 0; ky < k; ++ky)
            for (int d = 0; d < 3; ++d) {   // slot 3*ky + d holds taps (2d, 2d+1) of kernel row ky
                _Float16 h[2] = {tap(c, ky, 2 * d), tap(c, ky, 2 * d + 1)};
                uint32_t u;
                memcpy(&u, h, 4);
                dp[(size_t)(ky * 3 + d) * ce + c] = u;
            }
    return dp;
}

// the same 15 dwords `dp` + the bias `db` (as the 16th, exactly as the fp32 bias buffer holds it) in 16-byte requests: [4][ce][4] --
// request j of channel c holds slots 4j .. 4j+3; a wave's request is 1 KB contiguous (16 dword loads per thread were 16
// wave-instructions of 256 bytes)
static inline std::vector<uint32_t> pack_dw_requests(const uint32_t* dp, const float* db, int ce)
{
    std::vector<uint32_t> dp4((size_t)16 * ce, 0u);
    for (int c = 0; c < ce; ++c)
        for (int t = 0; t < 16; ++t) {
            uint32_t v = 0u;
            if (t < 15) v = dp[(size_t)t * ce + c];
            else memcpy(&v, &db[c], 4);
            dp4[((size_t)(t / 4) * ce + c) * 4 + (t % 4)] = v;
        }
    return dp4;
}

// Depthwise on the matrix pipe (v_mfma_f32_4x4x4_16B_f16: 16 independent blocks = 16 channels), [ce/16][k][2][64][4].  A operand
// of block c, kernel row ky, input quad h (columns x0 - 2 + 4h .. +3 of an output tile x0 .. x0+3): the Toeplitz slice
// A[i][k] = w[c][ky][k - i + 4h - 2 + R] (zero outside 0 .. K-1), lane 4 blk + i holding k = 0 .. 3, block blk = channel
// 2 (blk & 3) + ((blk >> 2) & 1) + 8 (blk >> 3) of the group (channels 2k, 2k+1 in neighbouring 16-lane rows: the kernel
// pairs them with v_permlane16_swap).
static inline std::vector<_Float16> pack_dw_toeplitz(const float* w, int ce, int K, double tsc)
{
    const int kk = K * K, R = K / 2, ngr = ce / 16;
    std::vector<_Float16> dd((size_t)ngr * K * 2 * 64 * 4, (_Float16)0.0f);
    for (int g = 0; g < ngr; ++g)
        for (int ky = 0; ky < K; ++ky)
            for (int h = 0; h < 2; ++h)
                for (int ln = 0; ln < 64; ++ln) {
                    const int blk = ln >> 2, ii = ln & 3;
                    const int cc = 2 * (blk & 3) + ((blk >> 2) & 1) + 8 * (blk >> 3);
                    for (int k = 0; k < 4; ++k) {
                        const int t = k - ii + 4 * h - 2 + R;
                        if (t < 0 || t >= K) continue;
                        dd[((((size_t)g * K + ky) * 2 + h) * 64 + ln) * 4 + k] = (_Float16)(float)(w[(size_t)(16 * g + cc) * kk + ky * K + t] * tsc);
                    }
                }
    return dd;
}

// Squeeze-excite weights, fp32 in MFMA fragment order (se_fused_kernel): 3 output/k fragments of 16 cover Cs <= 48; [ce/16][3][64][4]
// (+ 4 floats of tail).  FC1: element e of lane (q*16 + i) of fragment (g, t) = Wr[16t + i][16g + 4q + e] times psc
static inline std::vector<float> pack_se_fc1_frag(const float* wr, int ce, int cs, double psc)
{
    const int ng = ce / 16;
    std::vector<float> wrp((size_t)ng * 3 * 64 * 4 + 4, 0.f);
    for (int g = 0; g < ng; ++g)
        for (int t = 0; t < 3; ++t)
            for (int ln = 0; ln < 64; ++ln)
                for (int e = 0; e < 4; ++e) {
                    const int ii = ln & 15, qq = ln >> 4;
                    const size_t off = (((size_t)g * 3 + t) * 64 + ln) * 4 + e;
                    const int j = 16 * t + ii, c = 16 * g + 4 * qq + e;         // FC1: Wr[j][c]
                    if (j < cs) wrp[off] = (float)(wr[(size_t)j * ce + c] * psc);
                }
    return wrp;
}
// ... FC2: element e of lane (q*16 + i) of fragment (g, t) = We[16g + i][16t + 4q + e] (T = g, k-group = t)
static inline std::vector<float> pack_se_fc2_frag(const float* we, int ce, int cs)
{
    const int ng = ce / 16;
    std::vector<float> wep((size_t)ng * 3 * 64 * 4 + 4, 0.f);
    for (int g = 0; g < ng; ++g)
        for (int t = 0; t < 3; ++t)
            for (int ln = 0; ln < 64; ++ln)
                for (int e = 0; e < 4; ++e) {
                    const int ii = ln & 15, qq = ln >> 4;
                    const size_t off = (((size_t)g * 3 + t) * 64 + ln) * 4 + e;
                    const int n = 16 * g + ii, k = 16 * t + 4 * qq + e;         // FC2: We[n][k]
                    if (k < cs) wep[off] = we[(size_t)n * cs + k];
                }
    return wep;
}

// natural fp32 rows (se_small_kernel, se_wide_kernel): the squeeze FC [cs][ce] times psc
static inline std::vector<float> pack_se_fc1_nat(const float* wr, int ce, int cs, double psc)
{
    std::vector<float> wrn((size_t)cs * ce);
    for (size_t e = 0; e < wrn.size(); ++e) wrn[e] = (float)(wr[e] * psc);
    return wrn;
}
// ... se_wide_kernel reads the excite FC transposed, [Cs][C]: neighbouring lanes, neighbouring words
static inline std::vector<float> pack_se_fc2_t(const float* we, int ce, int cs)
{
    std::vector<float> wet((size_t)cs * ce);
    for (int c = 0; c < ce; ++c)
        for (int j = 0; j < cs; ++j) wet[(size_t)j * ce + c] = we[(size_t)c * cs + j];
    return wet;
}

// fp16, transposed for matrix-vector use: Wr^T [ce][csp], We^T [csp][ce] (csp = Cs padded to 4)
static inline std::vector<_Float16> pack_se_fc1_t16(const float* wr, int ce, int cs, int csp)
{
    std::vector<_Float16> wrt((size_t)ce * csp, (_Float16)0.0f);
    for (int c = 0; c < ce; ++c)
        for (int j = 0; j < cs; ++j) wrt[(size_t)c * csp + j] = (_Float16)wr[(size_t)j * ce + c];
    return wrt;
}
static inline std::vector<_Float16> pack_se_fc2_t16(const float* we, int ce, int cs, int csp)
{
    std::vector<_Float16> wet((size_t)csp * ce, (_Float16)0.0f);
    for (int c = 0; c < ce; ++c)
        for (int j = 0; j < cs; ++j) wet[(size_t)j * ce + c] = (_Float16)we[(size_t)c * cs + j];
    return wet;
}

// proj_patch_kernel's FC1 from Wr^T `wrt` ([ce][csp]): [group of four outputs][channel row][4] (ProjPatchArgs::wr_g) with `rows`
// (= proj_patch_fc1_rows(ce)) channel rows per group, zero beyond ce
static inline std::vector<_Float16> pack_se_fc1_groups(const _Float16* wrt, int ce, int csp, int rows)
{
    std::vector<_Float16> wrg((size_t)(csp / 4) * rows * 4, (_Float16)0.0f);
    for (int g = 0; g < csp / 4; ++g)
        for (int c = 0; c < ce; ++c)
            for (int e = 0; e < 4; ++e) wrg[((size_t)g * rows + c) * 4 + e] = wrt[(size_t)c * csp + 4 * g + e];
    return wrg;
}

// tail7_kernel's 16-byte request layout (TailBlock::wr_t / we_t): two rows of the transposed matrices per request.  The only shape:
// 1152 channels, SE width 48.  FC1 [18][384][8] from Wr^T `wrt` ([1152][48]): request p of thread (cr, j4) = Wr^T[64p + cr][4 j4 .. +3],
// Wr^T[64p + 32 + cr][4 j4 .. +3]
static inline std::vector<_Float16> pack_tail_fc1(const _Float16* wrt)
{
    const int csp = 48;
    std::vector<_Float16> wr2((size_t)18 * 384 * 8);
    for (int p = 0; p < 18; ++p)
        for (int t = 0; t < 384; ++t)
            for (int e = 0; e < 8; ++e) {
                const int cr = t / 12, j4 = t % 12, c = 64 * p + (e < 4 ? 0 : 32) + cr;
                wr2[((size_t)p * 384 + t) * 8 + e] = wrt[(size_t)c * csp + 4 * j4 + (e & 3)];
            }
    return wr2;
}
// ... FC2 [24][288][8] from We^T `wet` ([48][1152]): request p of thread t = We^T[2p][4t .. +3], We^T[2p + 1][4t .. +3]
static inline std::vector<_Float16> pack_tail_fc2(const _Float16* wet)
{
    const int ce = 1152;
    std::vector<_Float16> we2((size_t)24 * 288 * 8);
    for (int p = 0; p < 24; ++p)
        for (int t = 0; t < 288; ++t)
            for (int e = 0; e < 8; ++e) we2[((size_t)p * 288 + t) * 8 + e] = wet[(size_t)(2 * p + (e < 4 ? 0 : 1)) * ce + 4 * t + (e & 3)];
    return we2;
}

// A project conv with e4m3 weights for pw_gemm_fp8_kernel (MMC_PRECISION_FP8)
struct Fp8Image {
    int N = 0, K = 0, KS128 = 0, NFp = 0;
    std::vector<uint8_t> w8;   // [NFp][KS128][64][32]
    std::vector<float> sw;     // [16 NFp] per-output-channel scales
    std::vector<float> b;      // [16 NFp]
};
// e4m3 weights for pw_gemm_fp8_kernel: per-output-channel scale amax / 448 (the 1 / log2 e of the scaled domain rides in the
// scale), fragment f = channels 16 f .. +15, k-step of 128, lane (i, q) holds k = 128 ks + 32 q .. +31 of channel 16 f + i
static inline Fp8Image pack_fp8(const float* w, const float* b, int N, int K)
{
    Fp8Image L;
    L.N = N; L.K = K; L.KS128 = (K + 127) / 128; L.NFp = ((N + 15) / 16 + 6) / 7 * 7;
    L.w8.assign((size_t)L.NFp * L.KS128 * 64 * 32, (uint8_t)0);
    L.sw.assign((size_t)16 * L.NFp, 0.0f);
    L.b.assign((size_t)16 * L.NFp, 0.0f);
    for (int nn = 0; nn < L.N; ++nn) {
        float amax = 0.f;
        for (int k = 0; k < L.K; ++k) {
            const float v = std::fabs(w[(size_t)nn * L.K + k]);
            if (amax < v) amax = v;
        }
        const float sc = amax > 0.f ? amax / 448.0f : 1.0f;
        L.sw[nn] = (float)(sc / LOG2E);
        L.b[nn] = b[nn];
        for (int k = 0; k < L.K; ++k) {
            const int f = nn / 16, ii = nn % 16, ks = k / 128, qq = (k % 128) / 32, e = k % 32;
            L.w8[((((size_t)f * L.KS128 + ks) * 64) + qq * 16 + ii) * 32 + e] = e4m3_encode(w[(size_t)nn * L.K + k] / sc);
        }
    }
    return L;
}

// ------------------------------------------------------------------------------------------
// activation layouts a kernel writes that are not NHWC
// ------------------------------------------------------------------------------------------
// mb1_kernel<true>'s depthwise output (Mb1Args::D with `planar`, read back by thin_proj_kernel through x_plane_rows = n * hw): C / 32
// planes of n * hw pixel rows of 32 channels, [C / 32][n * hw][32].  Where NHWC element (patch b, pixel pix, channel c) of a launch
// over n patches stands in the planes:
static inline size_t planes_index(int n, int hw, int b, int pix, int c)
{
    return (((size_t)(c >> 5) * n + b) * hw + pix) * 32 + (c & 31);
}
// ... and the whole tensor back as NHWC [n][hw][C] (per-tensor mode hands `b1.dw` out in that layout whatever the kernels exchanged)
template <typename T>
static inline std::vector<T> planes_to_nhwc(const T* planes, int n, int hw, int C)
{
    std::vector<T> out((size_t)n * hw * C);
    for (int b = 0; b < n; ++b)
        for (int pix = 0; pix < hw; ++pix)
            for (int c = 0; c < C; ++c) out[((size_t)b * hw + pix) * C + c] = planes[planes_index(n, hw, b, pix, c)];
    return out;
}
