// pack_check.cpp -- stand-alone host check of csrc/backbone_pack.h: every weight layout, block 1's activation planes and the blob reader, no GPU and no HIP.
// For each packer: a tensor whose elements are all distinct (exact in fp16), then a walk over the packed IMAGE in the order the
// kernel reads it (kernels.h field comments) that says which tensor element, or zero, must stand at each position.  The packers
// walk the tensor; this walks the image, so gaps, duplicates and non-zero padding all show.
// One line per check; exits non-zero on the first mismatch.
//   clang++ -std=c++17 -O1 tests/host/pack_check.cpp -o pack_check && ./pack_check
#include "../../mermaid_classifier_amd/csrc/backbone_pack.h"

#include <cstdarg>
#include <cstdlib>
#include <string>

static const char* g_check = "";
[[noreturn]] static void bad(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    printf("FAIL %s: ", g_check);
    vprintf(fmt, ap);
    printf("\n");
    va_end(ap);
    exit(1);
}
static void begin(const char* name) { g_check = name; }
static void ok() { printf("ok   %s\n", g_check); }
#define REQUIRE(cond, ...) do { if (!(cond)) bad(__VA_ARGS__); } while (0)

// n distinct values, each exact in fp16: integers of magnitude <= 2048 while they last (n <= 4097), else distinct fp16 bit patterns
// (positive normals 0x0400 .. 0x77FF, then their negatives)
static std::vector<float> distinct(size_t n, int salt = 0)
{
    std::vector<float> v(n);
    if (n <= 4097) {
        for (size_t i = 0; i < n; ++i) v[i] = (float)((int)((i * 2731 + salt) % 4097) - 2048);   // 2731 is coprime to 4097: a permutation
        return v;
    }
    REQUIRE(n <= 2 * 0x7400, "distinct(%zu): too many", n);
    for (size_t i = 0; i < n; ++i) {
        const uint16_t bits = (uint16_t)(0x0400 + i % 0x7400) | (i >= 0x7400 ? 0x8000 : 0);
        _Float16 h;
        memcpy(&h, &bits, 2);
        v[i] = (float)h;
    }
    return v;
}
static bool same(_Float16 a, _Float16 b) { return memcmp(&a, &b, 2) == 0; }
static bool same(float a, float b) { return memcmp(&a, &b, 4) == 0; }
static const _Float16 H0 = (_Float16)0.0f;

// every tensor element must be read from exactly `times` image positions (0: at least once)
struct Cover {
    std::vector<int> seen;
    explicit Cover(size_t n) : seen(n, 0) {}
    void hit(size_t i) { ++seen[i]; }
    void done(int times = 1) const
    {
        for (size_t i = 0; i < seen.size(); ++i)
            REQUIRE(times ? seen[i] == times : seen[i] >= 1, "tensor element %zu stands at %d image positions", i, seen[i]);
    }
};

// ---- pw_gemm image: fragment (chunk, kstep, t), lane (q*16 + m), 8 halves; fragment row (t*16 + 4qr + jr) <- channel
// (chunk*16nt + qr*4nt + 4t + jr) ----
static void check_pw(int N, int K, int nt)
{
    const double wscale = 1.0 / LOG2E, bscale = LOG2E;
    const std::vector<float> w = distinct((size_t)N * K), b = distinct(N, 7);
    const PwImage L = pack_pw(w.data(), b.data(), N, K, nt, wscale, bscale);
    const int Kp = (K + 31) / 32 * 32, nch = (N + 16 * nt - 1) / (16 * nt), Np = nch * 16 * nt;
    REQUIRE(L.N == N && L.K == K && L.Kp == Kp && L.nt == nt && L.n_chunks == nch, "geometry");
    REQUIRE(L.w.size() == (size_t)Np * Kp && L.b.size() == (size_t)Np, "image size %zu / %zu", L.w.size(), L.b.size());
    Cover cov((size_t)N * K);
    size_t pos = 0;
    for (int ch = 0; ch < nch; ++ch)
        for (int ks = 0; ks < Kp / 32; ++ks)
            for (int t = 0; t < nt; ++t)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j, ++pos) {
                        const int q = lane >> 4, m = lane & 15, qr = m >> 2, jr = m & 3;
                        const int c = ch * 16 * nt + qr * 4 * nt + 4 * t + jr, k = ks * 32 + q * 8 + j;
                        _Float16 want = H0;
                        if (c < N && k < K) { want = (_Float16)(float)(w[(size_t)c * K + k] * wscale); cov.hit((size_t)c * K + k); }
                        REQUIRE(same(L.w[pos], want), "chunk %d kstep %d t %d lane %d elem %d", ch, ks, t, lane, j);
                    }
    cov.done();
    for (int c = 0; c < Np; ++c) REQUIRE(same(L.b[c], c < N ? (float)(b[c] * bscale) : 0.f), "bias %d", c);
}

// ---- plain fragment order [nf][ks][64 lanes][8]: lane (q*16 + m) of fragment (f, kstep) holds W[16f + m][32 kstep + 8q .. +8] ----
template <typename T>
static void check_frag(const T* w, int N, int K, int ld, int nf, int ks, double scale)
{
    const std::vector<_Float16> img = pack_frag(w, N, K, ld, nf, ks, scale);
    REQUIRE(img.size() == (size_t)nf * ks * 512, "image size %zu", img.size());
    Cover cov((size_t)N * K);
    size_t pos = 0;
    for (int f = 0; f < nf; ++f)
        for (int s = 0; s < ks; ++s)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j, ++pos) {
                    const int n = 16 * f + (lane & 15), k = 32 * s + 8 * (lane >> 4) + j;
                    _Float16 want = H0;
                    if (n < N && k < K) { want = (_Float16)(float)(w[(size_t)n * ld + k] * scale); cov.hit((size_t)n * K + k); }
                    REQUIRE(same(img[pos], want), "fragment %d kstep %d lane %d elem %d", f, s, lane, j);
                }
    cov.done();
}

// ---- stem: C/16 A fragments of K = 32; row (t*16 + 4q + j) <- channel q*4*(C/16) + 4t + j; kernel row qq's first 8 values at
// [8 qq .. +8], the ninth values at [24 .. 27) ----
static void check_stem(int C)
{
    const std::vector<float> w = distinct((size_t)C * 27);
    const std::vector<_Float16> img = pack_stem(w.data(), C);
    REQUIRE(img.size() == (size_t)C * 32, "image size %zu", img.size());
    Cover cov((size_t)C * 27);
    const int snt = C / 16;
    for (int row = 0; row < C; ++row)
        for (int col = 0; col < 32; ++col) {
            const int t = row / 16, q = (row % 16) / 4, j = row % 4, c = q * 4 * snt + 4 * t + j;
            int src = -1;
            if (col < 24) src = (col / 8) * 9 + col % 8;
            else if (col < 27) src = (col - 24) * 9 + 8;
            _Float16 want = H0;
            if (src >= 0) { want = (_Float16)(float)(w[(size_t)c * 27 + src] * LOG2E); cov.hit((size_t)c * 27 + src); }
            REQUIRE(same(img[(size_t)row * 32 + col], want), "row %d col %d", row, col);
        }
    cov.done();
}

// ---- expand: natural rows [ce][kp] (MbArgs::Wexp), and block 1's K-permuted rows [ce][32] (Mb1Args::wexp: slot 8q+j <- channel 4q+j) ----
static void check_expand_rows(int ce, int cin, int kp)
{
    const std::vector<float> w = distinct((size_t)ce * cin);
    const std::vector<_Float16> img = pack_expand_rows(w.data(), ce, cin, kp);
    REQUIRE(img.size() == (size_t)ce * kp, "image size %zu", img.size());
    for (int c = 0; c < ce; ++c)
        for (int k = 0; k < kp; ++k)
            REQUIRE(same(img[(size_t)c * kp + k], k < cin ? (_Float16)(float)(w[(size_t)c * cin + k] * LOG2E) : H0), "row %d col %d", c, k);
}
static void check_expand_kperm(int ce)
{
    const int cin = 16, kp = 32;
    const std::vector<float> w = distinct((size_t)ce * cin);
    const std::vector<_Float16> wn = pack_expand_rows(w.data(), ce, cin, kp), img = pack_expand_kperm(wn.data(), ce, kp);
    REQUIRE(img.size() == (size_t)ce * 32, "image size %zu", img.size());
    Cover cov((size_t)ce * cin);
    for (int c = 0; c < ce; ++c)
        for (int s = 0; s < 32; ++s) {
            const int q = s / 8, j = s % 8;
            _Float16 want = H0;
            if (j < 4) { want = (_Float16)(float)(w[(size_t)c * cin + 4 * q + j] * LOG2E); cov.hit((size_t)c * cin + 4 * q + j); }
            REQUIRE(same(img[(size_t)c * 32 + s], want), "row %d slot %d", c, s);
        }
    cov.done();
}

// ---- depthwise: tap-major fp32 [k*k][ce] + scaled bias (DwArgs::wt / bias) ----
static void check_dw_taps(int ce, int k, double tsc)
{
    const std::vector<float> w = distinct((size_t)ce * k * k), b = distinct(ce, 3);
    const std::vector<float> img = pack_dw_taps(w.data(), ce, k, tsc), bias = pack_bias(b.data(), ce, ce, LOG2E);
    REQUIRE(img.size() == (size_t)k * k * ce && bias.size() == (size_t)ce, "image size");
    for (int t = 0; t < k * k; ++t)
        for (int c = 0; c < ce; ++c) REQUIRE(same(img[(size_t)t * ce + c], (float)(w[(size_t)c * k * k + t] * tsc)), "tap %d channel %d", t, c);
    for (int c = 0; c < ce; ++c) REQUIRE(same(bias[c], (float)(b[c] * LOG2E)), "bias %d", c);
}

// the fp16 pair of slot s = 3 ky + d of channel c: taps (2d, 2d+1) of kernel row ky, zero beyond the kernel (TailBlock::dwp)
static uint32_t want_pair(const std::vector<float>& w, int c, int k, int s, Cover* cov)
{
    const int ky = s / 3, d = s % 3;
    _Float16 h[2] = {H0, H0};
    for (int e = 0; e < 2; ++e) {
        const int kx = 2 * d + e;
        if (ky < k && kx < k) {
            h[e] = (_Float16)w[(size_t)c * k * k + ky * k + kx];
            if (cov) cov->hit((size_t)c * k * k + ky * k + kx);
        }
    }
    uint32_t u;
    memcpy(&u, h, 4);
    return u;
}
// ---- pair taps [15][ce] (MbtArgs::dwp), and the same + bias in 16-byte requests [4][ce][4] (Mid14Args::dwp, TailBlock::dwp): request j
// of channel c = slots 4j .. 4j+3, slot 15 = the bias bits ----
static void check_dw_pairs(int ce, int k)
{
    const std::vector<float> w = distinct((size_t)ce * k * k), b = distinct(ce, 5);
    const std::vector<uint32_t> dp = pack_dw_pairs(w.data(), ce, k);
    REQUIRE(dp.size() == (size_t)15 * ce, "pairs size %zu", dp.size());
    Cover cov((size_t)ce * k * k);
    for (int s = 0; s < 15; ++s)
        for (int c = 0; c < ce; ++c) REQUIRE(dp[(size_t)s * ce + c] == want_pair(w, c, k, s, &cov), "pairs: slot %d channel %d", s, c);
    cov.done();
    const std::vector<float> db = pack_bias(b.data(), ce, ce, LOG2E);
    const std::vector<uint32_t> rq = pack_dw_requests(dp.data(), db.data(), ce);
    REQUIRE(rq.size() == (size_t)16 * ce, "requests size %zu", rq.size());
    for (int j = 0; j < 4; ++j)
        for (int c = 0; c < ce; ++c)
            for (int e = 0; e < 4; ++e) {
                const int s = 4 * j + e;
                uint32_t want;
                if (s < 15) want = want_pair(w, c, k, s, nullptr);
                else { const float bias = (float)(b[c] * LOG2E); memcpy(&want, &bias, 4); }
                REQUIRE(rq[((size_t)j * ce + c) * 4 + e] == want, "requests: request %d channel %d elem %d", j, c, e);
            }
}

// ---- Toeplitz fragments [ce/16][k][2][64][4] (Mid14Args::dwdiag): lane 4 blk + i holds A[i][0..3] of block blk,
// A[i][kk] = w[c][ky][kk - i + 4h - 2 + R], block blk = channel 2 (blk & 3) + ((blk >> 2) & 1) + 8 (blk >> 3) of the group ----
static void check_toeplitz(int ce, int k)
{
    const double tsc = 1.0;
    const std::vector<float> w = distinct((size_t)ce * k * k);
    const std::vector<_Float16> img = pack_dw_toeplitz(w.data(), ce, k, tsc);
    REQUIRE(img.size() == (size_t)(ce / 16) * k * 2 * 64 * 4, "image size %zu", img.size());
    int chan_seen[16] = {0};
    for (int blk = 0; blk < 16; ++blk) ++chan_seen[2 * (blk & 3) + ((blk >> 2) & 1) + 8 * (blk >> 3)];
    for (int c = 0; c < 16; ++c) REQUIRE(chan_seen[c] == 1, "block -> channel map misses channel %d", c);
    Cover cov((size_t)ce * k * k);
    const int R = k / 2;
    size_t pos = 0;
    for (int g = 0; g < ce / 16; ++g)
        for (int ky = 0; ky < k; ++ky)
            for (int h = 0; h < 2; ++h)
                for (int lane = 0; lane < 64; ++lane)
                    for (int kk = 0; kk < 4; ++kk, ++pos) {
                        const int blk = lane >> 2, i = lane & 3;
                        const int c = 16 * g + 2 * (blk & 3) + ((blk >> 2) & 1) + 8 * (blk >> 3), t = kk - i + 4 * h - 2 + R;
                        _Float16 want = H0;
                        if (t >= 0 && t < k) {
                            want = (_Float16)(float)(w[((size_t)c * k + ky) * k + t] * tsc);
                            cov.hit(((size_t)c * k + ky) * k + t);
                        }
                        REQUIRE(same(img[pos], want), "group %d ky %d quad %d lane %d k %d", g, ky, h, lane, kk);
                    }
    cov.done(0);   // a Toeplitz matrix repeats its taps
}

// ---- squeeze-excite, fp32 fragment order [ce/16][3][64][4] + 4 floats (launch_se_gate's WrP / WeP) ----
static void check_se_frag(int ce, int cs)
{
    const double psc = 1.0 / (196.0 * LOG2E);
    const std::vector<float> wr = distinct((size_t)cs * ce), we = distinct((size_t)ce * cs, 11);
    const std::vector<float> f1 = pack_se_fc1_frag(wr.data(), ce, cs, psc), f2 = pack_se_fc2_frag(we.data(), ce, cs);
    const size_t n = (size_t)(ce / 16) * 3 * 64 * 4;
    REQUIRE(f1.size() == n + 4 && f2.size() == n + 4, "image size %zu / %zu", f1.size(), f2.size());
    Cover c1((size_t)cs * ce), c2((size_t)ce * cs);
    size_t pos = 0;
    for (int g = 0; g < ce / 16; ++g)
        for (int t = 0; t < 3; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e, ++pos) {
                    const int i = lane & 15, q = lane >> 4;
                    const int j = 16 * t + i, c = 16 * g + 4 * q + e;   // FC1: Wr[j][c]
                    float want = 0.f;
                    if (j < cs) { want = (float)(wr[(size_t)j * ce + c] * psc); c1.hit((size_t)j * ce + c); }
                    REQUIRE(same(f1[pos], want), "FC1: group %d frag %d lane %d elem %d", g, t, lane, e);
                    const int nn = 16 * g + i, k = 16 * t + 4 * q + e;  // FC2: We[n][k]
                    want = 0.f;
                    if (k < cs) { want = we[(size_t)nn * cs + k]; c2.hit((size_t)nn * cs + k); }
                    REQUIRE(same(f2[pos], want), "FC2: group %d frag %d lane %d elem %d", g, t, lane, e);
                }
    for (size_t e = n; e < n + 4; ++e) REQUIRE(same(f1[e], 0.f) && same(f2[e], 0.f), "tail float %zu", e - n);
    c1.done();
    c2.done();
}

// ---- natural / transposed fp32 (se_small, se_wide), fp16 transposed Wr^T [ce][csp] / We^T [csp][ce] + padded bias, and proj_patch's
// FC1 groups [csp/4][rows][4] (ProjPatchArgs::wr_g) ----
static void check_se_t(int ce, int cs, int csp, int rows)
{
    const double psc = 1.0 / (49.0 * LOG2E);
    const std::vector<float> wr = distinct((size_t)cs * ce), we = distinct((size_t)ce * cs, 13), br = distinct(cs, 17);
    const std::vector<float> n1 = pack_se_fc1_nat(wr.data(), ce, cs, psc), t2 = pack_se_fc2_t(we.data(), ce, cs);
    REQUIRE(n1.size() == (size_t)cs * ce && t2.size() == (size_t)cs * ce, "fp32 sizes");
    for (int j = 0; j < cs; ++j)
        for (int c = 0; c < ce; ++c) {
            REQUIRE(same(n1[(size_t)j * ce + c], (float)(wr[(size_t)j * ce + c] * psc)), "fp32 FC1 [%d][%d]", j, c);
            REQUIRE(same(t2[(size_t)j * ce + c], we[(size_t)c * cs + j]), "fp32 FC2^T [%d][%d]", j, c);
        }
    const std::vector<_Float16> wrt = pack_se_fc1_t16(wr.data(), ce, cs, csp), wet = pack_se_fc2_t16(we.data(), ce, cs, csp);
    REQUIRE(wrt.size() == (size_t)ce * csp && wet.size() == (size_t)csp * ce, "fp16 sizes");
    for (int c = 0; c < ce; ++c)
        for (int j = 0; j < csp; ++j) {
            REQUIRE(same(wrt[(size_t)c * csp + j], j < cs ? (_Float16)wr[(size_t)j * ce + c] : H0), "Wr^T [%d][%d]", c, j);
            REQUIRE(same(wet[(size_t)j * ce + c], j < cs ? (_Float16)we[(size_t)c * cs + j] : H0), "We^T [%d][%d]", j, c);
        }
    const int padded = csp > 32 ? csp : 32;
    const std::vector<float> brp = pack_bias(br.data(), cs, padded, 1.0);
    REQUIRE(brp.size() == (size_t)padded, "bias size");
    for (int j = 0; j < padded; ++j) REQUIRE(same(brp[j], j < cs ? br[j] : 0.f), "bias %d", j);
    const std::vector<_Float16> g = pack_se_fc1_groups(wrt.data(), ce, csp, rows);
    REQUIRE(g.size() == (size_t)(csp / 4) * rows * 4, "groups size %zu", g.size());
    Cover cov((size_t)cs * ce);
    size_t pos = 0;
    for (int gr = 0; gr < csp / 4; ++gr)
        for (int row = 0; row < rows; ++row)
            for (int e = 0; e < 4; ++e, ++pos) {
                const int j = 4 * gr + e;
                _Float16 want = H0;
                if (row < ce && j < cs) { want = (_Float16)wr[(size_t)j * ce + row]; cov.hit((size_t)j * ce + row); }
                REQUIRE(same(g[pos], want), "groups: group %d row %d elem %d", gr, row, e);
            }
    cov.done();
}

// ---- tail7's requests (TailBlock::wr_t / we_t), 1152 channels x 48: FC1 request p of thread (cr, j4) = Wr^T[64p + cr][4 j4 .. +3],
// Wr^T[64p + 32 + cr][4 j4 .. +3]; FC2 request p of thread t = We^T[2p][4t .. +3], We^T[2p + 1][4t .. +3] ----
static void check_tail7()
{
    const int ce = 1152, cs = 48;
    const std::vector<float> wr = distinct((size_t)cs * ce), we = distinct((size_t)ce * cs);
    const std::vector<_Float16> wrt = pack_se_fc1_t16(wr.data(), ce, cs, cs), wet = pack_se_fc2_t16(we.data(), ce, cs, cs);
    const std::vector<_Float16> r1 = pack_tail_fc1(wrt.data()), r2 = pack_tail_fc2(wet.data());
    REQUIRE(r1.size() == (size_t)18 * 384 * 8 && r2.size() == (size_t)24 * 288 * 8, "sizes %zu / %zu", r1.size(), r2.size());
    Cover c1((size_t)cs * ce), c2((size_t)ce * cs);
    size_t pos = 0;
    for (int p = 0; p < 18; ++p)
        for (int t = 0; t < 384; ++t)
            for (int e = 0; e < 8; ++e, ++pos) {
                const int cr = t / 12, j4 = t % 12, c = 64 * p + (e < 4 ? 0 : 32) + cr, j = 4 * j4 + (e & 3);
                c1.hit((size_t)j * ce + c);
                REQUIRE(same(r1[pos], (_Float16)wr[(size_t)j * ce + c]), "FC1: request %d thread %d elem %d", p, t, e);
            }
    pos = 0;
    for (int p = 0; p < 24; ++p)
        for (int t = 0; t < 288; ++t)
            for (int e = 0; e < 8; ++e, ++pos) {
                const int j = 2 * p + (e < 4 ? 0 : 1), c = 4 * t + (e & 3);
                c2.hit((size_t)c * cs + j);
                REQUIRE(same(r2[pos], (_Float16)we[(size_t)c * cs + j]), "FC2: request %d thread %d elem %d", p, t, e);
            }
    c1.done();
    c2.done();
}

// ---- e4m3 image [NFp][KS128][64][32] (Fp8GemmArgs::W8): lane (i, q) = q*16 + i of fragment f holds k = 128 ks + 32 q .. +31 of
// channel 16 f + i; sw = amax / 448 / log2 e per channel (0 for padding), bias padded ----
static void check_fp8(int N, int K)
{
    const std::vector<float> w = distinct((size_t)N * K), b = distinct(N, 19);
    const Fp8Image L = pack_fp8(w.data(), b.data(), N, K);
    const int KS = (K + 127) / 128, NFp = ((N + 15) / 16 + 6) / 7 * 7;
    REQUIRE(L.N == N && L.K == K && L.KS128 == KS && L.NFp == NFp, "geometry: KS128 %d NFp %d", L.KS128, L.NFp);
    REQUIRE(L.w8.size() == (size_t)NFp * KS * 64 * 32 && L.sw.size() == (size_t)16 * NFp && L.b.size() == (size_t)16 * NFp, "sizes");
    std::vector<float> sc(N);
    for (int n = 0; n < N; ++n) {
        float amax = 0.f;
        for (int k = 0; k < K; ++k) amax = std::fmax(amax, std::fabs(w[(size_t)n * K + k]));
        sc[n] = amax > 0.f ? amax / 448.0f : 1.0f;
    }
    Cover cov((size_t)N * K);
    size_t pos = 0;
    for (int f = 0; f < NFp; ++f)
        for (int ks = 0; ks < KS; ++ks)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 32; ++e, ++pos) {
                    const int i = lane & 15, q = lane >> 4, n = 16 * f + i, k = 128 * ks + 32 * q + e;
                    uint8_t want = 0;
                    if (n < N && k < K) { want = e4m3_encode(w[(size_t)n * K + k] / sc[n]); cov.hit((size_t)n * K + k); }
                    REQUIRE(L.w8[pos] == want, "fragment %d kstep %d lane %d elem %d: 0x%02x, expected 0x%02x", f, ks, lane, e, L.w8[pos], want);
                }
    cov.done();
    for (int n = 0; n < 16 * NFp; ++n) {
        REQUIRE(same(L.sw[n], n < N ? (float)(sc[n] / LOG2E) : 0.f), "scale %d", n);
        REQUIRE(same(L.b[n], n < N ? b[n] : 0.f), "bias %d", n);
    }
}

// ---- block 1's planes [C/32][n * hw][32] (Mb1Args::D with planar): the image is filled in mb1_kernel<true>'s own address arithmetic,
// plane chunk at (chunk n hw + b hw + pix) 32 + c, with the NHWC position of every element as its value; planes_to_nhwc must then
// return 0, 1, 2, ... and planes_index must name every image position exactly once ----
static void check_planes(int n, int hw, int C)
{
    const size_t total = (size_t)n * hw * C;
    std::vector<uint32_t> img(total, 0xFFFFFFFFu);
    for (int chunk = 0; chunk < C / 32; ++chunk)
        for (int b = 0; b < n; ++b)
            for (int pix = 0; pix < hw; ++pix)
                for (int c = 0; c < 32; ++c)
                    img[((size_t)chunk * n * hw + (size_t)b * hw + pix) * 32 + c] = (uint32_t)(((size_t)b * hw + pix) * C + 32 * chunk + c);
    const std::vector<uint32_t> nhwc = planes_to_nhwc(img.data(), n, hw, C);
    REQUIRE(nhwc.size() == total, "size %zu", nhwc.size());
    for (size_t i = 0; i < total; ++i) REQUIRE(nhwc[i] == (uint32_t)i, "NHWC element %zu came from the image position of element %u", i, nhwc[i]);
    Cover cov(total);
    for (int b = 0; b < n; ++b)
        for (int pix = 0; pix < hw; ++pix)
            for (int c = 0; c < C; ++c) {
                const size_t at = planes_index(n, hw, b, pix, c);
                REQUIRE(at < total, "patch %d pixel %d channel %d: position %zu of %zu", b, pix, c, at, total);
                cov.hit(at);
                // thin_proj_kernel's read of k = c, row = pix with plane_rows = n hw (k_early.hip, plane_rows != 0)
                REQUIRE(at == ((size_t)(c >> 5) * ((size_t)n * hw) + (size_t)b * hw + pix) * 32 + (c & 31), "patch %d pixel %d channel %d", b, pix, c);
            }
    cov.done();
}

// ---- blobs ----
struct Blob {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off, nb;   // what the table says, in order
    std::vector<std::string> name;
};
// a well-formed blob of zeros for architecture `arch`: only the table matters
static Blob make_blob(int arch)
{
    const ArchDef A = make_arch(arch);
    Blob B;
    auto add = [&](size_t floats, const std::string& nm) { B.nb.push_back(floats * 4); B.name.push_back(nm); };
    add((size_t)A.stem * 27, "stem.weight"); add(A.stem, "stem.bias"); add(3, "stem.padval");
    for (size_t i = 0; i < A.blocks.size(); ++i) {
        const BlockDef& d = A.blocks[i];
        const size_t ce = (size_t)d.cin * d.e, cs = d.cin / 4 > 1 ? d.cin / 4 : 1;
        const std::string b = "b" + std::to_string(i);
        if (d.e != 1) { add(ce * d.cin, b + ".expand"); add(ce, b + ".expand"); }
        add(ce * d.k * d.k, b + ".dw"); add(ce, b + ".dw");
        add(cs * ce, b + ".se"); add(cs, b + ".se"); add(ce * cs, b + ".se"); add(ce, b + ".se");
        add((size_t)d.cout * ce, b + ".project"); add(d.cout, b + ".project");
    }
    add((size_t)A.feat * A.head_in, "head.weight"); add(A.feat, "head.bias");
    uint64_t at = 16 + 16 * B.nb.size();
    for (uint64_t n : B.nb) { B.off.push_back(at); at += n; }
    B.bytes.assign(at, 0);
    return B;
}
// (re)writes header and table from B's fields; n_tensors and the byte count may be overridden
static void seal(Blob& B, int arch, uint32_t n_tensors)
{
    uint32_t hdr[4] = {0, 1, (uint32_t)arch, n_tensors};
    memcpy(hdr, "MMCW", 4);
    memcpy(B.bytes.data(), hdr, 16);
    for (size_t i = 0; i < B.nb.size() && 16 + 16 * (i + 1) <= B.bytes.size(); ++i) {
        memcpy(B.bytes.data() + 16 + 16 * i, &B.off[i], 8);
        memcpy(B.bytes.data() + 24 + 16 * i, &B.nb[i], 8);
    }
}
static int read(const Blob& B, size_t nbytes, int arch, RawNet* net, BlobError* err)
{
    BlobReader rd;
    if (rd.open(B.bytes.data(), nbytes, arch, err)) return err->code;
    return read_blob(rd, make_arch(arch), net, err);
}
static void expect_refused(const Blob& B, size_t nbytes, int arch, const char* prefix)
{
    RawNet net;
    BlobError err;
    const int r = read(B, nbytes, arch, &net, &err);
    REQUIRE(r == MMC_ERR_WEIGHTS && err.code == r, "accepted (code %d), expected \"%s...\"", r, prefix);
    REQUIRE(strncmp(err.msg, prefix, strlen(prefix)) == 0, "message \"%s\", expected \"%s...\"", err.msg, prefix);
}
static void check_blob_good(int arch)
{
    Blob B = make_blob(arch);
    seal(B, arch, (uint32_t)B.nb.size());
    RawNet net;
    BlobError err;
    REQUIRE(read(B, B.bytes.size(), arch, &net, &err) == MMC_OK, "refused: %s", err.msg);
    const ArchDef A = make_arch(arch);
    REQUIRE(net.blk.size() == A.blocks.size(), "%zu blocks", net.blk.size());
    // the views in table order: each must start where its table entry says
    std::vector<const float*> v = {net.stem_w, net.stem_b, net.stem_pad};
    for (size_t i = 0; i < net.blk.size(); ++i) {
        const RawBlock& R = net.blk[i];
        REQUIRE((A.blocks[i].e != 1) == (R.exp_w != nullptr) && (R.exp_w != nullptr) == (R.exp_b != nullptr), "block %zu expand views", i);
        if (R.exp_w) { v.push_back(R.exp_w); v.push_back(R.exp_b); }
        for (const float* p : {R.dw_w, R.dw_b, R.se_wr, R.se_br, R.se_we, R.se_be, R.proj_w, R.proj_b}) v.push_back(p);
    }
    v.push_back(net.head_w); v.push_back(net.head_b);
    REQUIRE(v.size() == B.nb.size(), "%zu views for %zu tensors", v.size(), B.nb.size());
    for (size_t i = 0; i < v.size(); ++i)
        REQUIRE((const uint8_t*)v[i] == B.bytes.data() + B.off[i], "view %zu (%s) is not at its table offset", i, B.name[i].c_str());
}
static size_t find_tensor(const Blob& B, const char* name, int nth)
{
    for (size_t i = 0; i < B.name.size(); ++i)
        if (B.name[i] == name && nth-- == 0) return i;
    bad("no tensor %s", name);
}

int main()
{
    begin("pw_gemm image N 40 K 24 nt 2"); check_pw(40, 24, 2); ok();
    begin("pw_gemm image N 72 K 40 nt 4"); check_pw(72, 40, 4); ok();
    {
        const int N = 24, K = 40, ld = 48, nf = 2, ks = 3;
        std::vector<float> w = distinct((size_t)N * ld);
        begin("fragment order N 24 K 40 ld 48 nf 2 ks 3 from float"); check_frag(w.data(), N, K, ld, nf, ks, 1.0 / LOG2E); ok();
        std::vector<_Float16> h(w.size());
        for (size_t i = 0; i < w.size(); ++i) h[i] = (_Float16)w[i];
        begin("fragment order N 24 K 40 ld 48 nf 2 ks 3 from _Float16"); check_frag(h.data(), N, K, ld, nf, ks, 1.0); ok();
    }
    begin("stem 32 channels"); check_stem(32); ok();
    begin("stem 48 channels"); check_stem(48); ok();
    begin("expand rows ce 48 cin 24 kp 32"); check_expand_rows(48, 24, 32); ok();
    begin("expand rows ce 32 cin 40 kp 64"); check_expand_rows(32, 40, 64); ok();
    begin("expand K-permuted ce 96"); check_expand_kperm(96); ok();
    begin("tap-major taps k 3 ce 16"); check_dw_taps(16, 3, 1.0); ok();
    begin("tap-major taps k 5 ce 24, plain-domain input"); check_dw_taps(24, 5, LOG2E); ok();
    begin("pair taps + 16-byte requests k 3 ce 16"); check_dw_pairs(16, 3); ok();
    begin("pair taps + 16-byte requests k 5 ce 16"); check_dw_pairs(16, 5); ok();
    begin("Toeplitz k 3 ce 32"); check_toeplitz(32, 3); ok();
    begin("Toeplitz k 5 ce 32"); check_toeplitz(32, 5); ok();
    begin("squeeze-excite fp32 fragment order ce 32 cs 8"); check_se_frag(32, 8); ok();
    begin("squeeze-excite transposed + FC1 groups ce 96 cs 4 csp 4"); check_se_t(96, 4, 4, 128); ok();
    begin("squeeze-excite transposed + FC1 groups ce 40 cs 10 csp 12"); check_se_t(40, 10, 12, 64); ok();
    begin("tail7 requests 1152 / 48"); check_tail7(); ok();
    begin("e4m3 image N 20 K 130"); check_fp8(20, 130); ok();
    begin("block 1 planes -> NHWC, 1 patch 56x56x96"); check_planes(1, 3136, 96); ok();
    begin("block 1 planes -> NHWC, 3 patches 56x56x96"); check_planes(3, 3136, 96); ok();

    begin("blob: well-formed B0"); check_blob_good(MMC_ARCH_B0); ok();
    begin("blob: well-formed B4"); check_blob_good(MMC_ARCH_B4); ok();
    const int arch = MMC_ARCH_B0;
    const Blob good = make_blob(arch);
    const uint32_t nt = (uint32_t)good.nb.size();
    {
        begin("blob: offset 2^64 - 8 with 16 bytes is refused");
        Blob B = good;
        const size_t i = find_tensor(B, "b1.se", 1);   // block 1's squeeze bias: 4 floats, so only the offset is wrong
        REQUIRE(B.nb[i] == 16, "b1.se bias has %llu bytes", (unsigned long long)B.nb[i]);
        B.off[i] = ~(uint64_t)0 - 7;
        seal(B, arch, nt);
        expect_refused(B, B.bytes.size(), arch, "tensor ");
        ok();
    }
    {
        begin("blob: offset + size one past the end is refused");
        Blob B = good;
        B.off[nt - 1] += 1;
        seal(B, arch, nt);
        expect_refused(B, B.bytes.size(), arch, "tensor ");
        ok();
    }
    {
        begin("blob: wrong tensor size is refused");
        Blob B = good;
        B.nb[5] -= 4;
        seal(B, arch, nt);
        expect_refused(B, B.bytes.size(), arch, "tensor 5 (b0.se): expected ");
        ok();
    }
    {
        begin("blob: one tensor too few is refused");
        Blob B = good;
        seal(B, arch, nt - 1);
        expect_refused(B, B.bytes.size(), arch, "weights blob ended before head.bias");
        ok();
    }
    {
        begin("blob: one tensor too many is refused");
        Blob B = good;
        B.off.push_back(B.off[0]); B.nb.push_back(4); B.name.push_back("extra");
        for (uint64_t& o : B.off) o += 16;   // the table grows by one entry
        B.bytes.resize(B.bytes.size() + 16);
        seal(B, arch, nt + 1);
        expect_refused(B, B.bytes.size(), arch, "weights blob has ");
        ok();
    }
    {
        begin("blob: bad magic, version, arch are refused");
        Blob B = good;
        seal(B, arch, nt);
        expect_refused(B, 8, arch, "weights blob is empty");
        B.bytes[0] = 'X';
        expect_refused(B, B.bytes.size(), arch, "bad magic in weights blob");
        seal(B, arch, nt);
        B.bytes[4] = 2;
        expect_refused(B, B.bytes.size(), arch, "weights blob version 2, expected 1");
        seal(B, arch, nt);
        expect_refused(B, B.bytes.size(), MMC_ARCH_B4, "weights blob arch 0 != requested 1");
        ok();
    }
    {
        begin("blob: truncated table is refused");
        Blob B = good;
        seal(B, arch, nt);
        expect_refused(B, 16 + 16 * (size_t)nt - 1, arch, "weights blob truncated (table)");
        ok();
    }
    printf("all checks passed\n");
    return 0;
}
