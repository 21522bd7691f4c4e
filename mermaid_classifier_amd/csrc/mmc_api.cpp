// mmc_api.cpp -- the backbone half of the C ABI (include/mmc.h): the error buffer, the EfficientNet-B0 launch schedule and the crop.
// The calibrated head (predict, top-k, evaluate, classify) is the unit next to this one; the two share api_internal.h.
// Host C++ only; kernels live in k_*.hip.  No torch, no CUDA shims.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "../../include/mmc.h"
#include "api_internal.h"
#include "kernels.h"

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

// every translation unit reports through this (api_internal.h, kernels.h, trainer_internal.h)
int mmc_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char* mmc_last_error(void) { return g_err; }
extern "C" int mmc_version(void) { return 1; }
extern "C" int mmc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------------------------------
// EfficientNet-B0 stage table (the published architecture; mirrors oracle/efficientnet_b0_ref.py)
// ------------------------------------------------------------------------------------------
struct BlockDef { int k, s, e, cin, cout; };
static const BlockDef B0_BLOCKS[16] = {
    {3, 1, 1, 32, 16},  {3, 2, 6, 16, 24},  {3, 1, 6, 24, 24},   {5, 2, 6, 24, 40},
    {5, 1, 6, 40, 40},  {3, 2, 6, 40, 80},  {3, 1, 6, 80, 80},   {3, 1, 6, 80, 80},
    {5, 1, 6, 80, 112}, {5, 1, 6, 112, 112}, {5, 1, 6, 112, 112}, {5, 2, 6, 112, 192},
    {5, 1, 6, 192, 192}, {5, 1, 6, 192, 192}, {5, 1, 6, 192, 192}, {3, 1, 6, 192, 320}};
static const int IMG = 224;
// The published family: B0's stage table under compound scaling (widths to multiples of 8, never below 90 % of the scaled
// value; repeats rounded up).  B0 is the network the reference path runs; B4 (width 1.4, depth 1.8, BASELINE.json
// configs[4]) does not exist in the reference and runs on the generic per-layer kernels.
struct ArchDef { int stem = 32, head_in = 320, feat = 1280; std::vector<BlockDef> blocks; };
static int round_filters(int c, double width)
{
    const double v = c * width;
    int n = (int)(v + 4) / 8 * 8;
    if (n < 8) n = 8;
    if (n < 0.9 * v) n += 8;
    return n;
}
static ArchDef make_arch(int arch)
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

static void same_pad(int size, int k, int s, int* before, int* out)
{
    *out = (size + s - 1) / s;
    int pad = (*out - 1) * s + k - size;
    if (pad < 0) pad = 0;
    *before = pad / 2;
}

// A 1x1 convolution packed for pw_gemm_kernel
struct PwLayer {
    int N = 0, K = 0, Kp = 0, nt = 0, n_chunks = 0;
    _Float16* w = nullptr;  // device [n_chunks*16*nt][Kp]
    float* b = nullptr;     // device [n_chunks*16*nt]
    const char* label[2] = {nullptr, nullptr};   // plan: its pw_gemm instantiation with one / two row fragments per wave (gemm_mt)
};

// A project conv with e4m3 weights for pw_gemm_fp8_kernel (MMC_PRECISION_FP8)
struct Fp8Layer {
    int N = 0, K = 0, KS128 = 0, NFp = 0;
    uint8_t* w8 = nullptr;  // device [NFp][KS128][64][32]
    float* sw = nullptr;    // device [16 NFp] per-output-channel scales
    float* b = nullptr;     // device [16 NFp]
};

// fp32 -> OCP e4m3fn (4 exponent bits, bias 7, 3 mantissa bits, no infinities, largest finite 448), round to nearest even,
// saturating.  The device side uses v_cvt_pk_fp8_f32; the host needs the same encoding for the weights.
static uint8_t e4m3_encode(float x)
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

extern "C" int mmc_fp8_e4m3_encode(const float* in, uint8_t* out, size_t n)
{
    if (!in || !out) return fail(MMC_ERR_ARG, "NULL argument");
    for (size_t i = 0; i < n; ++i) out[i] = e4m3_encode(in[i]);
    return MMC_OK;
}

// Channel fragments (16 wide) per workgroup.  Big-M layers (early blocks) take the widest chunk that
// divides N (X is read once per chunk).  Small-M layers (14x14 and 7x7 blocks, head) take narrow
// chunks: more workgroups and registers left for a 4-step-deep fragment prefetch; X re-reads hit L2.
static int pick_nt(int N, bool small_m)
{
    const int tiles = (N + 15) / 16;
    if (small_m) {
        int best = 4, waste = 1 << 30;
        for (int nt = 4; nt >= 2; --nt) {
            const int w = (tiles + nt - 1) / nt * nt - tiles;
            if (w < waste) { waste = w; best = nt; }
        }
        return tiles <= 4 ? tiles : best;
    }
    for (int nt = 8; nt >= 1; --nt)
        if (tiles % nt == 0) return nt;
    return 1;
}

// ------------------------------------------------------------------------------------------
// schedule switches: read once per handle, by mmc_backbone_create_ex; nothing else on the backbone
// path reads the environment
// ------------------------------------------------------------------------------------------
struct Options {
    bool keep, graph, tail_clk, profile_serial;
    bool fuse, fuse_b0, mb1, mbt, mbt2, mbt4, mb_dot2, mid14, mid14m, projse, se_small, thin_proj, b1_planar;
    bool tail, tail_full, tail_b11;
    bool chain;
    int lanes, fp8_maxh;
};
static bool env_starts(const char* name, char c)
{
    const char* e = getenv(name);
    return e && e[0] == c;
}
static Options read_options()
{
    auto on = [](const char* name) { return !env_starts(name, '0'); };   // default-on switches: a leading 0 turns them off
    Options o;
    o.keep = env_starts("MMC_KEEP_ACTIVATIONS", '1');
    o.graph = on("MMC_GRAPH") && !o.keep;
    o.tail_clk = env_starts("MMC_TAIL_CLK", '1') && !o.keep;
    o.profile_serial = env_starts("MMC_PROFILE_SERIAL", '1');
    o.fuse = on("MMC_FUSE");
    o.fuse_b0 = on("MMC_FUSE_B0");
    o.mb1 = on("MMC_MB1");
    o.mbt = on("MMC_MBT");
    o.mbt2 = on("MMC_MBT2");
    o.mbt4 = on("MMC_MBT4");
    o.mb_dot2 = on("MMC_MB_DOT2");
    o.projse = on("MMC_PROJSE");
    o.se_small = on("MMC_SE_SMALL");
    o.thin_proj = on("MMC_THIN_PROJ");
    o.b1_planar = on("MMC_B1_PLANAR");
    o.tail = on("MMC_TAIL");
    o.tail_full = on("MMC_TAIL_FULL");
    o.tail_b11 = on("MMC_TAIL_B11");
    o.chain = on("MMC_CHAIN");
    const char* e = getenv("MMC_MID14");
    o.mid14 = !e || atoi(e) != 0;
    e = getenv("MMC_MID14M");
    o.mid14m = !e || atoi(e) >= 1;
    e = getenv("MMC_LANES");
    o.lanes = e ? atoi(e) : 2;
    e = getenv("MMC_FP8_MAXH");
    o.fp8_maxh = e && atoi(e) > 7 ? atoi(e) : 7;
    return o;
}

// ------------------------------------------------------------------------------------------
// the plan: which kernels run each block, decided at create time before any weight is packed
// ------------------------------------------------------------------------------------------
// front half (expand + depthwise) of a block
enum class Front {
    StemDw,    // block 0 with the stem (stem_dw_kernel)
    Mbt,       // mbt_kernel / mbt2_kernel / mbt4_kernel
    Mid14,     // mid14_kernel / mid14m_kernel
    Mb1,       // block 1 with block 0's project folded in (mb1_kernel)
    MbPre,     // ... on mbconv_a_kernel PRE
    MbD,       // mbconv_d_kernel
    MbA,       // mbconv_a_kernel
    Unfused,   // expand GEMM + dwconv
    Tail,      // inside the pass's tail7 launch
};
// back half (squeeze-excite + project) of a block
enum class Back {
    ProjPatch,   // proj_patch_kernel
    SeProject,   // squeeze-excite, then the project conv
    SeFolded,    // block 0: squeeze-excite only, its project runs inside block 1's kernel
    Tail,        // inside the pass's tail7 launch
};
enum class Se { Wide, Small, Fused };
enum class Proj { Thin, Fp8, Gemm };
// how the pass ends
enum class TailRoute {
    None,     // head GEMM
    B12,      // b12-15.tail + head GEMM
    B11,      // b11-head.tail (block 11's back half, blocks 12..15, head); per-tensor mode: b11.tail, b<j>.tail, head.tail
    B11All,   // b11all-head.tail (all of block 11 too)
};

struct BlockW {
    BlockDef d;
    // ---- geometry ----
    int H = 0, Ho = 0, ce = 0, cs = 0, cs4 = 0, pad = 0;
    bool has_expand = false, skip = false;
    int tw = 0, CG = 0, S = 0, iters = 0, parts = 0, nz = 1;   // dwconv
    bool fusable = false;   // mbconv_a's tile / chunk geometry (in `mb`) fits
    bool d_fits = false;    // ... and so does mbconv_d's (d_npair .. d_lds)
    int d_npair = 0, d_wl_off = 0, d_red_off = 0, d_lds = 0;
    MbArgs mb{};            // mbconv_a / mbconv_d / mbconv_a PRE: everything but the buffers and the batch
    // ---- plan ----
    Front front = Front::Unfused;
    Back back = Back::SeProject;
    Se se = Se::Fused;
    Proj proj = Proj::Gemm;
    bool mbt4 = false, mid14m = false;   // depthwise on 4x4x4 MFMA blocks (mbt4_kernel / mid14m_kernel)
    bool planar = false;                 // block 1: depthwise output as 32-channel planes between mb1_kernel and thin_proj_kernel
    int nparts = 0;                      // pool partials per patch left by the front half
    const char *front_label = nullptr, *back_label = nullptr;   // the templated instantiation the front half / proj_patch runs on
    // ---- packed weights ----
    PwLayer expand, project;
    Fp8Layer p8;             // the project conv on fp8 operands (Proj::Fp8)
    float *dw_w = nullptr, *dw_b = nullptr;                    // [k*k][ce], [ce]
    float *se_br = nullptr, *se_be = nullptr;
    float *se_wrp = nullptr, *se_wep = nullptr;   // fragment-ordered fp32 squeeze-excite weights (se_fused_kernel)
    float *se_wr_nat = nullptr, *se_we_nat = nullptr, *se_br_nat = nullptr;   // natural fp32 copies (se_small_kernel, se_wide_kernel)
    _Float16* exp_nat = nullptr;   // [ce][32*ksteps] natural rows (mbconv_a / mbconv_d)
    _Float16* exp_frag = nullptr;  // expand weights in MFMA fragment order
    uint32_t* t_dwp = nullptr;     // depthwise taps as fp16 pairs [15][ce] (mbt)
    uint32_t* t_dwp4 = nullptr;    // taps + bias, [4][ce][4] dwords (16-byte requests: mid14, tail7)
    _Float16* dw_diag = nullptr;   // Toeplitz depthwise fragments [ce/16][k][2][64][4] for v_mfma_f32_4x4x4_16B_f16 (mbt4, mid14m)
    _Float16* t_wproj = nullptr;   // tail7 blocks: project weights in plain fragment order
    _Float16 *t_wr = nullptr, *t_we = nullptr;   // squeeze-excite FCs transposed (fp16) for matrix-vector use
    _Float16* t_wrg = nullptr;                   // ... the squeeze FC as proj_patch_kernel reads it (ProjPatchArgs::wr_g)
    _Float16 *t_wr2 = nullptr, *t_we2 = nullptr; // ... blocks 12-15: paired rows for tail7_kernel's 16-byte requests
    _Float16* pp_w = nullptr;                    // proj_patch_kernel: project weights / bias padded to whole fragments
    float *pp_b = nullptr, *pp_br = nullptr;
};

// Output tile (TH x TWo) and channel chunk CC of the fused kernel, per B0 block (index 1..15):
// chosen so that E[P][CC] + the pool scratch stay <= 64 KB of LDS (>= 2 workgroups per CU) while
// the halo recompute and the per-chunk re-read of the (small) block input stay low.
struct FuseCfg { int TH, TWo, CC, TW, PB; };
static const FuseCfg B0_FUSE[16] = {
    {0, 0, 0, 0, 1},     {8, 8, 48, 2, 1},    {14, 14, 48, 2, 1},  {4, 14, 48, 2, 1},   {14, 14, 48, 2, 1},
    {7, 14, 80, 2, 1},   {14, 14, 96, 2, 1},  {14, 14, 96, 2, 1},  {14, 14, 48, 2, 1},  {14, 14, 48, 2, 1},
    {14, 14, 48, 2, 1},  {7, 7, 48, 1, 1},    {7, 7, 96, 1, 2},    {7, 7, 96, 1, 2},    {7, 7, 96, 1, 2},
    {7, 7, 96, 1, 2}};
// dot2 depthwise variant (mbconv_d_kernel): only where it measured faster (5x5 stride-1 blocks; MI355X, batch 128/256)
static const bool B0_DOT2[16] = {0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 1, 1, 1, 0};

// The same choices by layer geometry for the other members of the family (B4): the tile and chunk B0 uses at that
// resolution / stride / kernel size, with CC a divisor of the expanded width (5x5 layers at 14x14: CC 96 measured +1.3 %
// over 48).
static FuseCfg generic_fuse_cfg(int H, int k, int s, int ce)
{
    FuseCfg fc{0, 0, 0, 0, 1};
    if (H == 112 && s == 2) fc = {8, 8, 48, 2, 1};
    else if (H == 56 && s == 1) fc = {14, 14, 48, 2, 1};
    else if (H == 56 && s == 2) fc = {4, 14, 48, 2, 1};
    else if (H == 28 && s == 1) fc = {14, 14, 48, 2, 1};
    else if (H == 28 && s == 2) fc = {2, 14, 48, 2, 1};
    else if (H == 14 && s == 1) fc = {14, 14, 96, 2, 1};
    else if (H == 14 && s == 2) fc = {7, 7, 48, 1, 1};
    else if (H == 7 && s == 1) fc = {7, 7, 96, 1, 2};
    if (fc.CC && ce % fc.CC) fc.TH = 0;
    return fc;
}

// Geometry of block B (d, H filled in): pure arithmetic, no switch but `fuse` (whether a tile / chunk geometry is wanted)
static void block_geometry(BlockW& B, bool is_b0, int i, bool fuse)
{
    const int H = B.H, k = B.d.k, s = B.d.s;
    B.ce = B.d.cin * B.d.e;
    B.cs = B.d.cin / 4 > 1 ? B.d.cin / 4 : 1;
    B.cs4 = (B.cs + 3) / 4 * 4;
    B.has_expand = B.d.e != 1;
    B.skip = s == 1 && B.d.cin == B.d.cout;
    same_pad(H, k, s, &B.pad, &B.Ho);
    // depthwise (dwconv_kernel)
    B.tw = (B.Ho % 4 == 0) ? 4 : (B.Ho % 7 == 0 && B.Ho <= 7 ? 7 : 2);
    B.CG = B.ce / 8;
    B.nz = 1;
    while (B.CG / B.nz > 256 || B.CG % B.nz) ++B.nz;   // layers wider than 2048 channels: split the channel groups
    B.CG /= B.nz;
    B.S = 256 / B.CG > 0 ? 256 / B.CG : 1;
    const int strips = B.Ho * (B.Ho / B.tw);
    const int passes = (strips + B.S - 1) / B.S;
    B.iters = passes >= 8 ? 4 : 1;
    B.parts = (passes + B.iters - 1) / B.iters;
    // fused expand + depthwise (mbconv_a_kernel; mbconv_d_kernel's pair-aligned windows are a little wider)
    if (!B.has_expand || !fuse) return;
    const FuseCfg fc = is_b0 ? B0_FUSE[i] : generic_fuse_cfg(H, k, s, B.ce);
    if (!(fc.TH > 0 && B.Ho % fc.TH == 0 && B.Ho % fc.TWo == 0 && B.ce % fc.CC == 0 && fc.CC % 16 == 0)) return;
    MbArgs& a = B.mb;
    a.H = a.W = H; a.Cin = B.d.cin; a.Ce = B.ce; a.Ho = a.Wo = B.Ho; a.pad = B.pad; a.ks = k; a.stride = s;
    a.TH = fc.TH; a.TWo = fc.TWo; a.CC = fc.CC; a.tw = fc.TW;
    a.ksteps = (B.d.cin + 31) / 32;
    a.CCG = fc.CC / 8;
    a.S = 256 / a.CCG;
    a.tiles_x = B.Ho / fc.TWo; a.tiles_y = B.Ho / fc.TH;
    const int wh = std::min((fc.TH - 1) * s + k, H), wwid = std::min((fc.TWo - 1) * s + k, H);
    a.pb = fc.PB;
    const int ppad = (a.pb * wh * wwid + 15) / 16 * 16;
    a.npair = (ppad / 16 + 7) / 8;
    a.wfr_off = ppad * (fc.CC * 2 + 16);                       // E | taps+bias
    a.wl_off = a.wfr_off;
    a.lds_bytes = a.wl_off + (k * k + 1) * fc.CC * 4;
    a.red_off = 0;  // pool scratch [PB][S][CC] aliases E when it fits, else gets its own space
    if (a.pb * a.S * fc.CC * 4 > a.wfr_off) { a.red_off = a.lds_bytes; a.lds_bytes += a.pb * a.S * fc.CC * 4; }
    B.fusable = a.lds_bytes <= 128 * 1024 && fc.TWo % a.tw == 0;
    if (!B.fusable || !is_b0) return;
    int rowlen = 0;   // window of mbconv_d_kernel: rows as above, columns widened to whole pixel pairs (even absolute x)
    for (int tx = 0; tx < a.tiles_x; ++tx) {
        const int x0 = std::max(tx * fc.TWo * s - B.pad, 0), x1 = std::min((tx * fc.TWo + fc.TWo - 1) * s - B.pad + k, H);
        rowlen = std::max(rowlen, 2 * (((x1 + 1) >> 1) - (x0 >> 1)));
    }
    const int dpad = (a.pb * wh * rowlen + 15) / 16 * 16;
    const int np = (B.pad % 2 + s + k + 1) / 2;
    B.d_npair = (dpad / 16 + 7) / 8;
    B.d_wl_off = dpad * fc.CC * 2;
    B.d_lds = B.d_wl_off + k * 2 * np * fc.CC * 4 + fc.CC * 4;
    B.d_red_off = 0;
    if (a.pb * a.S * fc.CC * 4 > B.d_wl_off) { B.d_red_off = B.d_lds; B.d_lds += a.pb * a.S * fc.CC * 4; }
    B.d_fits = B.d_lds <= 128 * 1024;
}

struct Saved {
    void* dev = nullptr;
    size_t bytes = 0;
    size_t elems = 0;
    bool is_half = true;
};

#define MMC_GRAPH_CACHE 32   // captured (input, output, n) combinations kept per handle

struct mmc_backbone {
    int device = 0, max_batch = 0;
    int arch = MMC_ARCH_B0, nblk = 16, stem_ch = 32, head_in = 320, feat = 1280;
    Options opt;
    _Float16* stem_w = nullptr;
    float *stem_b = nullptr, *stem_pad = nullptr;
    std::vector<BlockW> blk;
    PwLayer head;
    // workspace: one lane per internal stream.  A pass over n patches is split into `nlanes` independent
    // sub-batches that run concurrently on their own HIP streams, so the latency-bound small launches of
    // one lane (squeeze-excite FCs, 7x7 layers) overlap the bandwidth/VALU-bound launches of the other.
    struct Lane {
        _Float16 *act0 = nullptr, *act1 = nullptr, *expbuf = nullptr, *dwbuf = nullptr;
        float *pool_part = nullptr, *gate = nullptr;
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
    };
    Lane lanes[4];
    // optional (MMC_GRAPH=1): a pass over device-resident buffers is captured once per (input, output, n) into a HIP graph
    // and replayed -- the ~20 launches per lane then cost one graph launch
    // (least recently used entry evicted beyond MMC_GRAPH_CACHE combinations)
    struct GraphEntry { const void* in; float* out; int n; hipGraphExec_t exec; };
    std::vector<GraphEntry> graphs;
    bool use_graph = false;
    int graph_warm = 0;
    // a (buffers, n) combination is captured the second time it is seen (ring of recent combinations): callers that
    // reuse their buffers (bench, BatchedExtractor's chunks, torch's caching allocator) get graphs, others plain launches
    struct SeenKey { const void* in; float* out; int n; };
    std::vector<SeenKey> seen;
    // combinations whose graph was evicted are NOT captured again (they run as plain launches from then on): a caller that
    // cycles through more combinations than the cache holds would otherwise pay capture + instantiate + destroy on every call.
    // After one full turnover of the cache (MMC_GRAPH_CACHE evictions) no new combination is captured at all.
    std::vector<SeenKey> evicted;
    int evictions = 0;
    long long captures = 0;
    hipStream_t gstream = nullptr;
    int nlanes = 1, lane_cap = 0;
    hipEvent_t fork = nullptr;
    uint8_t* in_stage = nullptr;
    float* out_stage = nullptr;
    size_t ws_bytes = 0;
    std::vector<void*> allocs;
    bool keep = false;
    bool fuse_stem = false;          // block 0's depthwise conv inside the stem launch (stem_dw_kernel): no stem tensor
    bool fuse_b0b1 = false;          // block 0's SE scale + project conv folded into block 1's kernel: no b0 output tensor
    TailRoute tail = TailRoute::None;
    int chain_first = -1, chain_last = -1;   // b<first>.projse .. b<last>.projse run as ONE chain14_kernel launch (-1: separate launches)
    int chain_cout = 0, chain_ce = 0;        // ... the widest block output / expanded tensor among them (see forward_lane)
    bool fp8 = false;                // MMC_PRECISION_FP8: project convs of the narrow late blocks on e4m3 MFMA operands
    float* dbg_clk = nullptr;        // keep mode: per-patch phase cycle counts of the patch-resident kernels
    float* mid_clk = nullptr;        // MMC_TAIL_CLK=1: [max_batch][8 workgroups][16] phase cycle counts of block 10's mid14 launch
    float* tail_clk = nullptr;       // MMC_TAIL_CLK=1: [max_batch][8 sections][8] phase cycle counts of the production tail7 launch
    _Float16 *b0_pre_w = nullptr, *b1_exp_pre = nullptr;   // fuse_b0b1: block 0's project as one MFMA fragment, block 1's K-permuted expand
    _Float16 *pre_wproj = nullptr, *head_wfrag = nullptr;  // tail7: block 11's project, the head conv (plain fragment order)
    TailBlock* tail_tab = nullptr;   // device table for tail7_kernel (blocks 12..15)
    std::map<std::string, Saved> saved;
    // One pass at a time per handle (lane workspaces, fork/done events and the staging buffers are shared): calls are
    // serialised on the host by `mu`, and a call on a different stream than the previous one waits for that one's work.
    std::mutex mu;
    hipEvent_t last_done = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_last = false;
};

// serialise against the previous call's device work when the caller switches streams; record this call's end
struct PassOrder {
    mmc_backbone* bb; hipStream_t st; bool armed = false;
    int begin()
    {
        if (bb->have_last && bb->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, bb->last_done, 0));
        armed = true;
        return 0;
    }
    ~PassOrder()
    {
        if (!armed) return;
        if (!bb->last_done && hipEventCreateWithFlags(&bb->last_done, hipEventDisableTiming) != hipSuccess) { bb->last_done = nullptr; return; }
        if (hipEventRecord(bb->last_done, st) == hipSuccess) { bb->last_stream = st; bb->have_last = true; }
    }
};

struct ProfEntry { std::string name; hipEvent_t e0, e1; };
struct Prof { std::vector<ProfEntry> entries; };

// ------------------------------------------------------------------------------------------
// blob parsing: header{magic,version,arch,n_tensors} + table{offset,nbytes} + fp32 tensors
// ------------------------------------------------------------------------------------------
struct BlobReader {
    const uint8_t* base;
    size_t nbytes;
    uint32_t n_tensors;
    const uint64_t* table;
    uint32_t next = 0;
    const float* take(size_t n_floats, const char* what, int* err)
    {
        if (next >= n_tensors) { *err = fail(MMC_ERR_WEIGHTS, "weights blob ended before %s", what); return nullptr; }
        const uint64_t off = table[2 * next], nb = table[2 * next + 1];
        if (off + nb > nbytes || nb != n_floats * sizeof(float)) {
            *err = fail(MMC_ERR_WEIGHTS, "tensor %u (%s): expected %zu bytes, blob has %llu", next, what,
                        n_floats * sizeof(float), (unsigned long long)nb);
            return nullptr;
        }
        ++next;
        return reinterpret_cast<const float*>(base + off);
    }
};

template <typename T>
static int dev_alloc(mmc_backbone* bb, T** p, size_t count)
{
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, count * sizeof(T) + 256);  // +256: vector tail reads stay in-bounds
    if (e != hipSuccess) return fail(MMC_ERR_NOMEM, "hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
    bb->allocs.push_back(d);
    bb->ws_bytes += count * sizeof(T);
    *p = reinterpret_cast<T*>(d);
    return 0;
}

template <typename T>
static int dev_upload(mmc_backbone* bb, T** p, const std::vector<T>& host)
{
    int r = dev_alloc(bb, p, host.size());
    if (r) return r;
    HIP_TRY(hipMemcpy(*p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// Pack a natural [N][K] fp32 1x1-conv weight into the fragment-ordered fp16 layout of pw_gemm_kernel:
// fragment (chunk, kstep, t) = 1 KB at ((chunk*KS32 + kstep)*nt + t)*512 halves; inside it lane
// (q*16 + m) holds W[channel(chunk, t, m)][kstep*32 + q*8 .. +8], with the row permutation
// fragment row (t*16 + 4qr + jr) <- channel (chunk*16nt + qr*4nt + 4t + jr).
static int pack_pw(mmc_backbone* bb, PwLayer* L, const float* w, const float* b, int N, int K, int nt, double wscale, double bscale)
{
    L->N = N;
    L->K = K;
    L->Kp = (K + 31) / 32 * 32;
    L->nt = nt;
    const int cw = 16 * L->nt;
    L->n_chunks = (N + cw - 1) / cw;
    const int Np = L->n_chunks * cw;
    const int ks32 = L->Kp / 32;
    std::vector<_Float16> wp((size_t)Np * L->Kp, (_Float16)0.0f);
    std::vector<float> bp(Np, 0.0f);
    for (int ch = 0; ch < L->n_chunks; ++ch)
        for (int ks = 0; ks < ks32; ++ks)
            for (int t = 0; t < L->nt; ++t)
                for (int m = 0; m < 16; ++m) {
                    const int c = ch * cw + (m >> 2) * 4 * L->nt + 4 * t + (m & 3);
                    if (c >= N) continue;
                    for (int q = 0; q < 4; ++q)
                        for (int j = 0; j < 8; ++j) {
                            const int k = ks * 32 + q * 8 + j;
                            if (k >= K) continue;
                            const size_t off = ((((size_t)ch * ks32 + ks) * L->nt + t) * 64 + (q * 16 + m)) * 8 + j;
                            wp[off] = (_Float16)(float)(w[(size_t)c * K + k] * wscale);
                        }
                }
    for (int c = 0; c < N; ++c) bp[c] = (float)(b[c] * bscale);
    int r = dev_upload(bb, &L->w, wp);
    if (r) return r;
    return dev_upload(bb, &L->b, bp);
}

extern "C" void mmc_backbone_destroy(mmc_backbone* bb)
{
    if (!bb) return;
    hipSetDevice(bb->device);
    for (void* p : bb->allocs) hipFree(p);
    for (auto& kv : bb->saved) hipFree(kv.second.dev);
    for (int l = 0; l < 4; ++l) {
        if (bb->lanes[l].stream) hipStreamDestroy(bb->lanes[l].stream);
        if (bb->lanes[l].done) hipEventDestroy(bb->lanes[l].done);
    }
    if (bb->fork) hipEventDestroy(bb->fork);
    if (bb->last_done) hipEventDestroy(bb->last_done);
    for (auto& g : bb->graphs) hipGraphExecDestroy(g.exec);
    if (bb->gstream) hipStreamDestroy(bb->gstream);
    delete bb;
}

extern "C" int mmc_backbone_create(const void* packed, size_t nbytes, int arch, int device, int max_batch,
                                   mmc_backbone** out)
{
    return mmc_backbone_create_ex(packed, nbytes, arch, device, max_batch, 0u, out);
}

// W[n][k] (rows of ld elements, n < N, k < K) times `scale` as fp16 in MFMA fragment order [nf][ks][64 lanes][8]: element (n, k)
// at ((n/16 * ks + k/32) * 64 + (k%32)/8 * 16 + n%16) * 8 + k%8 -- lane (q*16 + m) of fragment (f, kstep) holds
// W[16f + m][32 kstep + 8q .. +8].  Fragments and k-steps beyond the tensor stay zero.  (A source already in fp16 is only
// permuted: the expand weights keep the rounding of their natural fp16 rows.)
template <typename T>
static std::vector<_Float16> pack_frag(const T* w, int N, int K, int ld, int nf, int ks, double scale)
{
    std::vector<_Float16> wf((size_t)nf * ks * 512, (_Float16)0.0f);
    for (int c = 0; c < N; ++c)
        for (int k = 0; k < K; ++k)
            wf[((((size_t)(c / 16) * ks + k / 32) * 64) + ((k % 32) / 8) * 16 + (c % 16)) * 8 + (k % 8)] =
                (_Float16)(float)(w[(size_t)c * ld + k] * scale);
    return wf;
}

// 7x7 layers: few workgroups, deep K -> the gated GEMM overlaps its loads with MFMAs (pw_gemm's deferred-gate forms)
static int gemm_defer_gate(bool gate, int HW) { return (gate && HW <= 49) ? 1 : 0; }

// Looks up both pw_gemm forms layer L can take, whatever max_batch is (gemm_mt picks per call); the head's GAP form has one
static bool plan_gemm(PwLayer& L, int epi, bool gate, bool res, int HW)
{
    L.label[0] = pw_gemm_label(1, L.nt, epi, gate, res, gemm_defer_gate(gate, HW));
    L.label[1] = epi == EPI_GAP ? L.label[0] : pw_gemm_label(2, L.nt, epi, gate, res, 0);
    return L.label[0] && L.label[1] && (epi != EPI_GAP || HW <= 64);
}

// Plan block i (geometry done) under the handle's switches.  Pass-level choices (stem, b0/b1 fold, tail route) are in bb.
// Every templated launch it plans is looked up in that family's instantiation table (kernels.h) here, once: a shape
// without an instantiation takes the fallback where there is one and fails the create call where there is none.
static int plan_block(const mmc_backbone* bb, BlockW& B, int i)
{
    const Options& o = bb->opt;
    const bool is_b0 = bb->arch == MMC_ARCH_B0;
    const int HWo = B.Ho * B.Ho;
    const bool tail_blk = (bb->tail == TailRoute::B11All && i >= 11) || (bb->tail != TailRoute::None && i >= 12);
    // front half
    const bool mbt = o.fuse && o.mbt && (B.d.s == 1 || o.mbt2) && mbt_label(B.H, B.d.k, B.d.s, B.d.cin, B.ce, 0);
    const bool mid14 = is_b0 && o.fuse && o.projse && o.mid14 && i >= 6 && i <= 10 && mid14_label(B.d.cin, B.d.k, B.ce, 0);
    if (i == 0 && bb->fuse_stem) B.front = Front::StemDw;
    else if (tail_blk) B.front = Front::Tail;
    else if (B.fusable && mbt) B.front = Front::Mbt;
    else if (B.fusable && mid14) B.front = Front::Mid14;
    else if (B.fusable && is_b0 && o.mb_dot2 && B0_DOT2[i] && B.d_fits) B.front = Front::MbD;
    else if (B.fusable && i == 1 && bb->fuse_b0b1) B.front = o.mb1 ? Front::Mb1 : Front::MbPre;
    else if (B.fusable) B.front = Front::MbA;
    else B.front = Front::Unfused;
    B.mbt4 = B.front == Front::Mbt && o.mbt4 && B.ce % 16 == 0 && mbt_label(B.H, B.d.k, B.d.s, B.d.cin, B.ce, 1);
    B.mid14m = B.front == Front::Mid14 && o.mid14m && i >= 8 && B.ce % 16 == 0 && mid14_label(B.d.cin, B.d.k, B.ce, 1);
    if (B.front == Front::MbD) {
        B.mb.npair = B.d_npair; B.mb.wl_off = B.d_wl_off; B.mb.red_off = B.d_red_off; B.mb.lds_bytes = B.d_lds;
    }
    const char* family = nullptr;   // the front half's templated family, where a missing instantiation has no fallback
    const int tiles = B.mb.tiles_x * B.mb.tiles_y;
    switch (B.front) {
    case Front::StemDw: B.nparts = 49; break;
    case Front::Mb1: B.nparts = 14; break;
    case Front::Tail: B.nparts = B.parts; break;
    case Front::Mbt:
        B.nparts = B.d.s == 2 ? (B.Ho / 7) * (B.Ho / 14) : (B.H / 14) * (B.H / 28);
        B.front_label = mbt_label(B.H, B.d.k, B.d.s, B.d.cin, B.ce, B.mbt4);
        break;
    case Front::Mid14: B.nparts = 1; B.front_label = mid14_label(B.d.cin, B.d.k, B.ce, B.mid14m); break;
    case Front::MbPre: B.nparts = tiles; family = "mbconv_a PRE"; B.front_label = mbconv_pre_label(B.mb); break;
    case Front::MbD: B.nparts = tiles; family = "mbconv_d"; B.front_label = mbconv_d_label(B.mb); break;
    case Front::MbA: B.nparts = tiles; family = "mbconv_a"; B.front_label = mbconv_a_label(B.mb); break;
    case Front::Unfused:
        B.nparts = B.parts;
        family = "dwconv";
        B.front_label = dwconv_label(B.d.k, B.d.s, B.tw);
        if (B.front_label && B.has_expand && !plan_gemm(B.expand, EPI_SILU, false, false, B.H * B.H)) {
            family = "pw_gemm (expand)";
            B.front_label = nullptr;
        }
        break;
    }
    if (family && !B.front_label)
        return fail(MMC_ERR_ARG, "block %d: no %s instantiation for %dx%d, kernel %d, stride %d, %d -> %d channels (tile %dx%d, chunk %d)",
                    i, family, B.H, B.H, B.d.k, B.d.s, B.d.cin, B.ce, B.mb.TH, B.mb.TWo, B.mb.CC);
    // back half
    const bool fp8_blk = bb->fp8 && B.Ho <= o.fp8_maxh;
    const char* pp = proj_patch_label(B.ce, B.d.cout, HWo, B.skip ? 1 : 0);
    const bool proj_patch = o.fuse && o.projse && B.fusable && B.has_expand && B.cs4 <= 28 && pp && (is_b0 ? i >= 3 && i <= 10 : !fp8_blk);
    if (tail_blk || (i == 11 && bb->tail == TailRoute::B11)) B.back = Back::Tail;
    else if (proj_patch) B.back = Back::ProjPatch;
    else if (i == 0 && bb->fuse_b0b1) B.back = Back::SeFolded;
    else B.back = Back::SeProject;
    B.back_label = B.back == Back::ProjPatch ? pp : nullptr;
    B.se = !is_b0 ? Se::Wide : (o.se_small && B.ce <= 256 && B.cs <= 16) ? Se::Small : Se::Fused;
    // small-K, small-N project on a big image: thin_proj_kernel (up to 5 k-steps since the gate is folded into the weight
    // fragments: B0's b2 30.8 vs 43.7 us on pw_gemm; a shape without an instantiation stays on pw_gemm)
    PwLayer& P = B.project;
    const bool thin = o.thin_proj && P.nt == 2 && P.n_chunks == 1 && thin_proj_label(P.Kp / 32, B.skip ? 1 : 0) && P.N <= 32 &&
                      (P.N & 7) == 0 && (HWo & 15) == 0 && HWo >= 3136;
    B.proj = thin ? Proj::Thin : fp8_blk ? Proj::Fp8 : Proj::Gemm;
    if (B.back == Back::SeProject && B.proj == Proj::Gemm && !plan_gemm(P, EPI_LINEAR, true, B.skip, HWo))
        return fail(MMC_ERR_ARG, "block %d: no pw_gemm (project) instantiation for %d -> %d channels at %dx%d", i, B.ce, B.d.cout, B.Ho, B.Ho);
    // block 1's depthwise output as three 32-channel planes between mb1_kernel and thin_proj_kernel (see mb1_kernel); per-tensor
    // mode keeps the interleaved tensor it hands out
    B.planar = B.front == Front::Mb1 && thin && o.b1_planar && !o.keep && P.K == 96;
    return 0;
}

extern "C" int mmc_backbone_create_ex(const void* packed, size_t nbytes, int arch, int device, int max_batch, unsigned flags,
                                      mmc_backbone** out)
{
    if (!out) return fail(MMC_ERR_ARG, "out is NULL");
    if (flags & ~(unsigned)MMC_PRECISION_FP8) return fail(MMC_ERR_ARG, "unknown flags 0x%x", flags);
    if ((flags & MMC_PRECISION_FP8) && arch != MMC_ARCH_B4)
        return fail(MMC_ERR_ARG, "MMC_PRECISION_FP8 is implemented for MMC_ARCH_B4 (BASELINE configs[4]): B0's late blocks run fused kernels without a separate project GEMM");
    *out = nullptr;
    if (!packed || nbytes < 16) return fail(MMC_ERR_WEIGHTS, "weights blob is empty");
    if (arch != MMC_ARCH_B0 && arch != MMC_ARCH_B4) return fail(MMC_ERR_ARG, "unsupported arch %d (MMC_ARCH_B0 or MMC_ARCH_B4)", arch);
    if (max_batch < 1 || max_batch > 4096) return fail(MMC_ERR_ARG, "max_batch %d out of range [1,4096]", max_batch);
    const uint8_t* base = static_cast<const uint8_t*>(packed);
    uint32_t hdr[4];
    memcpy(hdr, base, 16);
    if (memcmp(base, "MMCW", 4) != 0) return fail(MMC_ERR_WEIGHTS, "bad magic in weights blob");
    if (hdr[1] != 1) return fail(MMC_ERR_WEIGHTS, "weights blob version %u, expected 1", hdr[1]);
    if ((int)hdr[2] != arch) return fail(MMC_ERR_WEIGHTS, "weights blob arch %u != requested %d", hdr[2], arch);
    const uint32_t nt = hdr[3];
    if (16 + (size_t)nt * 16 > nbytes) return fail(MMC_ERR_WEIGHTS, "weights blob truncated (table)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(MMC_ERR_HIP, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(MMC_ERR_ARG, "device %d out of range (%d visible)", device, ndev);
    HIP_TRY(hipSetDevice(device));

    mmc_backbone* bb = new mmc_backbone();
    bb->device = device;
    bb->max_batch = max_batch;
    bb->fp8 = (flags & MMC_PRECISION_FP8) != 0;
    bb->opt = read_options();
    const Options& o = bb->opt;
    const ArchDef AD = make_arch(arch);
    const bool is_b0 = arch == MMC_ARCH_B0;
    const int STEM_CH = AD.stem, HEAD_IN = AD.head_in, FEAT = AD.feat, NBLK = (int)AD.blocks.size();
    bb->arch = arch; bb->nblk = NBLK; bb->stem_ch = STEM_CH; bb->head_in = HEAD_IN; bb->feat = FEAT;
    bb->blk.resize(NBLK);
    bb->keep = o.keep;
    bb->use_graph = o.graph;
#define TRY_OR_FREE(expr)                          \
    do { int r__ = (expr); if (r__) { mmc_backbone_destroy(bb); return r__; } } while (0)
    if (bb->keep) TRY_OR_FREE(dev_alloc(bb, &bb->dbg_clk, (size_t)max_batch * 8));
    if (o.tail_clk) {
        // rows are indexed lane * lane_cap + row with lane_cap = ceil(max_batch / lanes): up to lanes - 1 <= 3 rows more than max_batch
        const size_t clk_rows = (size_t)max_batch + 4;
        TRY_OR_FREE(dev_alloc(bb, &bb->tail_clk, clk_rows * 64));
        hipMemset(bb->tail_clk, 0, clk_rows * 64 * sizeof(float));
        TRY_OR_FREE(dev_alloc(bb, &bb->mid_clk, clk_rows * 128));
        hipMemset(bb->mid_clk, 0, clk_rows * 128 * sizeof(float));
        bb->use_graph = false;
    }

    // ---- 1. geometry: per block, pure arithmetic ----
    for (int i = 0, H = IMG / 2; i < NBLK; ++i) {
        BlockW& B = bb->blk[i];
        B.d = AD.blocks[i];
        B.H = H;
        block_geometry(B, is_b0, i, o.fuse);
        B.expand.nt = pick_nt(B.ce, false);   // pack_pw's layouts (the plan reads them)
        B.project.N = B.d.cout;
        B.project.K = B.ce;
        B.project.Kp = (B.ce + 31) / 32 * 32;
        B.project.nt = pick_nt(B.d.cout, B.Ho <= 14);
        B.project.n_chunks = (B.d.cout + 16 * B.project.nt - 1) / (16 * B.project.nt);
        H = B.Ho;
    }
    // ---- 2. plan: pass-level routes, then each block ----
    {
        const std::vector<BlockW>& K = bb->blk;
        bb->fuse_stem = is_b0 && o.fuse;
        // block 0's project as one MFMA fragment in block 1's kernel: the tile of mbconv_a_kernel PRE / mb1_kernel
        const MbArgs& m1 = K[1].mb;
        bb->fuse_b0b1 = o.fuse_b0 && bb->fuse_stem && K[0].ce == 32 && K[0].d.cout == 16 && K[1].d.cin == 16 && K[1].fusable &&
                        !(o.mb_dot2 && B0_DOT2[1] && K[1].d_fits) && m1.TH == 8 && m1.TWo == 8 && m1.CC == 48 && m1.tw == 2 &&
                        m1.pb == 1 && m1.npair == 3;
        // tail7_kernel: blocks 12..15 at 7x7 (192 -> 1152 -> 192 / 320, SE width 48); block 11's back half (672 -> 192, SE width
        // 28) and the head; block 11's front half (5x5 stride 2 from 14x14)
        bool t12 = is_b0 && o.fuse && o.tail && NBLK == 16;
        for (int i = 12; i <= 15 && t12; ++i)
            t12 = K[i].fusable && K[i].H == 7 && K[i].d.s == 1 && K[i].d.cin == 192 && K[i].ce == 1152 && K[i].cs == 48;
        const BlockW& B11 = K[11 < NBLK ? 11 : 0];
        const bool t11 = t12 && o.tail_full && HEAD_IN % 32 == 0 && B11.fusable && B11.ce == 672 && B11.d.cout == 192 &&
                         B11.cs4 == 28 && B11.mb.tiles_x * B11.mb.tiles_y == 1;
        const bool t11all = t11 && o.tail_b11 && !o.keep && B11.mb.ksteps == 4 && B11.d.k == 5 && B11.d.s == 2 && B11.H == 14;
        bb->tail = t11all ? TailRoute::B11All : t11 ? TailRoute::B11 : t12 ? TailRoute::B12 : TailRoute::None;
        for (int i = 0; i < NBLK; ++i) TRY_OR_FREE(plan_block(bb, bb->blk[i], i));
        // chain14_kernel: the maximal run of consecutive launches that are one workgroup per patch on a body the chain kernel holds
        // (proj_patch, or mid14m with nsplit 1).  Launch 2 i is block i's front half, 2 i + 1 its back half.  Per-tensor mode and the
        // debug clocks keep separate launches.
        if (o.chain && is_b0 && !o.keep && !o.tail_clk) {
            auto chainable = [&](int l) {
                const BlockW& B = K[l >> 1];
                if (l & 1) return B.back == Back::ProjPatch && chain14_proj_kind(B.ce, B.d.cout, B.Ho * B.Ho, B.skip ? 1 : 0) >= 0;
                return B.front == Front::Mid14 && B.mid14m && chain14_mid_kind(B.d.cin, B.d.k, B.ce) >= 0;
            };
            int best0 = 0, bestn = 0;
            for (int l = 0, run = 0; l < 2 * NBLK; ++l) {
                run = chainable(l) ? run + 1 : 0;
                if (run > bestn) { bestn = run; best0 = l - run + 1; }
            }
            // only the schedule the chain was built and measured for, b7.projse .. b10.projse: any other run (MMC_MID14M=0,
            // MMC_PROJSE=0, ...) stays separate launches
            // ... whose tensors come in at most two row widths per buffer, the first block's and a wider one (forward_lane places them)
            bool two = K[7].skip;
            int cw = K[7].d.cout, ew = K[7].ce;
            for (int i = 8; i <= 10; ++i) { cw = std::max(cw, K[i].d.cout); ew = std::max(ew, K[i].ce); }
            for (int i = 8; i <= 10; ++i)
                two = two && (K[i].d.cout == K[7].d.cout || K[i].d.cout == cw) && (K[i].ce == K[7].ce || K[i].ce == ew);
            if (bestn == CHAIN14_MAX_PHASES && best0 == 2 * 7 + 1 && two) {
                bb->chain_first = 7; bb->chain_last = 10; bb->chain_cout = cw; bb->chain_ce = ew;
            }
        }
        bb->head.nt = 4;
        const int HWh = K[NBLK - 1].Ho * K[NBLK - 1].Ho;
        if (bb->tail != TailRoute::B11 && bb->tail != TailRoute::B11All && !plan_gemm(bb->head, EPI_GAP, false, false, HWh)) {
            mmc_backbone_destroy(bb);
            return fail(MMC_ERR_ARG, "head: no pw_gemm (average pool) instantiation for nt %d at %d pixels per patch", bb->head.nt, HWh);
        }
    }

    // ---- 3. packing: what the plan launches, reading the blob's tensors in their fixed order ----
    std::vector<uint64_t> table(2 * (size_t)nt);
    memcpy(table.data(), base + 16, (size_t)nt * 16);
    BlobReader rd{base, nbytes, nt, table.data()};
    int err = 0;
#define TAKE(var, n, what)                         \
    const float* var = rd.take((n), what, &err);   \
    if (!var) { mmc_backbone_destroy(bb); return err; }

    // ---- stem: [Cstem][27] folded (ky,kx,c), bias[Cstem], padval[3] ----
    {
        TAKE(w, (size_t)STEM_CH * 27, "stem.weight");
        TAKE(b, STEM_CH, "stem.bias");
        TAKE(pv, 3, "stem.padval");
        const int snt = STEM_CH / 16;   // output fragments: lane quarter q owns channels q*4*snt + 4t + j
        std::vector<_Float16> wp((size_t)STEM_CH * 32, (_Float16)0.0f);
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
        TRY_OR_FREE(dev_upload(bb, &bb->stem_w, wp));
        std::vector<float> sb(STEM_CH);
        for (int c = 0; c < STEM_CH; ++c) sb[c] = (float)(b[c] * LOG2E);
        TRY_OR_FREE(dev_upload(bb, &bb->stem_b, sb));
        std::vector<float> pvv = {pv[0], pv[1], pv[2], 0.f};
        TRY_OR_FREE(dev_upload(bb, &bb->stem_pad, pvv));
    }
    // ---- blocks ----
    size_t max_act = (size_t)(IMG / 2) * (IMG / 2) * STEM_CH, max_exp = 0, max_dw = 0, max_pool = 0;
    int max_c = 0;
    for (int i = 0; i < NBLK; ++i) {
        BlockW& B = bb->blk[i];
        const int H = B.H;
        const bool tail_blk = B.front == Front::Tail && i >= 12;               // a row of tail7's block table
        const bool tail_pre = i == 11 && bb->tail != TailRoute::None && bb->tail != TailRoute::B12;   // tail7's block 11
        const bool frag_exp = B.front == Front::Mbt || B.front == Front::Mid14 || tail_blk || (tail_pre && bb->tail == TailRoute::B11All);
        char nm[64];
        if (B.has_expand) {
            snprintf(nm, sizeof nm, "b%d.expand", i);
            TAKE(w, (size_t)B.ce * B.d.cin, nm);
            TAKE(b, B.ce, nm);
            TRY_OR_FREE(pack_pw(bb, &B.expand, w, b, B.ce, B.d.cin, B.expand.nt, LOG2E, LOG2E));
            const int kp = 32 * B.mb.ksteps;
            std::vector<_Float16> wn((size_t)B.ce * kp, (_Float16)0.0f);   // natural rows, K zero padded
            for (int c = 0; c < B.ce && B.fusable; ++c)
                for (int k = 0; k < B.d.cin; ++k) wn[(size_t)c * kp + k] = (_Float16)(float)(w[(size_t)c * B.d.cin + k] * LOG2E);
            if (B.front == Front::MbA || B.front == Front::MbD) TRY_OR_FREE(dev_upload(bb, &B.exp_nat, wn));
            if (B.front == Front::Mb1 || B.front == Front::MbPre) {
                // K-permuted copy for block 0's folded project: MFMA slot 8q+j holds input channel 4q+j (j < 4), the rest zero --
                // the layout block 0's in-kernel project leaves in the lanes
                std::vector<_Float16> wq((size_t)B.ce * 32, (_Float16)0.0f);
                for (int c = 0; c < B.ce; ++c)
                    for (int qq = 0; qq < 4; ++qq)
                        for (int j = 0; j < 4; ++j) wq[(size_t)c * 32 + 8 * qq + j] = wn[(size_t)c * kp + 4 * qq + j];
                TRY_OR_FREE(dev_upload(bb, &bb->b1_exp_pre, wq));
            }
            if (frag_exp) TRY_OR_FREE(dev_upload(bb, &B.exp_frag, pack_frag(wn.data(), B.ce, B.d.cin, kp, B.ce / 16, B.mb.ksteps, 1.0)));
        }
        {
            snprintf(nm, sizeof nm, "b%d.dw", i);
            TAKE(w, (size_t)B.ce * B.d.k * B.d.k, nm);  // [ce][k][k]
            TAKE(b, B.ce, nm);
            const int kk = B.d.k * B.d.k;
            // the taps see a log2(e)-scaled input (stem or expand output) and produce a scaled output: the factors cancel --
            // except for an expand-less block fed by a project conv (B4's block 1), whose input is in the plain domain
            const double tsc = (B.has_expand || i == 0) ? 1.0 : LOG2E;
            std::vector<float> wt((size_t)kk * B.ce);
            for (int c = 0; c < B.ce; ++c)
                for (int t = 0; t < kk; ++t) wt[(size_t)t * B.ce + c] = (float)(w[(size_t)c * kk + t] * tsc);
            TRY_OR_FREE(dev_upload(bb, &B.dw_w, wt));
            std::vector<float> db(B.ce);
            for (int c = 0; c < B.ce; ++c) db[c] = (float)(b[c] * LOG2E);
            TRY_OR_FREE(dev_upload(bb, &B.dw_b, db));
            const bool dwp4 = B.front == Front::Mid14 || tail_blk || (tail_pre && bb->tail == TailRoute::B11All);
            if (B.front == Front::Mbt || dwp4) {
                // taps of tail7_kernel / mid14_kernel / mbt_kernel as fp16 pairs: kernel row ky = (k0,k1), (k2,k3), (k4,0); the kernel derives the
                // odd-output pairs by shifts, giving the same values as mbconv_d_kernel's wl2 table
                std::vector<uint32_t> dp((size_t)15 * B.ce, 0u);
                auto tap = [&](int c, int ky, int kx) -> _Float16 {
                    return kx < B.d.k ? (_Float16)w[(size_t)c * kk + ky * B.d.k + kx] : (_Float16)0.0f;
                };
                for (int c = 0; c < B.ce; ++c)
                    for (int ky = 0; ky < B.d.k; ++ky)
                        for (int d = 0; d < 3; ++d) {   // slot 3*ky + d holds taps (2d, 2d+1) of kernel row ky
                            _Float16 h[2] = {tap(c, ky, 2 * d), tap(c, ky, 2 * d + 1)};
                            uint32_t u;
                            memcpy(&u, h, 4);
                            dp[(size_t)(ky * 3 + d) * B.ce + c] = u;
                        }
                if (B.front == Front::Mbt) TRY_OR_FREE(dev_upload(bb, &B.t_dwp, dp));
                if (dwp4) {
                    // the same 15 dwords + the bias (as the 16th) in 16-byte requests: [4][ce][4] -- request j of channel c holds slots
                    // 4j .. 4j+3; a wave's request is 1 KB contiguous (16 dword loads per thread were 16 wave-instructions of 256 bytes)
                    std::vector<uint32_t> dp4((size_t)16 * B.ce, 0u);
                    for (int c = 0; c < B.ce; ++c)
                        for (int t = 0; t < 16; ++t) {
                            uint32_t v = 0u;
                            if (t < 15) v = dp[(size_t)t * B.ce + c];
                            else memcpy(&v, &db[c], 4);   // the bias exactly as dw_b holds it
                            dp4[((size_t)(t / 4) * B.ce + c) * 4 + (t % 4)] = v;
                        }
                    TRY_OR_FREE(dev_upload(bb, &B.t_dwp4, dp4));
                }
            }
            if (B.mbt4 || B.mid14m) {
                // Depthwise on the matrix pipe (v_mfma_f32_4x4x4_16B_f16: 16 independent blocks = 16 channels).  A operand
                // of block c, kernel row ky, input quad h (columns x0 - 2 + 4h .. +3 of an output tile x0 .. x0+3): the Toeplitz slice
                // A[i][k] = w[c][ky][k - i + 4h - 2 + R] (zero outside 0 .. K-1), lane 4 blk + i holding k = 0 .. 3, block blk = channel
                // 2 (blk & 3) + ((blk >> 2) & 1) + 8 (blk >> 3) of the group (channels 2k, 2k+1 in neighbouring 16-lane rows: the kernel
                // pairs them with v_permlane16_swap).
                const int K = B.d.k, R = K / 2, ngr = B.ce / 16;
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
                TRY_OR_FREE(dev_upload(bb, &B.dw_diag, dd));
            }
        }
        {
            snprintf(nm, sizeof nm, "b%d.se", i);
            TAKE(wr, (size_t)B.cs * B.ce, nm);
            TAKE(br, B.cs, nm);
            TAKE(we, (size_t)B.ce * B.cs, nm);
            TAKE(be, B.ce, nm);
            const bool se_launch = B.back == Back::SeProject || B.back == Back::SeFolded;
            const double psc = 1.0 / ((double)B.Ho * B.Ho * LOG2E);   // FC1 on pooled sums of HW log2(e)-scaled activations
            if (se_launch && B.se == Se::Fused) {
                // Squeeze-excite weights, fp32 in MFMA fragment order (se_fused_kernel): 3 output/k fragments of 16 cover Cs <= 48
                const int ng = B.ce / 16;
                std::vector<float> wrp((size_t)ng * 3 * 64 * 4 + 4, 0.f), wep((size_t)ng * 3 * 64 * 4 + 4, 0.f);
                for (int g = 0; g < ng; ++g)
                    for (int t = 0; t < 3; ++t)
                        for (int ln = 0; ln < 64; ++ln)
                            for (int e = 0; e < 4; ++e) {
                                const int ii = ln & 15, qq = ln >> 4;
                                const size_t off = (((size_t)g * 3 + t) * 64 + ln) * 4 + e;
                                const int j = 16 * t + ii, c = 16 * g + 4 * qq + e;         // FC1: Wr[j][c]
                                if (j < B.cs) wrp[off] = (float)(wr[(size_t)j * B.ce + c] * psc);
                                const int n = 16 * g + ii, k = 16 * t + 4 * qq + e;         // FC2: We[n][k] (T = g, k-group = t)
                                if (k < B.cs) wep[off] = we[(size_t)n * B.cs + k];
                            }
                TRY_OR_FREE(dev_upload(bb, &B.se_wrp, wrp));
                TRY_OR_FREE(dev_upload(bb, &B.se_wep, wep));
            }
            if (se_launch && B.se != Se::Fused) {   // natural fp32 rows: se_small_kernel; se_wide_kernel reads the excite FC transposed
                std::vector<float> wrn((size_t)B.cs * B.ce);
                for (size_t e = 0; e < wrn.size(); ++e) wrn[e] = (float)(wr[e] * psc);
                TRY_OR_FREE(dev_upload(bb, &B.se_wr_nat, wrn));
                if (B.se == Se::Small) {
                    TRY_OR_FREE(dev_upload(bb, &B.se_we_nat, std::vector<float>(we, we + (size_t)B.ce * B.cs)));
                } else {   // [Cs][C]: neighbouring lanes, neighbouring words
                    std::vector<float> wet((size_t)B.cs * B.ce);
                    for (int c = 0; c < B.ce; ++c)
                        for (int j = 0; j < B.cs; ++j) wet[(size_t)j * B.ce + c] = we[(size_t)c * B.cs + j];
                    TRY_OR_FREE(dev_upload(bb, &B.se_we_nat, wet));
                }
                TRY_OR_FREE(dev_upload(bb, &B.se_br_nat, std::vector<float>(br, br + B.cs)));
            }
            if (B.back == Back::ProjPatch || tail_pre || tail_blk) {
                // fp16, transposed for matrix-vector use: Wr^T [ce][csp], We^T [csp][ce] (csp = Cs padded to 4)
                const int csp = B.cs4;
                std::vector<_Float16> wrt((size_t)B.ce * csp, (_Float16)0.0f), wet((size_t)csp * B.ce, (_Float16)0.0f);
                for (int c = 0; c < B.ce; ++c)
                    for (int j = 0; j < B.cs; ++j) {
                        wrt[(size_t)c * csp + j] = (_Float16)wr[(size_t)j * B.ce + c];
                        wet[(size_t)j * B.ce + c] = (_Float16)we[(size_t)c * B.cs + j];
                    }
                if (B.back == Back::ProjPatch || tail_pre) {
                    TRY_OR_FREE(dev_upload(bb, &B.t_wr, wrt));
                    TRY_OR_FREE(dev_upload(bb, &B.t_we, wet));
                    std::vector<float> brp(csp > 32 ? csp : 32, 0.f);
                    for (int j = 0; j < B.cs; ++j) brp[j] = br[j];
                    TRY_OR_FREE(dev_upload(bb, &B.pp_br, brp));
                }
                if (B.back == Back::ProjPatch) {
                    // proj_patch_kernel's FC1: [group of four outputs][channel row][4] (ProjPatchArgs::wr_g), zero beyond ce
                    const int rows = proj_patch_fc1_rows(B.ce);
                    std::vector<_Float16> wrg((size_t)(csp / 4) * rows * 4, (_Float16)0.0f);
                    for (int g = 0; g < csp / 4; ++g)
                        for (int c = 0; c < B.ce; ++c)
                            for (int e = 0; e < 4; ++e) wrg[((size_t)g * rows + c) * 4 + e] = wrt[(size_t)c * csp + 4 * g + e];
                    TRY_OR_FREE(dev_upload(bb, &B.t_wrg, wrg));
                }
                if (tail_blk) {
                    // tail7_kernel's 16-byte request layout (TailBlock::wr_t / we_t): two rows of the transposed matrices per request
                    std::vector<_Float16> wr2((size_t)18 * 384 * 8), we2((size_t)24 * 288 * 8);
                    for (int p = 0; p < 18; ++p)
                        for (int t = 0; t < 384; ++t)
                            for (int e = 0; e < 8; ++e) {
                                const int cr = t / 12, j4 = t % 12, c = 64 * p + (e < 4 ? 0 : 32) + cr;
                                wr2[((size_t)p * 384 + t) * 8 + e] = wrt[(size_t)c * csp + 4 * j4 + (e & 3)];
                            }
                    for (int p = 0; p < 24; ++p)
                        for (int t = 0; t < 288; ++t)
                            for (int e = 0; e < 8; ++e) we2[((size_t)p * 288 + t) * 8 + e] = wet[(size_t)(2 * p + (e < 4 ? 0 : 1)) * B.ce + 4 * t + (e & 3)];
                    TRY_OR_FREE(dev_upload(bb, &B.t_wr2, wr2));
                    TRY_OR_FREE(dev_upload(bb, &B.t_we2, we2));
                }
            }
            if ((se_launch && B.se == Se::Fused) || tail_blk) {   // se_fused_kernel's and tail7's FC1 bias, zero padded to 48
                std::vector<float> brs(B.cs > 48 ? B.cs : 48, 0.f);
                for (int j = 0; j < B.cs; ++j) brs[j] = br[j];
                TRY_OR_FREE(dev_upload(bb, &B.se_br, brs));
            }
            TRY_OR_FREE(dev_upload(bb, &B.se_be, std::vector<float>(be, be + B.ce)));
        }
        {
            snprintf(nm, sizeof nm, "b%d.project", i);
            TAKE(w, (size_t)B.d.cout * B.ce, nm);
            TAKE(b, B.d.cout, nm);
            TRY_OR_FREE(pack_pw(bb, &B.project, w, b, B.d.cout, B.ce, B.project.nt, 1.0 / LOG2E, 1.0));
            if (B.proj == Proj::Fp8 && (B.back == Back::SeProject || B.back == Back::SeFolded)) {
                // e4m3 weights for pw_gemm_fp8_kernel: per-output-channel scale amax / 448 (the 1 / log2 e of the scaled domain rides in the
                // scale), fragment f = channels 16 f .. +15, k-step of 128, lane (i, q) holds k = 128 ks + 32 q .. +31 of channel 16 f + i
                Fp8Layer& L = B.p8;
                L.N = B.d.cout; L.K = B.ce; L.KS128 = (B.ce + 127) / 128; L.NFp = ((B.d.cout + 15) / 16 + 6) / 7 * 7;
                std::vector<uint8_t> w8((size_t)L.NFp * L.KS128 * 64 * 32, (uint8_t)0);
                std::vector<float> sw((size_t)16 * L.NFp, 0.0f), bp((size_t)16 * L.NFp, 0.0f);
                for (int nn = 0; nn < L.N; ++nn) {
                    float amax = 0.f;
                    for (int k = 0; k < L.K; ++k) amax = std::max(amax, std::fabs(w[(size_t)nn * L.K + k]));
                    const float sc = amax > 0.f ? amax / 448.0f : 1.0f;
                    sw[nn] = (float)(sc / LOG2E);
                    bp[nn] = b[nn];
                    for (int k = 0; k < L.K; ++k) {
                        const int f = nn / 16, ii = nn % 16, ks = k / 128, qq = (k % 128) / 32, e = k % 32;
                        w8[((((size_t)f * L.KS128 + ks) * 64) + qq * 16 + ii) * 32 + e] = e4m3_encode(w[(size_t)nn * L.K + k] / sc);
                    }
                }
                TRY_OR_FREE(dev_upload(bb, &L.w8, w8));
                TRY_OR_FREE(dev_upload(bb, &L.sw, sw));
                TRY_OR_FREE(dev_upload(bb, &L.b, bp));
            }
            if (B.back == Back::SeFolded)   // block 0's project conv as ONE MFMA fragment (16 outputs x 32 inputs)
                TRY_OR_FREE(dev_upload(bb, &bb->b0_pre_w, pack_frag(w, 16, 32, 32, 1, 1, 1.0 / LOG2E)));
            if (B.back == Back::ProjPatch) {   // proj_patch_kernel: K and N zero-padded to whole fragments
                const int nf = (B.d.cout + 15) / 16;
                TRY_OR_FREE(dev_upload(bb, &B.pp_w, pack_frag(w, B.d.cout, B.ce, B.ce, nf, proj_patch_ksteps(B.ce), 1.0 / LOG2E)));
                std::vector<float> bp((size_t)16 * nf, 0.f);
                for (int c = 0; c < B.d.cout; ++c) bp[c] = b[c];
                TRY_OR_FREE(dev_upload(bb, &B.pp_b, bp));
            }
            if (tail_pre)   // tail7 pre-block: [12][24][64][8], k-steps 21..23 zero (its k-loop runs 4 steps at a time)
                TRY_OR_FREE(dev_upload(bb, &bb->pre_wproj, pack_frag(w, B.d.cout, B.ce, B.ce, 12, 24, 1.0 / LOG2E)));
            if (tail_blk)
                TRY_OR_FREE(dev_upload(bb, &B.t_wproj, pack_frag(w, B.d.cout, B.ce, B.ce, B.d.cout / 16, B.ce / 32, 1.0 / LOG2E)));
        }
        if (B.fusable) max_pool = std::max(max_pool, (size_t)B.mb.tiles_x * B.mb.tiles_y * B.ce);
        if ((size_t)H * H * B.ce > max_exp && B.has_expand && !B.fusable) max_exp = (size_t)H * H * B.ce;
        max_dw = std::max(max_dw, (size_t)B.Ho * B.Ho * B.ce);
        max_act = std::max(max_act, (size_t)B.Ho * B.Ho * B.d.cout);
        max_pool = std::max(max_pool, (size_t)B.parts * B.ce);
        if (i == 0) max_pool = std::max(max_pool, (size_t)49 * B.ce);
        max_c = std::max(max_c, B.ce);
    }
    {
        TAKE(w, (size_t)FEAT * HEAD_IN, "head.weight");
        TAKE(b, FEAT, "head.bias");
        TRY_OR_FREE(pack_pw(bb, &bb->head, w, b, FEAT, HEAD_IN, bb->head.nt, LOG2E, LOG2E));
        if (bb->tail == TailRoute::B11 || bb->tail == TailRoute::B11All)   // the same weights in plain fragment order for tail7's head phase
            TRY_OR_FREE(dev_upload(bb, &bb->head_wfrag, pack_frag(w, FEAT, HEAD_IN, HEAD_IN, FEAT / 16, HEAD_IN / 32, LOG2E)));
    }
    if (bb->tail != TailRoute::None) {
        std::vector<TailBlock> tab(4);
        for (int j = 0; j < 4; ++j) {
            const BlockW& B = bb->blk[12 + j];
            tab[j] = TailBlock{B.exp_frag, B.expand.b, B.t_dwp4, B.dw_b, B.t_wr2, B.se_br, B.t_we2, B.se_be, B.t_wproj, B.project.b,
                               B.d.cout, B.d.k};
        }
        TRY_OR_FREE(dev_upload(bb, &bb->tail_tab, tab));
    }
    if (rd.next != nt) {
        mmc_backbone_destroy(bb);
        return fail(MMC_ERR_WEIGHTS, "weights blob has %u tensors, expected %u", nt, rd.next);
    }
    if (bb->chain_first >= 0) {   // room for the chained launch's second tensor per buffer (the 112 x 112 layers already need more)
        const size_t hw = (size_t)bb->blk[bb->chain_first].Ho * bb->blk[bb->chain_first].Ho;
        max_act = std::max(max_act, 2 * hw * bb->chain_cout);
        max_dw = std::max(max_dw, 2 * hw * bb->chain_ce);
        max_pool = std::max(max_pool, (size_t)2 * bb->chain_ce);
    }
    const size_t mb = (size_t)max_batch;
    {
        int nl = std::max(1, std::min(o.lanes, 4));
        if (bb->keep || max_batch < 2 * nl) nl = 1;
        bb->nlanes = nl;
        bb->lane_cap = (max_batch + nl - 1) / nl;
        const size_t lc = (size_t)bb->lane_cap;
        for (int l = 0; l < nl; ++l) {
            mmc_backbone::Lane& L = bb->lanes[l];
            TRY_OR_FREE(dev_alloc(bb, &L.act0, lc * max_act));
            TRY_OR_FREE(dev_alloc(bb, &L.act1, lc * max_act));
            TRY_OR_FREE(dev_alloc(bb, &L.expbuf, lc * (max_exp ? max_exp : 64)));
            TRY_OR_FREE(dev_alloc(bb, &L.dwbuf, lc * max_dw));
            TRY_OR_FREE(dev_alloc(bb, &L.pool_part, lc * max_pool));
            TRY_OR_FREE(dev_alloc(bb, &L.gate, lc * (size_t)max_c));
            if (nl > 1) {
                if (hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking) != hipSuccess ||
                    hipEventCreateWithFlags(&L.done, hipEventDisableTiming) != hipSuccess) {
                    mmc_backbone_destroy(bb);
                    return fail(MMC_ERR_HIP, "cannot create internal stream/event");
                }
            }
        }
        if (nl > 1 && hipEventCreateWithFlags(&bb->fork, hipEventDisableTiming) != hipSuccess) {
            mmc_backbone_destroy(bb);
            return fail(MMC_ERR_HIP, "cannot create fork event");
        }
    }
    TRY_OR_FREE(dev_alloc(bb, &bb->in_stage, mb * (size_t)IMG * IMG * 3));
    TRY_OR_FREE(dev_alloc(bb, &bb->out_stage, mb * (size_t)FEAT));
#undef TAKE
#undef TRY_OR_FREE
    *out = bb;
    return MMC_OK;
}

extern "C" int mmc_feature_dim(const mmc_backbone* bb) { return bb ? bb->feat : 0; }
int mmc_backbone_device(const mmc_backbone* bb) { return bb->device; }
extern "C" int mmc_backbone_max_batch(const mmc_backbone* bb) { return bb ? bb->max_batch : 0; }
extern "C" int mmc_backbone_lanes(const mmc_backbone* bb) { return bb ? bb->nlanes : 0; }
extern "C" size_t mmc_backbone_workspace_bytes(const mmc_backbone* bb) { return bb ? bb->ws_bytes : 0; }

// ------------------------------------------------------------------------------------------
// the launch schedule for one pass over n <= max_batch resident patches
// ------------------------------------------------------------------------------------------
static int save_act(mmc_backbone* bb, const char* name, const void* dev, size_t elems, bool is_half, hipStream_t st)
{
    Saved& s = bb->saved[name];
    const size_t bytes = elems * (is_half ? 2 : 4);
    if (s.bytes < bytes) {
        if (s.dev) hipFree(s.dev);
        HIP_TRY(hipMalloc(&s.dev, bytes));
        s.bytes = bytes;
    }
    s.elems = elems;
    s.is_half = is_half;
    HIP_TRY(hipMemcpyAsync(s.dev, dev, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
}

static int gemm_mt(const PwLayer& L, int M)
{
    // two row fragments per wave when that still leaves >= ~4 workgroups per CU
    const long wgs2 = ((long)M + 127) / 128 * L.n_chunks;
    return wgs2 >= 1024 ? 2 : 1;
}

static int run_gemm(const PwLayer& L, const _Float16* X, int M, _Float16* Y, int epi, const float* gate, int HW,
                    const _Float16* res, float* gap_out, hipStream_t st)
{
    GemmArgs a{};
    a.X = X; a.M = M; a.K = L.K; a.Wp = L.w; a.Kp = L.Kp; a.bias = L.b; a.Y = Y; a.N = L.N;
    a.nt = L.nt; a.n_chunks = L.n_chunks; a.epi = epi; a.gate = gate; a.HW = HW; a.res = res;
    a.gap_out = gap_out; a.inv_hw = (float)(1.0 / ((double)HW * LOG2E));  // GAP input is log2(e)-scaled
    a.mt = gemm_mt(L, M);
    a.defer_gate = gemm_defer_gate(gate != nullptr, HW);
    return launch_pw_gemm(a, st);
}

static int forward_lane(mmc_backbone* bb, mmc_backbone::Lane& ws, const uint8_t* patches_dev, int n, float* out_dev,
                        hipStream_t st, Prof* prof)
{
#define STEP(nm, label, expr)                                                           \
    do {                                                                                \
        ProfEntry pe_;                                                                  \
        if (prof) {                                                                     \
            pe_.name = std::string(nm) + "|" + std::string(label);                     \
            HIP_TRY(hipEventCreate(&pe_.e0));                                           \
            HIP_TRY(hipEventCreate(&pe_.e1));                                           \
            HIP_TRY(hipEventRecord(pe_.e0, st));                                        \
        }                                                                               \
        KTRY(expr);                                                                     \
        if (prof) {                                                                     \
            HIP_TRY(hipEventRecord(pe_.e1, st));                                        \
            prof->entries.push_back(pe_);                                               \
        }                                                                               \
    } while (0)
    // per-tensor mode (MMC_KEEP_ACTIVATIONS=1): copy a tensor out under its name
#define SAVE(name, dev, elems, is_half)                                                                  \
    do {                                                                                                 \
        if (bb->keep) { int r_ = save_act(bb, name, dev, elems, is_half, st); if (r_) return r_; }      \
    } while (0)
    char nm[64];
    _Float16* x = ws.act0;
    _Float16* y = ws.act1;
    auto swap_xy = [&] { _Float16* t = x; x = y; y = t; };
    const int lane_idx = (int)(&ws - bb->lanes);
    // The chained launch: its members' arguments are collected in launch order and go out with the last one.  Its workgroups are
    // NOT in step: while workgroup b writes a phase's output, another may still be reading an earlier phase's input.  A buffer's
    // patch b starts at b x (pixels x row width), so two tensors of different row width in one buffer overlap ACROSS patches --
    // between separate launches that is harmless, inside the chain it is a race.  So a chained tensor whose row width differs from
    // what its buffer holds when the chain starts (block ch0's widths) lives in the buffer's upper part, beyond lane_cap patches of
    // the widest tensor: every region then holds ONE row width, and a workgroup only ever touches its own patch's rows of it.
    Chain14Args ca{};
    const int ch0 = bb->chain_first, ch1 = bb->chain_last;
    const size_t ch_hw = ch0 >= 0 ? (size_t)bb->blk[ch0].Ho * bb->blk[ch0].Ho : 0;
    auto ch_act = [&](_Float16* base, int cout) { return base + (cout == bb->blk[ch0].d.cout ? 0 : (size_t)bb->lane_cap * ch_hw * bb->chain_cout); };
    auto ch_dw = [&](int ce) { return ws.dwbuf + (ce == bb->blk[ch0].ce ? 0 : (size_t)bb->lane_cap * ch_hw * bb->chain_ce); };
    auto ch_pool = [&](int ce) { return ws.pool_part + (ce == bb->blk[ch0].ce ? 0 : (size_t)bb->lane_cap * bb->chain_ce); };
    _Float16 *xbase = nullptr, *ybase = nullptr;   // inside the chain: the buffers x and the next output live in
    if (!bb->fuse_stem) {   // (fused: the stem tensor never exists in HBM, no "stem" activation to keep)
        STEP("stem", "stem_conv", launch_stem(patches_dev, bb->stem_w, bb->stem_b, bb->stem_pad, x, n, bb->stem_ch, st));
        SAVE("stem", x, (size_t)n * 112 * 112 * bb->stem_ch, true);
    }
    for (int i = 0; i < bb->nblk; ++i) {
        BlockW& B = bb->blk[i];
        if (B.front == Front::Tail) break;
        const int HWi = B.H * B.H, HWo = B.Ho * B.Ho;
        snprintf(nm, sizeof nm, "b%d.mbconv", i);
        switch (B.front) {
        case Front::StemDw:
            // with block 0's project folded into block 1's kernel the depthwise output goes to the spare activation
            // buffer (block 1 reads it while writing its own depthwise output to dwbuf)
            STEP("stem+b0.dw", "stem_dw", launch_stem_dw(patches_dev, bb->stem_w, bb->stem_b, bb->stem_pad, B.dw_w, B.dw_b,
                                                          bb->fuse_b0b1 ? y : ws.dwbuf, ws.pool_part, n, st));
            break;
        case Front::Mbt: {
            MbtArgs ta{};
            ta.X = x; ta.wexp = B.exp_frag; ta.bexp = B.expand.b; ta.dwp = B.t_dwp; ta.bdw = B.dw_b; ta.D = ws.dwbuf;
            ta.pool = ws.pool_part; ta.B = n; ta.H = B.H; ta.Cin = B.d.cin; ta.Ce = B.ce; ta.ks = B.d.k; ta.stride = B.d.s;
            ta.dwtoe = B.mbt4 ? B.dw_diag : nullptr;
            STEP(nm, B.front_label, launch_mbt(ta, st));
            break;
        }
        case Front::Mid14: {
            Mid14Args ma{};
            ma.X = x; ma.wexp = B.exp_frag; ma.bexp = B.expand.b; ma.dwp = B.t_dwp4; ma.bdw = B.dw_b; ma.D = ws.dwbuf;
            ma.pool = ws.pool_part; ma.B = n; ma.Cin = B.d.cin; ma.Ce = B.ce; ma.ks = B.d.k;
            ma.dwdiag = B.mid14m ? B.dw_diag : nullptr;
            ma.nsplit = B.mid14m ? 1 : 4;
            if (bb->mid_clk && i == 10) ma.dbg_clk = bb->mid_clk + (size_t)lane_idx * bb->lane_cap * 128;
            if (ch0 >= 0 && i > ch0 && i <= ch1) {
                ma.D = ch_dw(B.ce);
                ma.pool = ch_pool(B.ce);
                Chain14Phase& ph = ca.ph[ca.nph++];
                ph.kind = chain14_mid_kind(ma.Cin, ma.ks, ma.Ce);
                ph.mid = ma;
                break;
            }
            STEP(nm, B.front_label, launch_mid14(ma, st));
            break;
        }
        case Front::Mb1: {
            Mb1Args m1{};
            m1.X = y; m1.pre_w = bb->b0_pre_w; m1.pre_b = bb->blk[0].project.b; m1.pre_gate = ws.gate; m1.wexp = bb->b1_exp_pre;
            m1.bexp = B.expand.b; m1.wdw = B.dw_w; m1.bdw = B.dw_b; m1.D = ws.dwbuf; m1.pool = ws.pool_part; m1.B = n;
            m1.planar = B.planar ? 1 : 0;
            STEP("b0.project+b1.mbconv", "mb1", launch_mb1(m1, st));
            break;
        }
        case Front::MbPre: case Front::MbD: case Front::MbA: {
            MbArgs a = B.mb;
            a.X = x; a.Wexp = B.exp_nat; a.bexp = B.expand.b; a.Wdw = B.dw_w; a.bdw = B.dw_b; a.out = ws.dwbuf;
            a.pool_part = ws.pool_part; a.B = n;
            if (B.front == Front::MbD) {
                STEP(nm, B.front_label, launch_mbconv_d(a, st));
            } else if (B.front == Front::MbPre) {
                a.X = y; a.Cin = 32; a.Wexp = bb->b1_exp_pre;   // block 0's depthwise output; its gate is in ws.gate
                STEP("b0.project+b1.mbconv", B.front_label, launch_mbconv_pre(a, bb->b0_pre_w, bb->blk[0].project.b, ws.gate, st));
            } else {
                STEP(nm, B.front_label, launch_mbconv_a(a, st));
            }
            break;
        }
        default: {   // Front::Unfused
            const _Float16* dw_in = x;
            if (B.has_expand) {
                snprintf(nm, sizeof nm, "b%d.expand", i);
                STEP(nm, B.expand.label[gemm_mt(B.expand, n * HWi) - 1],
                     run_gemm(B.expand, x, n * HWi, ws.expbuf, EPI_SILU, nullptr, HWi, nullptr, nullptr, st));
                SAVE(nm, ws.expbuf, (size_t)n * HWi * B.ce, true);
                dw_in = ws.expbuf;
            }
            DwArgs d{};
            d.in = dw_in; d.wt = B.dw_w; d.bias = B.dw_b; d.out = ws.dwbuf; d.pool_part = ws.pool_part;
            d.B = n; d.H = B.H; d.W = B.H; d.C = B.ce; d.Ho = B.Ho; d.Wo = B.Ho; d.pad_t = B.pad; d.pad_l = B.pad;
            d.ks = B.d.k; d.stride = B.d.s; d.tw = B.tw; d.CG = B.CG; d.S = B.S; d.iters = B.iters; d.parts = B.parts; d.nz = B.nz;
            snprintf(nm, sizeof nm, "b%d.dw", i);
            STEP(nm, B.front_label, launch_dwconv(d, st));
        }
        }
        snprintf(nm, sizeof nm, "b%d.dw", i);
        SAVE(nm, (i == 0 && bb->fuse_b0b1) ? y : ws.dwbuf, (size_t)n * HWo * B.ce, true);
        if (B.back == Back::Tail) break;   // block 11's back half: the tail launch below
        if (B.back == Back::ProjPatch) {
            // squeeze-excite + project, one patch per workgroup (proj_patch_kernel): no gate tensor, one launch
            ProjPatchArgs pa{};
            pa.X = ws.dwbuf; pa.pool_part = ws.pool_part; pa.wr_g = B.t_wrg; pa.br = B.pp_br; pa.we_t = B.t_we; pa.be = B.se_be;
            pa.wfrag = B.pp_w; pa.bias = B.pp_b; pa.res = B.skip ? x : nullptr; pa.Y = y;
            pa.dbg_gate = bb->keep ? ws.gate : nullptr;
            pa.dbg_clk = bb->keep ? bb->dbg_clk : nullptr;
            pa.B = n; pa.HW = HWo; pa.K = B.ce; pa.N = B.d.cout; pa.CSP = B.cs4; pa.nparts = B.nparts;
            pa.psc = (float)(1.0 / ((double)HWo * LOG2E));
            if (ch0 >= 0 && i >= ch0 && i <= ch1) {
                if (i == ch0) { xbase = x; ybase = y; }
                pa.X = ch_dw(B.ce);
                pa.pool_part = ch_pool(B.ce);
                pa.Y = ch_act(ybase, B.d.cout);
                Chain14Phase& ph = ca.ph[ca.nph++];
                ph.kind = chain14_proj_kind(pa.K, pa.N, pa.HW, pa.res ? 1 : 0);
                ph.pp = pa;
                x = pa.Y;
                std::swap(xbase, ybase);
                y = ybase;   // (after the chain: the other buffer, whose tensors are dead by then)
                if (i == ch1) {
                    ca.B = n;
                    snprintf(nm, sizeof nm, "b%d.projse-b%d.projse.chain", ch0, ch1);
                    STEP(nm, "chain14", launch_chain14(ca, st));
                }
                continue;
            }
            snprintf(nm, sizeof nm, "b%d.projse", i);
            STEP(nm, B.back_label, launch_proj_patch(pa, st));
            snprintf(nm, sizeof nm, "b%d.gate", i);
            SAVE(nm, ws.gate, (size_t)n * B.ce, false);
            snprintf(nm, sizeof nm, "b%d.out", i);
            SAVE(nm, y, (size_t)n * HWo * B.d.cout, true);
            snprintf(nm, sizeof nm, "b%d.clk", i);
            SAVE(nm, bb->dbg_clk, (size_t)n * 8, false);
            swap_xy();
            continue;
        }
        snprintf(nm, sizeof nm, "b%d.gate", i);
        if (B.se == Se::Wide)
            STEP(nm, "se_wide", launch_se_wide(ws.pool_part, B.nparts, n, B.ce, B.cs, B.se_wr_nat, B.se_br_nat, B.se_we_nat, B.se_be,
                                               ws.gate, st));
        else if (B.se == Se::Small)
            STEP(nm, "se_small", launch_se_small(ws.pool_part, B.nparts, n, B.ce, B.cs, B.se_wr_nat, B.se_br_nat, B.se_we_nat, B.se_be,
                                                 ws.gate, st));
        else
            STEP(nm, "se_fused", launch_se_gate(ws.pool_part, B.nparts, n, B.ce, B.cs4, B.se_wrp, B.se_br, B.se_wep, B.se_be,
                                                ws.gate, st));
        SAVE(nm, ws.gate, (size_t)n * B.ce, false);
        if (B.back == Back::SeFolded) continue;   // block 0's project runs inside block 1's kernel
        snprintf(nm, sizeof nm, "b%d.project", i);
        if (B.proj == Proj::Thin) {
            // small-K, small-N project on a big image (B4 blocks 0, 1; B0 block 1): stream one patch's fragments per workgroup
            GemmArgs a{};
            a.X = ws.dwbuf; a.M = n * HWo; a.K = B.project.K; a.Wp = B.project.w; a.Kp = B.project.Kp; a.bias = B.project.b; a.Y = y;
            a.N = B.project.N; a.nt = B.project.nt; a.n_chunks = B.project.n_chunks; a.epi = EPI_LINEAR; a.gate = ws.gate; a.HW = HWo;
            a.res = B.skip ? x : nullptr;
            a.x_plane_rows = B.planar ? n * HWo : 0;
            STEP(nm, "thin_proj", launch_thin_proj(a, n, st));
        } else if (B.proj == Proj::Fp8) {
            Fp8GemmArgs fa{};
            fa.X = ws.dwbuf; fa.M = n * HWo; fa.K = B.p8.K; fa.W8 = B.p8.w8; fa.KS128 = B.p8.KS128; fa.NFp = B.p8.NFp; fa.sw = B.p8.sw;
            fa.bias = B.p8.b; fa.Y = y; fa.N = B.p8.N; fa.gate = ws.gate; fa.HW = HWo; fa.res = B.skip ? x : nullptr;
            STEP(nm, "pw_gemm_fp8", launch_pw_gemm_fp8(fa, st));
        } else
            STEP(nm, B.project.label[gemm_mt(B.project, n * HWo) - 1],
                 run_gemm(B.project, ws.dwbuf, n * HWo, y, EPI_LINEAR, ws.gate, HWo, B.skip ? x : nullptr, nullptr, st));
        snprintf(nm, sizeof nm, "b%d.out", i);
        SAVE(nm, y, (size_t)n * HWo * B.d.cout, true);
        swap_xy();
    }
    // ---- the tail and the head ----
    const float inv_hw7 = (float)(1.0 / (49.0 * LOG2E));
    if (bb->tail == TailRoute::B11All || (bb->tail == TailRoute::B11 && !bb->keep)) {
        // from block 11's input (B11All) or its depthwise output (B11) through blocks 12..15 and the head conv to the features, ONE launch
        const BlockW& B11 = bb->blk[11];
        TailArgs ta{};
        ta.B = n; ta.blk = bb->tail_tab; ta.nblk = 4;
        if (bb->tail == TailRoute::B11All) {
            ta.pre_X = x; ta.pre_wexp = B11.exp_frag; ta.pre_bexp = B11.expand.b; ta.pre_dwp = B11.t_dwp4; ta.pre_bdw = B11.dw_b;
        } else {
            ta.pre_D = ws.dwbuf; ta.pre_pool = ws.pool_part;
        }
        ta.pre_wr_t = B11.t_wr; ta.pre_br = B11.pp_br; ta.pre_we_t = B11.t_we; ta.pre_be = B11.se_be; ta.pre_wproj = bb->pre_wproj;
        ta.pre_bproj = B11.project.b; ta.inv_hw = inv_hw7;
        ta.head_w = bb->head_wfrag; ta.head_b = bb->head.b; ta.feat = out_dev;
        if (bb->tail == TailRoute::B11All && bb->tail_clk) {   // debug clock: rows of this lane's patches
            ta.dbg_clk = bb->tail_clk + (size_t)lane_idx * bb->lane_cap * 64; ta.clk_sections = 1;
        }
        STEP(bb->tail == TailRoute::B11All ? "b11all-head.tail" : "b11-head.tail", "tail7", launch_tail7(ta, st));
        return 0;
    }
    if (bb->tail == TailRoute::B11) {   // per-tensor mode: block 11's back half on its own
        const BlockW& B11 = bb->blk[11];
        TailArgs ta{};
        ta.B = n; ta.blk = bb->tail_tab; ta.nblk = 0; ta.Y = y; ta.dbg_gate = ws.gate;
        ta.pre_D = ws.dwbuf; ta.pre_pool = ws.pool_part; ta.pre_wr_t = B11.t_wr; ta.pre_br = B11.pp_br; ta.pre_we_t = B11.t_we;
        ta.pre_be = B11.se_be; ta.pre_wproj = bb->pre_wproj; ta.pre_bproj = B11.project.b; ta.inv_hw = inv_hw7;
        STEP("b11.tail", "tail7", launch_tail7(ta, st));
        SAVE("b11.gate", ws.gate, (size_t)n * B11.ce, false);
        SAVE("b11.out", y, (size_t)n * 49 * 192, true);
        swap_xy();
    }
    if (bb->tail != TailRoute::None && !bb->keep) {
        // blocks 12..15 in one launch, one patch per workgroup, tensors resident in LDS (tail7_kernel)
        TailArgs ta{};
        ta.X = x; ta.Y = y; ta.B = n; ta.nblk = 4; ta.blk = bb->tail_tab;
        STEP("b12-15.tail", "tail7", launch_tail7(ta, st));
        swap_xy();
    } else if (bb->tail != TailRoute::None) {
        for (int j = 0; j < 4; ++j) {   // block at a time so every intermediate tensor can be read back
            const BlockW& B = bb->blk[12 + j];
            TailArgs ta{};
            ta.X = x; ta.Y = y; ta.B = n; ta.nblk = 1; ta.blk = bb->tail_tab + j;
            ta.dbg_dw = ws.dwbuf; ta.dbg_gate = ws.gate; ta.dbg_clk = ws.pool_part;
            snprintf(nm, sizeof nm, "b%d.tail", 12 + j);
            STEP(nm, "tail7", launch_tail7(ta, st));
            snprintf(nm, sizeof nm, "b%d.dw", 12 + j);
            SAVE(nm, ws.dwbuf, (size_t)n * 49 * B.ce, true);
            snprintf(nm, sizeof nm, "b%d.gate", 12 + j);
            SAVE(nm, ws.gate, (size_t)n * B.ce, false);
            snprintf(nm, sizeof nm, "b%d.out", 12 + j);
            SAVE(nm, y, (size_t)n * 49 * B.d.cout, true);
            snprintf(nm, sizeof nm, "b%d.clk", 12 + j);
            SAVE(nm, ws.pool_part, (size_t)n * 8, false);
            swap_xy();
        }
    }
    if (bb->tail == TailRoute::B11) {   // per-tensor mode: the head phase of tail7_kernel on its own
        TailArgs ta{};
        ta.X = x; ta.B = n; ta.nblk = 0; ta.blk = bb->tail_tab; ta.in_wide = 1;
        ta.head_w = bb->head_wfrag; ta.head_b = bb->head.b; ta.feat = out_dev; ta.inv_hw = inv_hw7;
        STEP("head.tail", "tail7", launch_tail7(ta, st));
    } else {
        const int HWh = bb->blk[bb->nblk - 1].Ho * bb->blk[bb->nblk - 1].Ho;
        STEP("head", bb->head.label[0],
             run_gemm(bb->head, x, n * HWh, nullptr, EPI_GAP, nullptr, HWh, nullptr, out_dev, st));
    }
#undef SAVE
#undef STEP
    return 0;
}

// One pass over n resident patches: split into lanes, fork from / join to the caller's stream ONCE.  n may exceed
// max_batch: the pass is then a sequence of max_batch-sized chunks, and each lane walks its sub-batch of every chunk on its
// own stream without waiting for the other lanes -- the drain of one chunk (the last lane's per-patch kernels, which fill
// half the chip) overlaps the first kernels of the next chunk.  Sub-batch shapes are those of separate calls, so results are
// bitwise the same.
static int forward_pass(mmc_backbone* bb, const uint8_t* patches_dev, int n, float* out_dev, hipStream_t st, Prof* prof)
{
    // Profiling records HIP events on each lane's own stream, i.e. durations as they are with the lanes running
    // concurrently (what rocprofv3 sees); MMC_PROFILE_SERIAL=1 profiles one lane at a time instead (isolated kernels).
    const size_t psz = (size_t)IMG * IMG * 3, FEAT = (size_t)bb->feat;
    if (bb->nlanes == 1 || (prof && bb->opt.profile_serial) || n < 2 * bb->nlanes) {
        for (int off = 0; off < n; off += bb->lane_cap) {
            const int cur = n - off < bb->lane_cap ? n - off : bb->lane_cap;
            int r = forward_lane(bb, bb->lanes[0], patches_dev + (size_t)off * psz, cur, out_dev + (size_t)off * FEAT, st, prof);
            if (r) return r;
        }
        return 0;
    }
    HIP_TRY(hipEventRecord(bb->fork, st));
    for (int l = 0; l < bb->nlanes; ++l) HIP_TRY(hipStreamWaitEvent(bb->lanes[l].stream, bb->fork, 0));
    for (int base = 0; base < n; base += bb->max_batch) {          // chunk-major enqueue: the lanes' launches interleave on the host
        const int cn = n - base < bb->max_batch ? n - base : bb->max_batch;
        const int per = (cn + bb->nlanes - 1) / bb->nlanes;
        for (int l = 0; l < bb->nlanes; ++l) {
            const int off = l * per;
            const int cur = cn - off < per ? cn - off : per;
            if (cur <= 0) break;
            mmc_backbone::Lane& L = bb->lanes[l];
            int r = forward_lane(bb, L, patches_dev + (size_t)(base + off) * psz, cur, out_dev + (size_t)(base + off) * FEAT, L.stream, prof);
            if (r) return r;
        }
    }
    for (int l = 0; l < bb->nlanes; ++l) {
        mmc_backbone::Lane& L = bb->lanes[l];
        HIP_TRY(hipEventRecord(L.done, L.stream));
        HIP_TRY(hipStreamWaitEvent(st, L.done, 0));
    }
    return 0;
}

// forward_pass through a cached HIP graph (device-resident buffers only); falls back to plain launches on any error
static int run_pass(mmc_backbone* bb, const uint8_t* pin, int n, float* pout, hipStream_t st)
{
    if (!bb->use_graph || n > 8 * bb->max_batch) return forward_pass(bb, pin, n, pout, st, nullptr);   // (bounded graph size)
    for (size_t gi = 0; gi < bb->graphs.size(); ++gi) {
        const mmc_backbone::GraphEntry g = bb->graphs[gi];
        if (g.in == pin && g.out == pout && g.n == n) {
            if (gi + 1 != bb->graphs.size()) {   // most recently used last
                bb->graphs.erase(bb->graphs.begin() + (long)gi);
                bb->graphs.push_back(g);
            }
            HIP_TRY(hipGraphLaunch(g.exec, st));
            return 0;
        }
    }
    if (bb->evictions >= MMC_GRAPH_CACHE) return forward_pass(bb, pin, n, pout, st, nullptr);   // cache frozen: see `evicted`
    for (auto& k : bb->evicted)
        if (k.in == pin && k.out == pout && k.n == n) return forward_pass(bb, pin, n, pout, st, nullptr);
    bool repeat = false;
    for (auto& k : bb->seen) repeat = repeat || (k.in == pin && k.out == pout && k.n == n);
    if (!repeat) {
        if (bb->seen.size() >= 2 * MMC_GRAPH_CACHE) bb->seen.erase(bb->seen.begin());
        bb->seen.push_back({pin, pout, n});
    }
    if (bb->graph_warm < 2 || !repeat) {   // first passes un-captured: lazy per-kernel attribute setup happens there
        ++bb->graph_warm;
        return forward_pass(bb, pin, n, pout, st, nullptr);
    }
    if (!bb->gstream && hipStreamCreateWithFlags(&bb->gstream, hipStreamNonBlocking) != hipSuccess) {
        bb->use_graph = false;
        return forward_pass(bb, pin, n, pout, st, nullptr);
    }
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    bool ok = hipStreamBeginCapture(bb->gstream, hipStreamCaptureModeRelaxed) == hipSuccess;
    int r = ok ? forward_pass(bb, pin, n, pout, bb->gstream, nullptr) : 0;
    if (ok) ok = hipStreamEndCapture(bb->gstream, &graph) == hipSuccess && r == 0 && graph;
    if (ok) ok = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if (graph) hipGraphDestroy(graph);
    if (!ok) {
        (void)hipGetLastError();
        bb->use_graph = false;
        return forward_pass(bb, pin, n, pout, st, nullptr);
    }
    if (bb->graphs.size() >= MMC_GRAPH_CACHE) {
        // least recently used graph goes; it may still be executing on a stream this handle was given earlier: passes of a
        // handle are serialised (PassOrder), so waiting for the last pass's completion event covers every earlier replay
        if (bb->have_last && hipEventSynchronize(bb->last_done) != hipSuccess) {
            (void)hipGetLastError();
            hipGraphExecDestroy(exec);
            return forward_pass(bb, pin, n, pout, st, nullptr);
        }
        const mmc_backbone::GraphEntry old = bb->graphs.front();
        hipGraphExecDestroy(old.exec);
        bb->graphs.erase(bb->graphs.begin());
        if (bb->evicted.size() >= 8 * MMC_GRAPH_CACHE) bb->evicted.erase(bb->evicted.begin());
        bb->evicted.push_back({old.in, old.out, old.n});
        ++bb->evictions;
    }
    bb->graphs.push_back({pin, pout, n, exec});
    ++bb->captures;
    HIP_TRY(hipGraphLaunch(exec, st));
    return 0;
}

extern "C" int mmc_backbone_graph_stats(mmc_backbone* bb, int64_t stats[3])
{
    if (!bb || !stats) return fail(MMC_ERR_ARG, "backbone handle / stats is NULL");
    std::lock_guard<std::mutex> lock(bb->mu);
    stats[0] = bb->captures; stats[1] = bb->evictions; stats[2] = (int64_t)bb->graphs.size();
    return MMC_OK;
}

extern "C" int mmc_backbone_extract(mmc_backbone* bb, const void* patches, int64_t n, float* out_features,
                                    unsigned flags, void* hip_stream)
{
    if (!bb) return fail(MMC_ERR_ARG, "backbone handle is NULL");
    if (n < 0) return fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    if (n == 0) return MMC_OK;
    if (!patches || !out_features) return fail(MMC_ERR_ARG, "patches/out_features is NULL");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(bb->mu);
    HIP_TRY(hipSetDevice(bb->device));
    PassOrder order{bb, st};
    { int r = order.begin(); if (r) return r; }
    const size_t psz = (size_t)IMG * IMG * 3;
    const uint8_t* in = static_cast<const uint8_t*>(patches);
    if (!(flags & (MMC_IN_HOST | MMC_OUT_HOST)) && !bb->keep) {
        // device-resident buffers: the whole call is one pass (pipelined over max_batch-sized chunks when n is larger)
        for (int64_t off = 0; off < n; off += (1 << 20)) {
            const int cur = (int)((n - off) < (1 << 20) ? (n - off) : (1 << 20));
            int r = run_pass(bb, in + (size_t)off * psz, cur, out_features + (size_t)off * bb->feat, st);
            if (r) return r;
        }
        return MMC_OK;
    }
    for (int64_t off = 0; off < n; off += bb->max_batch) {
        const int cur = (int)((n - off) < bb->max_batch ? (n - off) : bb->max_batch);
        const uint8_t* pin = in + (size_t)off * psz;
        if (flags & MMC_IN_HOST) {
            HIP_TRY(hipMemcpyAsync(bb->in_stage, pin, (size_t)cur * psz, hipMemcpyHostToDevice, st));
            pin = bb->in_stage;
        }
        const size_t FEAT = (size_t)bb->feat;
        float* pout = (flags & MMC_OUT_HOST) ? bb->out_stage : out_features + (size_t)off * FEAT;
        int r = run_pass(bb, pin, cur, pout, st);   // (host buffers go through the fixed staging buffers: same graph every call)
        if (r) return r;
        if (flags & MMC_OUT_HOST)
            HIP_TRY(hipMemcpyAsync(out_features + (size_t)off * FEAT, bb->out_stage, (size_t)cur * FEAT * sizeof(float),
                                   hipMemcpyDeviceToHost, st));
    }
    if (flags & MMC_OUT_HOST) HIP_TRY(hipStreamSynchronize(st));
    return MMC_OK;
}

extern "C" int mmc_backbone_read_activation(mmc_backbone* bb, const char* name, float* out, size_t capacity,
                                            size_t* n_written)
{
    if (!bb || !name || !out) return fail(MMC_ERR_ARG, "NULL argument");
    if (bb->mid_clk && strcmp(name, "mid14.clk") == 0) {
        const size_t ne = (size_t)bb->max_batch * 128;
        if (ne > capacity) return fail(MMC_ERR_ARG, "'mid14.clk' has %zu elements, capacity %zu", ne, capacity);
        HIP_TRY(hipSetDevice(bb->device));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, bb->mid_clk, ne * 4, hipMemcpyDeviceToHost));
        if (n_written) *n_written = ne;
        return MMC_OK;
    }
    if (bb->tail_clk && strcmp(name, "tail.clk") == 0) {   // MMC_TAIL_CLK=1: phase clock of the last production pass
        const size_t ne = (size_t)bb->max_batch * 64;
        if (ne > capacity) return fail(MMC_ERR_ARG, "'tail.clk' has %zu elements, capacity %zu", ne, capacity);
        HIP_TRY(hipSetDevice(bb->device));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, bb->tail_clk, ne * 4, hipMemcpyDeviceToHost));
        if (n_written) *n_written = ne;
        return MMC_OK;
    }
    if (!bb->keep) return fail(MMC_ERR_ARG, "activations are not kept: set MMC_KEEP_ACTIVATIONS=1 before create");
    auto it = bb->saved.find(name);
    if (it == bb->saved.end()) return fail(MMC_ERR_ARG, "no saved activation named '%s'", name);
    const Saved& s = it->second;
    if (s.elems > capacity) return fail(MMC_ERR_ARG, "'%s' has %zu elements, capacity %zu", name, s.elems, capacity);
    HIP_TRY(hipSetDevice(bb->device));
    HIP_TRY(hipDeviceSynchronize());
    if (s.is_half) {
        std::vector<_Float16> tmp(s.elems);
        HIP_TRY(hipMemcpy(tmp.data(), s.dev, s.elems * 2, hipMemcpyDeviceToHost));
        const size_t ln = strlen(name);
        const bool scaled = strcmp(name, "stem") == 0 || (ln > 3 && strcmp(name + ln - 3, ".dw") == 0) ||
                            (ln > 7 && strcmp(name + ln - 7, ".expand") == 0);   // SiLU outputs live times log2(e)
        const float inv = scaled ? (float)(1.0 / LOG2E) : 1.0f;
        for (size_t i = 0; i < s.elems; ++i) out[i] = (float)tmp[i] * inv;
    } else {
        HIP_TRY(hipMemcpy(out, s.dev, s.elems * 4, hipMemcpyDeviceToHost));
    }
    if (n_written) *n_written = s.elems;
    return MMC_OK;
}

extern "C" int mmc_backbone_profile(mmc_backbone* bb, const void* patches_dev, int64_t n, float* out_features_dev,
                                    void* hip_stream, char (*names)[64], float* ms, int* launches, int cap, int* n_out)
{
    if (!bb || !patches_dev || !out_features_dev || !names || !ms || !n_out)
        return fail(MMC_ERR_ARG, "NULL argument");
    if (n < 1 || n > bb->max_batch) return fail(MMC_ERR_ARG, "n must be in [1, max_batch]");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(bb->mu);
    HIP_TRY(hipSetDevice(bb->device));
    PassOrder order{bb, st};
    { int r = order.begin(); if (r) return r; }
    Prof prof;
    int r = forward_pass(bb, static_cast<const uint8_t*>(patches_dev), (int)n, out_features_dev, st, &prof);
    if (r) return r;
    HIP_TRY(hipStreamSynchronize(st));
    int cnt = 0;
    for (auto& e : prof.entries) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, e.e0, e.e1));
        hipEventDestroy(e.e0);
        hipEventDestroy(e.e1);
        if (cnt < cap) {
            snprintf(names[cnt], 64, "%s", e.name.c_str());
            ms[cnt] = t;
            if (launches) launches[cnt] = 1;
            ++cnt;
        }
    }
    *n_out = cnt;
    return MMC_OK;
}

// ------------------------------------------------------------------------------------------
// crop front-end
// ------------------------------------------------------------------------------------------
// Host-side cut for sparse points: pinned ring of 4 slots; a slot is reused only after the H2D copy that read it has
// completed (event), so calls stay asynchronous on the caller's stream.  One thread at a time per process (mutex).
namespace {
struct PinnedSlot { void* host = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool busy = false; };
PinnedSlot g_slots[4];
int g_slot_next = 0;
std::mutex g_slot_mu;
// upload path of mmc_crop_patches (dense points on a host image): per-device staging buffers kept between calls
// (rc holds the points and, behind them, the view codes of mmc_crop_patches_views)
struct CropStage { void* img = nullptr; size_t img_cap = 0; void* rc = nullptr; size_t rc_cap = 0; hipEvent_t ev = nullptr; };
CropStage g_crop_stage[16];
}  // namespace

// views: one code per point (checked by the caller) or NULL = all 0; view 0 is the row-memcpy cut, every other view goes pixel by
// pixel through view_source(), the mapping the kernel uses
static int crop_on_host(const uint8_t* img, int H, int W, const int32_t* rowcols, const uint8_t* views, int64_t n, void* out_dev,
                        hipStream_t st)
{
    std::lock_guard<std::mutex> lock(g_slot_mu);
    PinnedSlot& s = g_slots[g_slot_next];
    g_slot_next = (g_slot_next + 1) & 3;
    const size_t psz = (size_t)IMG * IMG * 3, need = (size_t)n * psz;
    if (s.busy) { HIP_TRY(hipEventSynchronize(s.ev)); s.busy = false; }
    if (!s.ev) HIP_TRY(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    if (s.cap < need) {
        if (s.host) hipHostFree(s.host);
        s.host = nullptr; s.cap = 0;
        HIP_TRY(hipHostMalloc(&s.host, need, hipHostMallocDefault));
        s.cap = need;
    }
    auto refl = [](int i, int nn) { i = i < 0 ? -i : i; return i >= nn ? 2 * (nn - 1) - i : i; };   // numpy 'reflect'
    uint8_t* dst = static_cast<uint8_t*>(s.host);
    auto cut = [&](int64_t p0, int64_t p1) {
        for (int64_t p = p0; p < p1; ++p) {
            const int row = rowcols[2 * p], col = rowcols[2 * p + 1];
            const int v = views ? views[p] : 0;
            if (v != 0) {
                uint8_t* d = dst + (size_t)p * psz;
                for (int i = 0; i < IMG; ++i)
                    for (int j = 0; j < IMG; ++j, d += 3) {
                        int by, bx;
                        view_source(v, i, j, by, bx);
                        if (!(v & 8)) {
                            const uint8_t* src = img + ((size_t)refl(row - IMG / 2 + by, H) * W + refl(col - IMG / 2 + bx, W)) * 3;
                            d[0] = src[0]; d[1] = src[1]; d[2] = src[2];
                        } else {   // the 2x2 footprint in the 448-pixel window, rounded mean
                            const size_t y0 = (size_t)refl(row - IMG + 2 * by, H) * W, y1 = (size_t)refl(row - IMG + 2 * by + 1, H) * W;
                            const int x0 = refl(col - IMG + 2 * bx, W), x1 = refl(col - IMG + 2 * bx + 1, W);
                            for (int c = 0; c < 3; ++c)
                                d[c] = (uint8_t)((img[(y0 + x0) * 3 + c] + img[(y0 + x1) * 3 + c] + img[(y1 + x0) * 3 + c] +
                                                  img[(y1 + x1) * 3 + c] + 2) >> 2);
                        }
                    }
                continue;
            }
            const int sx0 = col - IMG / 2;
            const bool inside = sx0 >= 0 && sx0 + IMG <= W;
            for (int y = 0; y < IMG; ++y) {
                const int sy = refl(row - IMG / 2 + y, H);
                uint8_t* d = dst + (size_t)p * psz + (size_t)y * IMG * 3;
                if (inside) {
                    memcpy(d, img + ((size_t)sy * W + sx0) * 3, (size_t)IMG * 3);
                } else {
                    for (int x = 0; x < IMG; ++x) {
                        const uint8_t* src = img + ((size_t)sy * W + refl(sx0 + x, W)) * 3;
                        d[3 * x] = src[0]; d[3 * x + 1] = src[1]; d[3 * x + 2] = src[2];
                    }
                }
            }
        }
    };
    static const int max_threads = [] { const char* e = getenv("MMC_CROP_THREADS"); const int v = e ? atoi(e) : 4; return v < 1 ? 1 : (v > 4 ? 4 : v); }();
    const int nthreads = n >= 8 ? max_threads : 1;   // the cut is memcpy-bound: a few threads saturate what one core cannot
    if (nthreads == 1) cut(0, n);
    else {
        std::thread th[3];
        const int64_t per = (n + nthreads - 1) / nthreads;
        for (int t = 1; t < nthreads; ++t) th[t - 1] = std::thread(cut, t * per < n ? t * per : n, (t + 1) * per < n ? (t + 1) * per : n);
        cut(0, per < n ? per : n);
        for (int t = 1; t < nthreads; ++t) th[t - 1].join();
    }
    HIP_TRY(hipMemcpyAsync(out_dev, s.host, need, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s.ev, st));
    s.busy = true;
    return MMC_OK;
}

// mmc_crop_patches (with_views false: crop_kernel and the row-memcpy cut, as ever) and mmc_crop_patches_views (views may be NULL)
static int crop_patches(const void* image, int height, int width, const int32_t* rowcols, int64_t n, bool with_views,
                        const uint8_t* views, void* patches_out_dev, unsigned flags, int device, void* hip_stream)
{
    if (!image || !rowcols || !patches_out_dev) return fail(MMC_ERR_ARG, "NULL argument");
    if (n < 0 || n > 65535) return fail(MMC_ERR_ARG, "n = %lld out of range [0,65535]", (long long)n);
    if (n == 0) return MMC_OK;
    if (height <= IMG || width <= IMG)
        return fail(MMC_ERR_ARG, "image %dx%d must exceed the crop size %d in both dimensions", height, width, IMG);
    if (views && (flags & MMC_IN_HOST))   // host codes are checked (no device needed); device codes are masked by the kernel
        for (int64_t i = 0; i < n; ++i)
            if (views[i] >= VIEWS_MAX)
                return fail(MMC_ERR_ARG, "view code %d of patch %lld is outside [0, 15]", (int)views[i], (long long)i);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(device));
    const uint8_t* img = static_cast<const uint8_t*>(image);
    const int32_t* rc = rowcols;
    if (flags & MMC_IN_HOST) {
        for (int64_t i = 0; i < n; ++i) {
            const int r = rowcols[2 * i], c = rowcols[2 * i + 1];
            if (r < 0 || r >= height || c < 0 || c >= width)
                return fail(MMC_ERR_ARG, "point %lld (%d,%d) outside the %dx%d image", (long long)i, r, c, height, width);
        }
        const size_t ib = (size_t)height * width * 3;
        // Sparse points on a big host image (the reference's data: 10-25 points on a 27 MP image): uploading the image moves
        // 81 MB to cut 3.8 MB of patches.  Cut them on the host instead -- same index arithmetic, row memcpys into a pinned
        // ring slot -- and upload only the patches.  Dense points keep the upload + crop_kernel path.  MMC_CROP_HOST=0/1 forces.
        static const int force = [] { const char* e = getenv("MMC_CROP_HOST"); return e ? atoi(e) : -1; }();
        const bool host_crop = force >= 0 ? force != 0 : (size_t)n * IMG * IMG * 3 * 6 <= ib;
        if (host_crop) return crop_on_host(img, height, width, rowcols, views, n, patches_out_dev, st);
        // dense points: upload the image once into a per-device staging buffer that is kept between calls (grown on demand)
        std::lock_guard<std::mutex> lock(g_slot_mu);
        CropStage& cs = g_crop_stage[device & 15];
        const size_t rb = (size_t)n * 8 + (views ? (size_t)n : 0);
        if (cs.img_cap < ib) {
            if (cs.img) { hipStreamSynchronize(st); hipFree(cs.img); }
            cs.img = nullptr; cs.img_cap = 0;
            HIP_TRY(hipMalloc(&cs.img, ib));
            cs.img_cap = ib;
        }
        if (cs.rc_cap < rb) {
            if (cs.rc) { hipStreamSynchronize(st); hipFree(cs.rc); }
            cs.rc = nullptr; cs.rc_cap = 0;
            HIP_TRY(hipMalloc(&cs.rc, rb));
            cs.rc_cap = rb;
        }
        // the previous call's kernel may still be reading the staging buffers on another stream
        if (cs.ev) HIP_TRY(hipStreamWaitEvent(st, cs.ev, 0));
        else HIP_TRY(hipEventCreateWithFlags(&cs.ev, hipEventDisableTiming));
        HIP_TRY(hipMemcpyAsync(cs.img, image, ib, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(cs.rc, rowcols, (size_t)n * 8, hipMemcpyHostToDevice, st));
        const uint8_t* vdev = views ? static_cast<const uint8_t*>(cs.rc) + (size_t)n * 8 : nullptr;
        if (views) HIP_TRY(hipMemcpyAsync(const_cast<uint8_t*>(vdev), views, (size_t)n, hipMemcpyHostToDevice, st));
        int r = with_views ? launch_crop_views(static_cast<const uint8_t*>(cs.img), height, width, static_cast<const int32_t*>(cs.rc),
                                               vdev, (int)n, static_cast<uint8_t*>(patches_out_dev), st)
                           : launch_crop(static_cast<const uint8_t*>(cs.img), height, width, static_cast<const int32_t*>(cs.rc), (int)n,
                                         static_cast<uint8_t*>(patches_out_dev), st);
        HIP_TRY(hipEventRecord(cs.ev, st));
        // the host image / rowcols are pageable caller memory the caller may free or overwrite right after this call
        HIP_TRY(hipStreamSynchronize(st));
        if (r) return fail(MMC_ERR_HIP, "crop kernel launch failed (%d)", r);
        return MMC_OK;
    }
    // device-resident image and points: the kernel clamps each point into the image (see crop_kernel) and masks each view code
    int r = with_views ? launch_crop_views(img, height, width, rc, views, (int)n, static_cast<uint8_t*>(patches_out_dev), st)
                       : launch_crop(img, height, width, rc, (int)n, static_cast<uint8_t*>(patches_out_dev), st);
    if (r) return fail(MMC_ERR_HIP, "crop kernel launch failed (%d)", r);
    return MMC_OK;
}

extern "C" int mmc_crop_patches(const void* image, int height, int width, const int32_t* rowcols, int64_t n,
                                void* patches_out_dev, unsigned flags, int device, void* hip_stream)
{
    return crop_patches(image, height, width, rowcols, n, false, nullptr, patches_out_dev, flags, device, hip_stream);
}

extern "C" int mmc_crop_patches_views(const void* image, int height, int width, const int32_t* rowcols, int64_t n, const uint8_t* views,
                                      void* patches_out_dev, unsigned flags, int device, void* hip_stream)
{
    return crop_patches(image, height, width, rowcols, n, true, views, patches_out_dev, flags, device, hip_stream);
}
