// mmc_api.cpp -- the backbone half of the C ABI (include/mmc.h): the error buffer, the EfficientNet-B0 launch schedule and the crop.
// The calibrated head (predict, top-k, evaluate, classify) is the unit next to this one; the two share api_internal.h.
// The architecture tables, the blob reader and every weight layout are backbone_pack.h (host-only, no HIP); this unit plans, binds the
// packed images to the launch structs of kernels.h, and launches.
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
#include "backbone_pack.h"
#include "kernels.h"

static const int IMG = 224;

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

// A 1x1 convolution packed for pw_gemm_kernel
struct PwLayer {
    int N = 0, K = 0, Kp = 0, nt = 0, n_chunks = 0;
    _Float16* w = nullptr;  // device [n_chunks*16*nt][Kp]
    float* b = nullptr;     // device [n_chunks*16*nt]
    const char* label[2] = {nullptr, nullptr};   // plan: its pw_gemm instantiation with one / two row fragments per wave (gemm_mt)
};

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

// the weight half of the launch_se_gate / launch_se_small / launch_se_wide argument lists
struct SeArgs {
    int Cs = 0;   // squeeze width as that launcher takes it (launch_se_gate: padded to 4)
    const float *wr = nullptr, *br = nullptr, *we = nullptr, *be = nullptr;
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
    MbArgs mb{};            // mbconv_a / mbconv_d / mbconv_a PRE: geometry here, weights by bind_mb; all but the buffers and the batch
    // ---- plan ----
    Front front = Front::Unfused;
    Back back = Back::SeProject;
    Se se = Se::Fused;
    Proj proj = Proj::Gemm;
    bool mbt4 = false, mid14m = false;   // depthwise on 4x4x4 MFMA blocks (mbt4_kernel / mid14m_kernel)
    bool planar = false;                 // block 1: depthwise output as 32-channel planes between mb1_kernel and thin_proj_kernel
    int nparts = 0;                      // pool partials per patch left by the front half
    const char *front_label = nullptr, *back_label = nullptr;   // the templated instantiation the front half / proj_patch runs on
    // ---- weights several families read, each uploaded once ----
    PwLayer expand, project;                  // pw_gemm image + padded bias
    float *dw_w = nullptr, *dw_b = nullptr;   // tap-major fp32 taps [k*k][ce], bias [ce]
    float* se_be = nullptr;                   // excite bias [ce]
    // ---- the launch arguments of the planned kernels: weights and constant scalars, bound at create time (bind_*); build_lane
    // copies the struct into the lane's launch list and sets the buffers ----
    MbtArgs mbt{};         // Front::Mbt
    Mid14Args mid{};       // Front::Mid14
    Mb1Args mb1{};         // Front::Mb1; Front::MbPre passes its pre_w / pre_b next to `mb`
    DwArgs dw{};           // Front::Unfused
    GemmArgs exp_gemm{};   // ... its expand conv
    ProjPatchArgs pp{};    // Back::ProjPatch
    SeArgs sea{};          // Back::SeProject / SeFolded: the squeeze-excite launch `se` picks
    GemmArgs proj_gemm{};  // Back::SeProject on Proj::Thin / Proj::Gemm
    Fp8GemmArgs proj8{};   // Back::SeProject on Proj::Fp8
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
    int plane_hw = 0, plane_c = 0;   // != 0: the copy is plane_c / 32 planes of n * plane_hw rows (planes_index), read back as NHWC
};

// ------------------------------------------------------------------------------------------
// the launch list: one entry per kernel launch of a lane's pass, in stream order.  build_lane writes it once, at the end of
// create; forward_lane replays it and fills in only what depends on the call (the batch, the pass's two end pointers).
// ------------------------------------------------------------------------------------------
enum class Op { Stem, StemDw, Mbt, Mid14, Mb1, MbA, MbD, MbPre, Gemm, ThinProj, GemmFp8, Dw, SeWide, SeSmall, SeFused, ProjPatch, Chain14, Tail7 };
// the launchers without an argument struct in kernels.h: what they take besides the handle's stem weights, the batch and the stream
struct StemArgs { const float *wdw, *bdw; _Float16* out; float* pool; };   // launch_stem (out), launch_stem_dw (all four)
struct SeLaunch { const float* pool; int nparts, C; SeArgs w; float* gate; };
struct MbPreArgs { MbArgs mb; const _Float16* pre_w; const float *pre_b, *pre_gate; };
// a tensor per-tensor mode (MMC_KEEP_ACTIVATIONS=1) copies out after the launch
struct KeptTensor { std::string name; const void* dev; size_t per_patch; bool is_half; int plane_hw = 0, plane_c = 0; };   // planes: see Saved
struct Launch {
    std::string name;                         // as mmc_backbone_profile reports it, before the '|'
    const char* label[2] = {nullptr, nullptr};   // ... and behind it; a pw_gemm launch has one per mt (gemm_mt), every other the same twice
    Op op = Op::Stem;
    const PwLayer* layer = nullptr;           // Gemm: the layer gemm_mt asks
    int rows = 0;                             // Gemm, ThinProj, GemmFp8: rows per patch (M = n * rows)
    bool planar = false;                      // ThinProj: X comes as 32-channel planes of n * rows rows
    bool features = false;                    // Gemm, Tail7: writes the pass's features (Stem and StemDw read the pass's patches)
    unsigned mid_phases = 0;                  // Chain14: bit p set when phase p is a mid14m body (clear: proj_patch); each carries its own B
    union Args {
        StemArgs stem; MbtArgs mbt; Mid14Args mid; Mb1Args mb1; MbArgs mb; MbPreArgs pre; GemmArgs gemm; Fp8GemmArgs fp8; DwArgs dw;
        SeLaunch se; ProjPatchArgs pp; Chain14Args chain; TailArgs tail;
        Args() { memset(static_cast<void*>(this), 0, sizeof *this); }
    } a;                                      // everything but the per-call fields
    std::vector<KeptTensor> keep;
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
        std::vector<Launch> list;   // this lane's pass (build_lane); immutable after create
    };
    Lane lanes[4];
    size_t cap_act = 0, cap_exp = 0, cap_dw = 0, cap_pool = 0, cap_gate = 0;   // elements per patch of each lane buffer (create, step 4)
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
    int chain_cout = 0, chain_ce = 0;        // ... the widest block output / expanded tensor among them (see build_lane)
    bool fp8 = false;                // MMC_PRECISION_FP8: project convs of the narrow late blocks on e4m3 MFMA operands
    float* dbg_clk = nullptr;        // keep mode: per-patch phase cycle counts of the patch-resident kernels
    float* mid_clk = nullptr;        // MMC_TAIL_CLK=1: [max_batch][8 workgroups][16] phase cycle counts of block 10's mid14 launch
    float* tail_clk = nullptr;       // MMC_TAIL_CLK=1: [max_batch][8 sections][8] phase cycle counts of the production tail7 launch
    std::vector<TailBlock> tail_rows;   // tail7_kernel's block table (blocks 12..15) as bind_tail_block fills it ...
    TailArgs tail_args{};               // ... on the device in tail_args.blk, with block 11's (pre_*) and the head's weights and inv_hw
    GemmArgs head_gemm{};               // the head conv on pw_gemm (no tail7 head phase)
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

struct ProfEntry { const Launch* launch; int mt; hipEvent_t e0, e1; };   // reported as name|label[mt - 1]
struct Prof { std::vector<ProfEntry> entries; };

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

// ... into the pointer-to-const field of a launch struct
template <typename T>
static int dev_upload(mmc_backbone* bb, const T** p, const std::vector<T>& host)
{
    T* d = nullptr;
    const int r = dev_upload(bb, &d, host);
    *p = d;
    return r;
}

static int upload_pw(mmc_backbone* bb, PwLayer* L, const PwImage& img)
{
    L->N = img.N; L->K = img.K; L->Kp = img.Kp; L->nt = img.nt; L->n_chunks = img.n_chunks;
    int r = dev_upload(bb, &L->w, img.w);
    if (r) return r;
    return dev_upload(bb, &L->b, img.b);
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
    // mode runs the same two kernels and hands the planes out as NHWC (planes_to_nhwc)
    B.planar = B.front == Front::Mb1 && thin && o.b1_planar && P.K == 96;
    return 0;
}

// ------------------------------------------------------------------------------------------
// binding: one function per kernel family.  It packs that family's weight images (backbone_pack.h), uploads them and writes the
// pointers and the constant scalars into the struct its launcher reads -- so who packs a buffer and who reads it is one place.
// An image two families read has one upload helper, and a block runs it once.
// ------------------------------------------------------------------------------------------
#define BIND(expr)                                 \
    do { int r__ = (expr); if (r__) return r__; } while (0)

// (the depthwise taps see a log2(e)-scaled input and produce a scaled output, except in an expand-less block behind a project conv)
static double dw_tap_scale(const BlockW& B, int i) { return (B.has_expand || i == 0) ? 1.0 : LOG2E; }

// a pw_gemm / thin_proj launch of layer L: everything but the buffers, the row count and mt (gemm_mt, per call)
static GemmArgs gemm_args(const PwLayer& L, int epi, bool gate, int HW)
{
    GemmArgs a{};
    a.K = L.K; a.Wp = L.w; a.Kp = L.Kp; a.bias = L.b; a.N = L.N; a.nt = L.nt; a.n_chunks = L.n_chunks; a.epi = epi; a.HW = HW;
    a.inv_hw = (float)(1.0 / ((double)HW * LOG2E));  // GAP input is log2(e)-scaled
    a.defer_gate = gemm_defer_gate(gate, HW);
    return a;
}

// expand weights in MFMA fragment order [ce/16][ksteps][64][8], permuted from their natural fp16 rows (mbt, mid14, tail7)
static int upload_exp_frag(mmc_backbone* bb, const BlockW& B, const RawBlock& R, const _Float16** dst)
{
    const int kp = 32 * B.mb.ksteps;
    const std::vector<_Float16> wn = pack_expand_rows(R.exp_w, B.ce, B.d.cin, kp);
    return dev_upload(bb, dst, pack_frag(wn.data(), B.ce, B.d.cin, kp, B.ce / 16, B.mb.ksteps, 1.0));
}

// depthwise taps as fp16 pairs + the bias, in 16-byte requests [4][ce][4] (mid14, tail7)
static int upload_dw_requests(mmc_backbone* bb, const BlockW& B, const RawBlock& R, const uint32_t** dst)
{
    const std::vector<uint32_t> dp = pack_dw_pairs(R.dw_w, B.ce, B.d.k);
    const std::vector<float> db = pack_bias(R.dw_b, B.ce, B.ce, LOG2E);   // the bias exactly as dw_b holds it
    return dev_upload(bb, dst, pack_dw_requests(dp.data(), db.data(), B.ce));
}

// Wr^T [ce][cs4] and We^T [cs4][ce] in fp16 + the squeeze bias padded to 32 (proj_patch, tail7's block 11)
static int upload_se_t16(mmc_backbone* bb, const BlockW& B, const RawBlock& R, const _Float16** wr_t, const _Float16** we_t, const float** br)
{
    BIND(dev_upload(bb, wr_t, pack_se_fc1_t16(R.se_wr, B.ce, B.cs, B.cs4)));
    BIND(dev_upload(bb, we_t, pack_se_fc2_t16(R.se_we, B.ce, B.cs, B.cs4)));
    return dev_upload(bb, br, pack_bias(R.se_br, B.cs, B.cs4 > 32 ? B.cs4 : 32, 1.0));
}

// what every block uploads, whichever kernels run it: the pw_gemm images + padded biases of expand and project, the tap-major
// depthwise taps, the depthwise and the excite bias
static int bind_shared(mmc_backbone* bb, BlockW& B, int i, const RawBlock& R)
{
    if (B.has_expand) BIND(upload_pw(bb, &B.expand, pack_pw(R.exp_w, R.exp_b, B.ce, B.d.cin, B.expand.nt, LOG2E, LOG2E)));
    BIND(dev_upload(bb, &B.dw_w, pack_dw_taps(R.dw_w, B.ce, B.d.k, dw_tap_scale(B, i))));
    BIND(dev_upload(bb, &B.dw_b, pack_bias(R.dw_b, B.ce, B.ce, LOG2E)));
    BIND(dev_upload(bb, &B.se_be, pack_bias(R.se_be, B.ce, B.ce, 1.0)));
    return upload_pw(bb, &B.project, pack_pw(R.proj_w, R.proj_b, B.d.cout, B.ce, B.project.nt, 1.0 / LOG2E, 1.0));
}

static int bind_mbt(mmc_backbone* bb, BlockW& B, int i, const RawBlock& R)
{
    MbtArgs& a = B.mbt;
    BIND(upload_exp_frag(bb, B, R, &a.wexp));
    BIND(dev_upload(bb, &a.dwp, pack_dw_pairs(R.dw_w, B.ce, B.d.k)));
    if (B.mbt4) BIND(dev_upload(bb, &a.dwtoe, pack_dw_toeplitz(R.dw_w, B.ce, B.d.k, dw_tap_scale(B, i))));
    a.bexp = B.expand.b; a.bdw = B.dw_b;
    a.H = B.H; a.Cin = B.d.cin; a.Ce = B.ce; a.ks = B.d.k; a.stride = B.d.s;
    return 0;
}

static int bind_mid14(mmc_backbone* bb, BlockW& B, int i, const RawBlock& R)
{
    Mid14Args& a = B.mid;
    BIND(upload_exp_frag(bb, B, R, &a.wexp));
    BIND(upload_dw_requests(bb, B, R, &a.dwp));
    if (B.mid14m) BIND(dev_upload(bb, &a.dwdiag, pack_dw_toeplitz(R.dw_w, B.ce, B.d.k, dw_tap_scale(B, i))));
    a.bexp = B.expand.b; a.bdw = B.dw_b;
    a.Cin = B.d.cin; a.Ce = B.ce; a.ks = B.d.k;
    a.nsplit = B.mid14m ? 1 : 4;
    return 0;
}

// block 1 behind block 0's folded project (mb1_kernel, or mbconv_a_kernel PRE with mb1's pre_w / pre_b next to `mb`): block 0's
// project conv as ONE MFMA fragment (16 outputs x 32 inputs), block 1's expand rows K-permuted to match
static int bind_mb1(mmc_backbone* bb, BlockW& B, const RawNet& raw)
{
    const int kp = 32 * B.mb.ksteps;
    Mb1Args& m = B.mb1;
    BIND(dev_upload(bb, &m.pre_w, pack_frag(raw.blk[0].proj_w, 16, 32, 32, 1, 1, 1.0 / LOG2E)));
    const std::vector<_Float16> wn = pack_expand_rows(raw.blk[1].exp_w, B.ce, B.d.cin, kp);
    BIND(dev_upload(bb, &m.wexp, pack_expand_kperm(wn.data(), B.ce, kp)));
    m.pre_b = bb->blk[0].project.b; m.bexp = B.expand.b; m.wdw = B.dw_w; m.bdw = B.dw_b;
    m.planar = B.planar ? 1 : 0;
    if (B.front == Front::MbPre) {   // reads block 0's depthwise output: 32 input channels
        MbArgs& a = B.mb;
        a.Cin = 32; a.Wexp = m.wexp; a.bexp = B.expand.b; a.Wdw = B.dw_w; a.bdw = B.dw_b;
    }
    return 0;
}

static int bind_mb(mmc_backbone* bb, BlockW& B, const RawBlock& R)   // mbconv_a, mbconv_d
{
    MbArgs& a = B.mb;
    BIND(dev_upload(bb, &a.Wexp, pack_expand_rows(R.exp_w, B.ce, B.d.cin, 32 * a.ksteps)));
    a.bexp = B.expand.b; a.Wdw = B.dw_w; a.bdw = B.dw_b;
    return 0;
}

static int bind_unfused(BlockW& B)   // expand GEMM + dwconv: shared images only
{
    if (B.has_expand) B.exp_gemm = gemm_args(B.expand, EPI_SILU, false, B.H * B.H);
    DwArgs& d = B.dw;
    d.wt = B.dw_w; d.bias = B.dw_b;
    d.H = B.H; d.W = B.H; d.C = B.ce; d.Ho = B.Ho; d.Wo = B.Ho; d.pad_t = B.pad; d.pad_l = B.pad;
    d.ks = B.d.k; d.stride = B.d.s; d.tw = B.tw; d.CG = B.CG; d.S = B.S; d.iters = B.iters; d.parts = B.parts; d.nz = B.nz;
    return 0;
}

// tail7's front half of block i: a row of its block table (12..15), or the pre_* arguments of all of block 11 (TailRoute::B11All)
static int bind_tail_front(mmc_backbone* bb, BlockW& B, int i, const RawBlock& R)
{
    if (i == 11) {
        TailArgs& t = bb->tail_args;
        BIND(upload_exp_frag(bb, B, R, &t.pre_wexp));
        BIND(upload_dw_requests(bb, B, R, &t.pre_dwp));
        t.pre_bexp = B.expand.b; t.pre_bdw = B.dw_b;
        return 0;
    }
    TailBlock& t = bb->tail_rows[i - 12];
    BIND(upload_exp_frag(bb, B, R, &t.wexp));
    BIND(upload_dw_requests(bb, B, R, &t.dwp));
    t.bexp = B.expand.b; t.bdw = B.dw_b; t.ks = B.d.k;
    return 0;
}

static int bind_front(mmc_backbone* bb, BlockW& B, int i, const RawNet& raw)
{
    const RawBlock& R = raw.blk[i];
    switch (B.front) {
    case Front::StemDw: return 0;   // launch_stem_dw takes the stem's buffers and the shared taps
    case Front::Mbt: return bind_mbt(bb, B, i, R);
    case Front::Mid14: return bind_mid14(bb, B, i, R);
    case Front::Mb1: case Front::MbPre: return bind_mb1(bb, B, raw);
    case Front::MbD: case Front::MbA: return bind_mb(bb, B, R);
    case Front::Unfused: return bind_unfused(B);
    case Front::Tail: return bind_tail_front(bb, B, i, R);
    }
    return 0;
}

static int bind_proj_patch(mmc_backbone* bb, BlockW& B, const RawBlock& R)
{
    ProjPatchArgs& a = B.pp;
    const _Float16* wr_t = nullptr;   // (uploaded as it always was; proj_patch_kernel reads the grouped copy)
    BIND(upload_se_t16(bb, B, R, &wr_t, &a.we_t, &a.br));
    const std::vector<_Float16> wrt = pack_se_fc1_t16(R.se_wr, B.ce, B.cs, B.cs4);
    BIND(dev_upload(bb, &a.wr_g, pack_se_fc1_groups(wrt.data(), B.ce, B.cs4, proj_patch_fc1_rows(B.ce))));
    // K and N zero-padded to whole fragments
    const int nf = (B.d.cout + 15) / 16;
    BIND(dev_upload(bb, &a.wfrag, pack_frag(R.proj_w, B.d.cout, B.ce, B.ce, nf, proj_patch_ksteps(B.ce), 1.0 / LOG2E)));
    BIND(dev_upload(bb, &a.bias, pack_bias(R.proj_b, B.d.cout, 16 * nf, 1.0)));
    a.be = B.se_be;
    a.HW = B.Ho * B.Ho; a.K = B.ce; a.N = B.d.cout; a.CSP = B.cs4; a.nparts = B.nparts;
    a.psc = (float)(1.0 / ((double)a.HW * LOG2E));
    return 0;
}

// the squeeze-excite launch: se_fused_kernel's fragment order, or natural fp32 rows (se_small_kernel; se_wide_kernel reads the excite
// FC transposed)
static int bind_se(mmc_backbone* bb, BlockW& B, const RawBlock& R)
{
    SeArgs& s = B.sea;
    const double psc = 1.0 / ((double)B.Ho * B.Ho * LOG2E);   // FC1 on pooled sums of HW log2(e)-scaled activations
    s.be = B.se_be;
    switch (B.se) {
    case Se::Fused:
        BIND(dev_upload(bb, &s.wr, pack_se_fc1_frag(R.se_wr, B.ce, B.cs, psc)));
        BIND(dev_upload(bb, &s.we, pack_se_fc2_frag(R.se_we, B.ce, B.cs)));
        BIND(dev_upload(bb, &s.br, pack_bias(R.se_br, B.cs, B.cs > 48 ? B.cs : 48, 1.0)));
        s.Cs = B.cs4;
        return 0;
    case Se::Small:
        BIND(dev_upload(bb, &s.wr, pack_se_fc1_nat(R.se_wr, B.ce, B.cs, psc)));
        BIND(dev_upload(bb, &s.we, std::vector<float>(R.se_we, R.se_we + (size_t)B.ce * B.cs)));
        break;
    case Se::Wide:
        BIND(dev_upload(bb, &s.wr, pack_se_fc1_nat(R.se_wr, B.ce, B.cs, psc)));
        BIND(dev_upload(bb, &s.we, pack_se_fc2_t(R.se_we, B.ce, B.cs)));
        break;
    }
    s.Cs = B.cs;
    return dev_upload(bb, &s.br, pack_bias(R.se_br, B.cs, B.cs, 1.0));
}

static int bind_project(mmc_backbone* bb, BlockW& B, const RawBlock& R)
{
    const int HWo = B.Ho * B.Ho;
    switch (B.proj) {
    case Proj::Thin: case Proj::Gemm: B.proj_gemm = gemm_args(B.project, EPI_LINEAR, true, HWo); return 0;
    case Proj::Fp8: {
        const Fp8Image L = pack_fp8(R.proj_w, R.proj_b, B.d.cout, B.ce);
        Fp8GemmArgs& a = B.proj8;
        BIND(dev_upload(bb, &a.W8, L.w8));
        BIND(dev_upload(bb, &a.sw, L.sw));
        BIND(dev_upload(bb, &a.bias, L.b));
        a.K = L.K; a.KS128 = L.KS128; a.NFp = L.NFp; a.N = L.N; a.HW = HWo;
        return 0;
    }
    }
    return 0;
}

// tail7's back half of block i: the rest of its table row (12..15), or the pre_* arguments of block 11's back half
static int bind_tail_back(mmc_backbone* bb, BlockW& B, int i, const RawBlock& R)
{
    if (i == 11) {
        TailArgs& t = bb->tail_args;
        BIND(upload_se_t16(bb, B, R, &t.pre_wr_t, &t.pre_we_t, &t.pre_br));
        // [12][24][64][8], k-steps 21..23 zero (its k-loop runs 4 steps at a time)
        BIND(dev_upload(bb, &t.pre_wproj, pack_frag(R.proj_w, B.d.cout, B.ce, B.ce, 12, 24, 1.0 / LOG2E)));
        t.pre_be = B.se_be; t.pre_bproj = B.project.b;
        return 0;
    }
    TailBlock& t = bb->tail_rows[i - 12];
    const std::vector<_Float16> wrt = pack_se_fc1_t16(R.se_wr, B.ce, B.cs, B.cs4), wet = pack_se_fc2_t16(R.se_we, B.ce, B.cs, B.cs4);
    BIND(dev_upload(bb, &t.wr_t, pack_tail_fc1(wrt.data())));
    BIND(dev_upload(bb, &t.we_t, pack_tail_fc2(wet.data())));
    BIND(dev_upload(bb, &t.br, pack_bias(R.se_br, B.cs, B.cs > 48 ? B.cs : 48, 1.0)));
    BIND(dev_upload(bb, &t.wproj, pack_frag(R.proj_w, B.d.cout, B.ce, B.ce, B.d.cout / 16, B.ce / 32, 1.0 / LOG2E)));
    t.be = B.se_be; t.bproj = B.project.b; t.cout = B.d.cout;
    return 0;
}

static int bind_back(mmc_backbone* bb, BlockW& B, int i, const RawBlock& R)
{
    switch (B.back) {
    case Back::ProjPatch: return bind_proj_patch(bb, B, R);
    case Back::SeFolded: return bind_se(bb, B, R);   // its project runs inside block 1's kernel (bind_mb1)
    case Back::SeProject:
        BIND(bind_se(bb, B, R));
        return bind_project(bb, B, R);
    case Back::Tail: return bind_tail_back(bb, B, i, R);
    }
    return 0;
}

// the stem, every block, the head and tail7's table
static int bind_net(mmc_backbone* bb, const RawNet& raw)
{
    BIND(dev_upload(bb, &bb->stem_w, pack_stem(raw.stem_w, bb->stem_ch)));
    BIND(dev_upload(bb, &bb->stem_b, pack_bias(raw.stem_b, bb->stem_ch, bb->stem_ch, LOG2E)));
    BIND(dev_upload(bb, &bb->stem_pad, std::vector<float>{raw.stem_pad[0], raw.stem_pad[1], raw.stem_pad[2], 0.f}));
    bb->tail_rows.assign(bb->tail != TailRoute::None ? 4 : 0, TailBlock{});
    for (int i = 0; i < bb->nblk; ++i) {
        BlockW& B = bb->blk[i];
        BIND(bind_shared(bb, B, i, raw.blk[i]));
        BIND(bind_front(bb, B, i, raw));
        BIND(bind_back(bb, B, i, raw.blk[i]));
    }
    BIND(upload_pw(bb, &bb->head, pack_pw(raw.head_w, raw.head_b, bb->feat, bb->head_in, bb->head.nt, LOG2E, LOG2E)));
    TailArgs& t = bb->tail_args;
    if (bb->tail == TailRoute::B11 || bb->tail == TailRoute::B11All) {   // the same weights in plain fragment order for tail7's head phase
        BIND(dev_upload(bb, &t.head_w, pack_frag(raw.head_w, bb->feat, bb->head_in, bb->head_in, bb->feat / 16, bb->head_in / 32, LOG2E)));
        t.head_b = bb->head.b;
    } else {
        const int HWh = bb->blk[bb->nblk - 1].Ho * bb->blk[bb->nblk - 1].Ho;
        bb->head_gemm = gemm_args(bb->head, EPI_GAP, false, HWh);
    }
    if (bb->tail != TailRoute::None) {
        BIND(dev_upload(bb, &t.blk, bb->tail_rows));
        t.inv_hw = (float)(1.0 / (49.0 * LOG2E));
    }
    return 0;
}
#undef BIND

// ------------------------------------------------------------------------------------------
// the launch list of lane `lane_idx`, from the plan's enums and the bound structs, once the workspace is allocated: which buffer every
// launch reads and writes (the x / y ping-pong of the block outputs resolved), the names, and what per-tensor mode keeps
// ------------------------------------------------------------------------------------------
static int build_lane(mmc_backbone* bb, int lane_idx)
{
    mmc_backbone::Lane& ws = bb->lanes[lane_idx];
    std::vector<Launch>& list = ws.list;
    const size_t lc = (size_t)bb->lane_cap;
    int err = 0;
    auto add = [&](const std::string& name, const char* label, Op op) -> Launch& {
        list.emplace_back();
        Launch& L = list.back();
        L.name = name; L.label[0] = L.label[1] = label; L.op = op;
        return L;
    };
    auto add_gemm = [&](const std::string& name, const PwLayer& P, const GemmArgs& a, int rows) -> GemmArgs& {
        Launch& L = add(name, P.label[0], Op::Gemm);
        L.label[1] = P.label[1]; L.layer = &P; L.rows = rows; L.a.gemm = a;
        return L.a.gemm;
    };
    auto bn = [](int i, const char* what) { return "b" + std::to_string(i) + what; };
    // The last entry writes `per_patch` elements per patch at p: with lane_cap patches that must end inside the lane buffer p lies in
    // (step 4 of create sized the buffers from per-block maxima; this ties those sizes to what is launched).  Under a name, per-tensor
    // mode copies the tensor out behind the launch.
    auto writes = [&](auto* p, size_t per_patch, const std::string& keep_as = std::string()) {
        if (bb->keep && !keep_as.empty()) list.back().keep.push_back({keep_as, p, per_patch, sizeof(*p) == 2});
        const struct { const char* name; const void* base; size_t bytes; } bufs[] = {
            {"act0", ws.act0, lc * bb->cap_act * 2}, {"act1", ws.act1, lc * bb->cap_act * 2}, {"expbuf", ws.expbuf, lc * bb->cap_exp * 2},
            {"dwbuf", ws.dwbuf, lc * bb->cap_dw * 2}, {"pool_part", ws.pool_part, lc * bb->cap_pool * 4}, {"gate", ws.gate, lc * bb->cap_gate * 4}};
        const char* b = reinterpret_cast<const char*>(p);
        const size_t bytes = lc * per_patch * sizeof(*p);
        for (const auto& f : bufs) {
            const char* base = static_cast<const char*>(f.base);
            if (b < base || b >= base + f.bytes) continue;
            if (!err && b + bytes > base + f.bytes)
                err = fail(MMC_ERR_ARG, "launch %s writes %zu bytes at offset %zu of lane buffer %s, which holds %zu", list.back().name.c_str(),
                           bytes, (size_t)(b - base), f.name, f.bytes);
            return;
        }
        if (!err) err = fail(MMC_ERR_ARG, "launch %s writes outside every lane buffer", list.back().name.c_str());
    };
    _Float16 *x = ws.act0, *y = ws.act1;   // the block's input, and where its output goes
    // The chained launch: its members' arguments are collected in launch order into ONE entry.  Its workgroups are NOT in step: while
    // workgroup b writes a phase's output, another may still be reading an earlier phase's input.  A buffer's patch b starts at
    // b x (pixels x row width), so two tensors of different row width in one buffer overlap ACROSS patches -- between separate launches
    // that is harmless, inside the chain it is a race.  So a chained tensor whose row width differs from what its buffer holds when the
    // chain starts (block ch0's widths) lives in the buffer's upper part, beyond lane_cap patches of the widest tensor: every region
    // then holds ONE row width, and a workgroup only ever touches its own patch's rows of it.
    const int ch0 = bb->chain_first, ch1 = bb->chain_last;
    const size_t ch_hw = ch0 >= 0 ? (size_t)bb->blk[ch0].Ho * bb->blk[ch0].Ho : 0;
    auto ch_act = [&](_Float16* base, int cout) { return base + (cout == bb->blk[ch0].d.cout ? 0 : lc * ch_hw * bb->chain_cout); };
    auto ch_dw = [&](int ce) { return ws.dwbuf + (ce == bb->blk[ch0].ce ? 0 : lc * ch_hw * bb->chain_ce); };
    auto ch_pool = [&](int ce) { return ws.pool_part + (ce == bb->blk[ch0].ce ? 0 : lc * bb->chain_ce); };
    _Float16 *xbase = nullptr, *ybase = nullptr;   // inside the chain: the buffers x and the next output live in
    if (!bb->fuse_stem) {   // (fused: the stem tensor never exists in HBM, no "stem" activation to keep)
        add("stem", "stem_conv", Op::Stem).a.stem.out = x;
        writes(x, (size_t)112 * 112 * bb->stem_ch, "stem");
    }
    for (int i = 0; i < bb->nblk; ++i) {
        const BlockW& B = bb->blk[i];
        if (B.front == Front::Tail) break;
        const int HWi = B.H * B.H, HWo = B.Ho * B.Ho;
        const bool chained = ch0 >= 0 && i >= ch0 && i <= ch1;   // its back half is a phase of the chain, and behind ch0 its front half too
        // ---- front half: the depthwise output D and its pool partials ----
        // with block 0's project folded into block 1's kernel block 0's depthwise output goes to the spare activation buffer (block 1
        // reads it while writing its own depthwise output to dwbuf)
        _Float16* D = (i == 0 && bb->fuse_b0b1) ? y : (chained && i > ch0) ? ch_dw(B.ce) : ws.dwbuf;
        float* pool = (chained && i > ch0) ? ch_pool(B.ce) : ws.pool_part;
        switch (B.front) {
        case Front::StemDw: add("stem+b0.dw", "stem_dw", Op::StemDw).a.stem = {B.dw_w, B.dw_b, D, pool}; break;
        case Front::Mbt: {
            MbtArgs& a = add(bn(i, ".mbconv"), B.front_label, Op::Mbt).a.mbt = B.mbt;
            a.X = x; a.D = D; a.pool = pool;
            break;
        }
        case Front::Mid14: {
            Mid14Args a = B.mid;
            a.X = x; a.D = D; a.pool = pool;
            if (bb->mid_clk && i == 10) a.dbg_clk = bb->mid_clk + (size_t)lane_idx * lc * 128;   // debug clock: rows of this lane's patches
            if (chained && i > ch0) {   // a phase of the chain entry
                Chain14Args& ca = list.back().a.chain;
                list.back().mid_phases |= 1u << ca.nph;
                ca.ph[ca.nph].kind = chain14_mid_kind(a.Cin, a.ks, a.Ce);
                ca.ph[ca.nph++].mid = a;
            } else
                add(bn(i, ".mbconv"), B.front_label, Op::Mid14).a.mid = a;
            break;
        }
        case Front::Mb1: {   // reads block 0's depthwise output (in y: no swap behind Back::SeFolded) and its gate
            // (per-tensor mode says which instantiation ran; the product pass keeps the one label its profiles are keyed by)
            Mb1Args& a = add("b0.project+b1.mbconv", bb->keep && B.planar ? "mb1<planar>" : "mb1", Op::Mb1).a.mb1 = B.mb1;
            a.X = y; a.pre_gate = ws.gate; a.D = D; a.pool = pool;
            break;
        }
        case Front::MbPre: {   // ... the same on mbconv_a_kernel PRE
            MbPreArgs& a = add("b0.project+b1.mbconv", B.front_label, Op::MbPre).a.pre = {B.mb, B.mb1.pre_w, B.mb1.pre_b, ws.gate};
            a.mb.X = y; a.mb.out = D; a.mb.pool_part = pool;
            break;
        }
        case Front::MbD: case Front::MbA: {
            MbArgs& a = add(bn(i, ".mbconv"), B.front_label, B.front == Front::MbD ? Op::MbD : Op::MbA).a.mb = B.mb;
            a.X = x; a.out = D; a.pool_part = pool;
            break;
        }
        case Front::Unfused: {
            const _Float16* dw_in = x;
            if (B.has_expand) {
                GemmArgs& g = add_gemm(bn(i, ".expand"), B.expand, B.exp_gemm, HWi);
                g.X = x; g.Y = ws.expbuf;
                writes(ws.expbuf, (size_t)HWi * B.ce, bn(i, ".expand"));
                dw_in = ws.expbuf;
            }
            DwArgs& d = add(bn(i, ".dw"), B.front_label, Op::Dw).a.dw = B.dw;
            d.in = dw_in; d.out = D; d.pool_part = pool;
            break;
        }
        case Front::Tail: break;
        }
        writes(D, (size_t)HWo * B.ce, bn(i, ".dw"));
        if (bb->keep && B.planar) { list.back().keep.back().plane_hw = HWo; list.back().keep.back().plane_c = B.ce; }
        writes(pool, (size_t)B.nparts * B.ce);
        // ---- back half ----
        if (B.back == Back::Tail) break;   // block 11's back half: the tail launch below
        if (B.back == Back::ProjPatch) {
            // squeeze-excite + project, one patch per workgroup (proj_patch_kernel): no gate tensor, one launch
            ProjPatchArgs pa = B.pp;
            pa.X = D; pa.pool_part = pool; pa.res = B.skip ? x : nullptr; pa.Y = y;
            pa.dbg_gate = bb->keep ? ws.gate : nullptr;
            pa.dbg_clk = bb->keep ? bb->dbg_clk : nullptr;
            if (chained) {
                if (i == ch0) {
                    xbase = x; ybase = y;
                    add(bn(ch0, ".projse-") + bn(ch1, ".projse.chain"), "chain14", Op::Chain14);
                }
                pa.Y = ch_act(ybase, B.d.cout);
                Chain14Args& ca = list.back().a.chain;
                ca.ph[ca.nph].kind = chain14_proj_kind(pa.K, pa.N, pa.HW, pa.res ? 1 : 0);
                ca.ph[ca.nph++].pp = pa;
                writes(pa.Y, (size_t)HWo * B.d.cout);
                x = pa.Y;
                std::swap(xbase, ybase);
                y = ybase;   // (after the chain: the other buffer, whose tensors are dead by then)
                continue;
            }
            add(bn(i, ".projse"), B.back_label, Op::ProjPatch).a.pp = pa;
            writes(ws.gate, (size_t)B.ce, bn(i, ".gate"));   // (per-tensor mode only: dbg_gate)
            writes(y, (size_t)HWo * B.d.cout, bn(i, ".out"));
            if (bb->keep) list.back().keep.push_back({bn(i, ".clk"), bb->dbg_clk, 8, false});   // the handle's [max_batch][8], no lane buffer
            std::swap(x, y);
            continue;
        }
        add(bn(i, ".gate"), B.se == Se::Wide ? "se_wide" : B.se == Se::Small ? "se_small" : "se_fused",
            B.se == Se::Wide ? Op::SeWide : B.se == Se::Small ? Op::SeSmall : Op::SeFused).a.se = {pool, B.nparts, B.ce, B.sea, ws.gate};
        writes(ws.gate, (size_t)B.ce, bn(i, ".gate"));
        if (B.back == Back::SeFolded) continue;  // block 0's project runs inside block 1's kernel
        const _Float16* res = B.skip ? x : nullptr;
        if (B.proj == Proj::Fp8) {
            Fp8GemmArgs& a = add(bn(i, ".project"), "pw_gemm_fp8", Op::GemmFp8).a.fp8 = B.proj8;
            a.X = D; a.Y = y; a.gate = ws.gate; a.res = res;
            list.back().rows = HWo;
        } else {
            // Proj::Thin: small-K, small-N project on a big image (B4 blocks 0, 1; B0 block 1), one patch's fragments streamed per workgroup
            GemmArgs& a = add_gemm(bn(i, ".project"), B.project, B.proj_gemm, HWo);
            a.X = D; a.Y = y; a.gate = ws.gate; a.res = res;
            if (B.proj == Proj::Thin) {
                Launch& L = list.back();
                L.op = Op::ThinProj; L.label[0] = L.label[1] = bb->keep && B.planar ? "thin_proj<planar>" : "thin_proj"; L.planar = B.planar;
            }
        }
        writes(y, (size_t)HWo * B.d.cout, bn(i, ".out"));
        std::swap(x, y);
    }
    // ---- the tail and the head ----
    // Every tail7 launch starts from the handle's bound TailArgs (block table, block 11's and the head's weights, inv_hw).  The kernel
    // runs block 11 when pre_D or pre_X is set and the head phase when head_w is: a launch without the head phase clears it.
    auto add_tail = [&](const std::string& name, bool head) -> TailArgs& {
        Launch& L = add(name, "tail7", Op::Tail7);
        L.features = head;
        L.a.tail = bb->tail_args;
        if (!head) L.a.tail.head_w = nullptr;
        return L.a.tail;
    };
    if (!bb->keep && (bb->tail == TailRoute::B11All || bb->tail == TailRoute::B11)) {
        // from block 11's input (B11All) or its depthwise output (B11) through blocks 12..15 and the head conv to the features, ONE launch
        TailArgs& ta = add_tail(bb->tail == TailRoute::B11All ? "b11all-head.tail" : "b11-head.tail", true);
        ta.nblk = 4;
        if (bb->tail == TailRoute::B11All) {
            ta.pre_X = x;
        } else {
            ta.pre_D = ws.dwbuf; ta.pre_pool = ws.pool_part;
        }
        if (bb->tail == TailRoute::B11All && bb->tail_clk) {   // debug clock: rows of this lane's patches
            ta.dbg_clk = bb->tail_clk + (size_t)lane_idx * lc * 64; ta.clk_sections = 1;
        }
        return err;
    }
    const bool head_phase = bb->tail == TailRoute::B11 || bb->tail == TailRoute::B11All;   // the head conv runs on tail7_kernel
    if (head_phase) {   // per-tensor mode: block 11 on its own, all of it from the block's input (B11All) or its back half (B11)
        const BlockW& B11 = bb->blk[11];
        TailArgs& ta = add_tail("b11.tail", false);
        ta.nblk = 0; ta.Y = y; ta.dbg_gate = ws.gate;
        if (bb->tail == TailRoute::B11All) {
            ta.pre_X = x; ta.dbg_dw = ws.dwbuf;
            writes(ws.dwbuf, (size_t)49 * B11.ce, "b11.dw");
        } else {
            ta.pre_D = ws.dwbuf; ta.pre_pool = ws.pool_part;
        }
        writes(ws.gate, (size_t)B11.ce, "b11.gate");
        writes(y, (size_t)49 * 192, "b11.out");
        std::swap(x, y);
    }
    if (bb->tail != TailRoute::None && !bb->keep) {
        // blocks 12..15 in one launch, one patch per workgroup, tensors resident in LDS (tail7_kernel)
        TailArgs& ta = add_tail("b12-15.tail", false);
        ta.X = x; ta.Y = y; ta.nblk = 4;
        writes(y, (size_t)49 * bb->blk[15].d.cout);
        std::swap(x, y);
    } else if (bb->tail != TailRoute::None) {
        for (int j = 12; j < 16; ++j) {   // block at a time so every intermediate tensor can be read back
            const BlockW& B = bb->blk[j];
            TailArgs& ta = add_tail(bn(j, ".tail"), false);
            ta.X = x; ta.Y = y; ta.nblk = 1; ta.blk += j - 12;
            ta.dbg_dw = ws.dwbuf; ta.dbg_gate = ws.gate; ta.dbg_clk = ws.pool_part;
            writes(ws.dwbuf, (size_t)49 * B.ce, bn(j, ".dw"));
            writes(ws.gate, (size_t)B.ce, bn(j, ".gate"));
            writes(y, (size_t)49 * B.d.cout, bn(j, ".out"));
            writes(ws.pool_part, 8, bn(j, ".clk"));
            std::swap(x, y);
        }
    }
    if (head_phase) {   // per-tensor mode: the head phase of tail7_kernel on its own
        TailArgs& ta = add_tail("head.tail", true);
        ta.X = x; ta.nblk = 0; ta.in_wide = 1;
    } else {
        const int HWh = bb->blk[bb->nblk - 1].Ho * bb->blk[bb->nblk - 1].Ho;
        add_gemm("head", bb->head, bb->head_gemm, HWh).X = x;
        list.back().features = true;
    }
    return err;
}

extern "C" int mmc_backbone_create_ex(const void* packed, size_t nbytes, int arch, int device, int max_batch, unsigned flags,
                                      mmc_backbone** out)
{
    // ---- 1. arguments and the blob's header ----
    if (!out) return fail(MMC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (flags & ~(unsigned)MMC_PRECISION_FP8) return fail(MMC_ERR_ARG, "unknown flags 0x%x", flags);
    if ((flags & MMC_PRECISION_FP8) && arch != MMC_ARCH_B4)
        return fail(MMC_ERR_ARG, "MMC_PRECISION_FP8 is implemented for MMC_ARCH_B4 (BASELINE configs[4]): B0's late blocks run fused kernels without a separate project GEMM");
    if (!packed || nbytes < 16) return fail(MMC_ERR_WEIGHTS, "weights blob is empty");
    if (arch != MMC_ARCH_B0 && arch != MMC_ARCH_B4) return fail(MMC_ERR_ARG, "unsupported arch %d (MMC_ARCH_B0 or MMC_ARCH_B4)", arch);
    if (max_batch < 1 || max_batch > 4096) return fail(MMC_ERR_ARG, "max_batch %d out of range [1,4096]", max_batch);
    BlobReader rd;
    BlobError berr;
    if (rd.open(packed, nbytes, arch, &berr)) return fail(berr.code, "%s", berr.msg);
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

    // ---- 2. geometry (per block, pure arithmetic), then the plan: pass-level routes, then each block ----
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
        const bool t11all = t11 && o.tail_b11 && B11.mb.ksteps == 4 && B11.d.k == 5 && B11.d.s == 2 && B11.H == 14;
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
            // ... whose tensors come in at most two row widths per buffer, the first block's and a wider one (build_lane places them)
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

    // ---- 3. the blob's tensors in their fixed order, then what the plan launches: packed, uploaded, bound ----
    {
        RawNet raw;
        if (read_blob(rd, AD, &raw, &berr)) {
            mmc_backbone_destroy(bb);
            return fail(berr.code, "%s", berr.msg);
        }
        TRY_OR_FREE(bind_net(bb, raw));
    }

    // ---- 4. workspace and lanes ----
    size_t max_act = (size_t)(IMG / 2) * (IMG / 2) * STEM_CH, max_exp = 0, max_dw = 0, max_pool = 0;
    int max_c = 0;
    for (int i = 0; i < NBLK; ++i) {
        const BlockW& B = bb->blk[i];
        const int H = B.H;
        if (B.fusable) max_pool = std::max(max_pool, (size_t)B.mb.tiles_x * B.mb.tiles_y * B.ce);
        if ((size_t)H * H * B.ce > max_exp && B.has_expand && !B.fusable) max_exp = (size_t)H * H * B.ce;
        max_dw = std::max(max_dw, (size_t)B.Ho * B.Ho * B.ce);
        max_act = std::max(max_act, (size_t)B.Ho * B.Ho * B.d.cout);
        max_pool = std::max(max_pool, (size_t)B.parts * B.ce);
        if (i == 0) max_pool = std::max(max_pool, (size_t)49 * B.ce);
        max_c = std::max(max_c, B.ce);
    }
    if (bb->chain_first >= 0) {   // room for the chained launch's second tensor per buffer
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
        bb->cap_act = max_act; bb->cap_exp = max_exp ? max_exp : 64; bb->cap_dw = max_dw; bb->cap_pool = max_pool; bb->cap_gate = (size_t)max_c;
        for (int l = 0; l < nl; ++l) {
            mmc_backbone::Lane& L = bb->lanes[l];
            TRY_OR_FREE(dev_alloc(bb, &L.act0, lc * bb->cap_act));
            TRY_OR_FREE(dev_alloc(bb, &L.act1, lc * bb->cap_act));
            TRY_OR_FREE(dev_alloc(bb, &L.expbuf, lc * bb->cap_exp));
            TRY_OR_FREE(dev_alloc(bb, &L.dwbuf, lc * bb->cap_dw));
            TRY_OR_FREE(dev_alloc(bb, &L.pool_part, lc * bb->cap_pool));
            TRY_OR_FREE(dev_alloc(bb, &L.gate, lc * bb->cap_gate));
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

    // ---- 5. every lane's launch list, each write checked against the buffer sizes of step 4 ----
    for (int l = 0; l < bb->nlanes; ++l) TRY_OR_FREE(build_lane(bb, l));
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

// Replays a lane's launch list on n patches.  An entry's arguments are copied before the per-call fields go in -- the batch (B, or
// M = n x rows with the mt and label that follow from it), the pass's input and its feature output -- so a call leaves nothing behind.
static int forward_lane(mmc_backbone* bb, const std::vector<Launch>& list, const uint8_t* patches_dev, int n, float* out_dev,
                        hipStream_t st, Prof* prof)
{
    for (const Launch& L : list) {
        Launch::Args a = L.a;
        ProfEntry pe{&L, 1, nullptr, nullptr};
        if (prof) {
            HIP_TRY(hipEventCreate(&pe.e0));
            HIP_TRY(hipEventCreate(&pe.e1));
            HIP_TRY(hipEventRecord(pe.e0, st));
        }
        const SeLaunch& se = a.se;
        switch (L.op) {
        case Op::Stem: KTRY(launch_stem(patches_dev, bb->stem_w, bb->stem_b, bb->stem_pad, a.stem.out, n, bb->stem_ch, st)); break;
        case Op::StemDw:
            KTRY(launch_stem_dw(patches_dev, bb->stem_w, bb->stem_b, bb->stem_pad, a.stem.wdw, a.stem.bdw, a.stem.out, a.stem.pool, n, st));
            break;
        case Op::Mbt: a.mbt.B = n; KTRY(launch_mbt(a.mbt, st)); break;
        case Op::Mid14: a.mid.B = n; KTRY(launch_mid14(a.mid, st)); break;
        case Op::Mb1: a.mb1.B = n; KTRY(launch_mb1(a.mb1, st)); break;
        case Op::MbA: a.mb.B = n; KTRY(launch_mbconv_a(a.mb, st)); break;
        case Op::MbD: a.mb.B = n; KTRY(launch_mbconv_d(a.mb, st)); break;
        case Op::MbPre: a.pre.mb.B = n; KTRY(launch_mbconv_pre(a.pre.mb, a.pre.pre_w, a.pre.pre_b, a.pre.pre_gate, st)); break;
        case Op::Gemm:
            a.gemm.M = n * L.rows;
            a.gemm.mt = pe.mt = gemm_mt(*L.layer, a.gemm.M);
            if (L.features) a.gemm.gap_out = out_dev;
            KTRY(launch_pw_gemm(a.gemm, st));
            break;
        case Op::ThinProj:
            a.gemm.M = n * L.rows;
            a.gemm.x_plane_rows = L.planar ? n * L.rows : 0;
            KTRY(launch_thin_proj(a.gemm, n, st));
            break;
        case Op::GemmFp8: a.fp8.M = n * L.rows; KTRY(launch_pw_gemm_fp8(a.fp8, st)); break;
        case Op::Dw: a.dw.B = n; KTRY(launch_dwconv(a.dw, st)); break;
        case Op::SeWide: KTRY(launch_se_wide(se.pool, se.nparts, n, se.C, se.w.Cs, se.w.wr, se.w.br, se.w.we, se.w.be, se.gate, st)); break;
        case Op::SeSmall: KTRY(launch_se_small(se.pool, se.nparts, n, se.C, se.w.Cs, se.w.wr, se.w.br, se.w.we, se.w.be, se.gate, st)); break;
        case Op::SeFused: KTRY(launch_se_gate(se.pool, se.nparts, n, se.C, se.w.Cs, se.w.wr, se.w.br, se.w.we, se.w.be, se.gate, st)); break;
        case Op::ProjPatch: a.pp.B = n; KTRY(launch_proj_patch(a.pp, st)); break;
        case Op::Chain14:
            a.chain.B = n;
            for (int p = 0; p < a.chain.nph; ++p) ((L.mid_phases >> p & 1) ? a.chain.ph[p].mid.B : a.chain.ph[p].pp.B) = n;
            KTRY(launch_chain14(a.chain, st));
            break;
        case Op::Tail7:
            a.tail.B = n;
            if (L.features) a.tail.feat = out_dev;
            KTRY(launch_tail7(a.tail, st));
            break;
        }
        if (prof) {
            HIP_TRY(hipEventRecord(pe.e1, st));
            prof->entries.push_back(pe);
        }
        if (bb->keep)   // per-tensor mode (MMC_KEEP_ACTIVATIONS=1): copy the entry's tensors out under their names
            for (const KeptTensor& k : L.keep) {
                const int r = save_act(bb, k.name.c_str(), k.dev, (size_t)n * k.per_patch, k.is_half, st);
                if (r) return r;
                Saved& s = bb->saved[k.name];
                s.plane_hw = k.plane_hw; s.plane_c = k.plane_c;
            }
    }
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
            int r = forward_lane(bb, bb->lanes[0].list, patches_dev + (size_t)off * psz, cur, out_dev + (size_t)off * FEAT, st, prof);
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
            int r = forward_lane(bb, L.list, patches_dev + (size_t)(base + off) * psz, cur, out_dev + (size_t)(base + off) * FEAT, L.stream, prof);
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
        if (s.plane_hw)   // the copy of a launch over n patches: elems = n * plane_hw * plane_c
            tmp = planes_to_nhwc(tmp.data(), (int)(s.elems / ((size_t)s.plane_hw * s.plane_c)), s.plane_hw, s.plane_c);
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
            snprintf(names[cnt], 64, "%s|%s", e.launch->name.c_str(), e.launch->label[e.mt - 1]);
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
