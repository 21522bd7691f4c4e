// kernels.h -- launcher interface between the host units of the C ABI (mmc_api.cpp: network schedule; mmc_head.cpp: calibrated head) and the kernel translation units (k_generic.hip, k_mbconv.hip, k_early.hip, k_mid.hip, k_tail.hip, metrics.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// after a launch, in a launch_* function: hands a launch error back as the function's result
#define LAUNCH_CHECK()                          \
    do {                                        \
        hipError_t e__ = hipGetLastError();     \
        if (e__ != hipSuccess) return (int)e__; \
    } while (0)

enum { EPI_SILU = 0, EPI_LINEAR = 1, EPI_GAP = 2 };

// Each templated family keeps ONE table of its instantiations next to its launcher.  launch_<family>() dispatches on it and
// <family>_label() answers from it: the label (as mmc_backbone_profile reports it) of the instantiation that would run a shape,
// or null when there is none.  mmc_backbone_create asks for every launch it plans, so a missing shape fails there.

// sets the thread-local message mmc_last_error() returns and hands back `code` (defined in mmc_api.cpp)
int mmc_fail(int code, const char* fmt, ...);

struct GemmArgs {
    const _Float16* X;   // [M][K] activations (NHWC rows)
    int M, K;
    const _Float16* Wp;  // [n_chunks*16*nt][Kp] row-permuted, zero padded
    int Kp;
    const float* bias;   // [n_chunks*16*nt] natural channel order, zero padded
    _Float16* Y;         // [M][N]
    int N;
    int mt, nt, n_chunks, defer_gate;
    int epi;
    const float* gate;   // [patch][K] or null
    int HW;              // rows per patch
    const _Float16* res; // [M][N] or null
    float* gap_out;      // EPI_GAP: [patches][N]
    int x_plane_rows;    // thin_proj only: X is [K/32][x_plane_rows][32] planes (0: rows of K)
    float inv_hw;
};

// Project conv on fp8 (OCP e4m3) MFMA operands (pw_gemm_fp8_kernel; BASELINE configs[4]): weights quantised on the host with one
// scale per output channel, activations (x * squeeze-excite gate) quantised in the kernel with one scale per pixel row.
struct Fp8GemmArgs {
    const _Float16* X;   // [M][K] depthwise output (NHWC rows), K a multiple of 8
    int M, K;
    const uint8_t* W8;   // [NFp][KS128][64 lanes][32] e4m3: fragment f = channels 16 f .. +15, lane (i, q) holds k = 128 ks + 32 q .. +31 of channel 16 f + i
    int KS128, NFp;      // k-steps of 128 (K zero padded), fragments (padded to whole workgroups of 7)
    const float* sw;     // [16 NFp] weight scales (0 for padding channels)
    const float* bias;   // [16 NFp]
    _Float16* Y;         // [M][N]
    int N;
    const float* gate;   // [patch][K]
    int HW;              // rows per patch
    const _Float16* res; // [M][N] or null
};
int launch_pw_gemm_fp8(const Fp8GemmArgs& a, hipStream_t st);

struct DwArgs {
    const _Float16* in;
    const float* wt;     // [ks*ks][C]
    const float* bias;   // [C]
    _Float16* out;
    float* pool_part;    // [B][parts][C]
    int B, H, W, C, Ho, Wo, pad_t, pad_l;
    int ks, stride, tw;
    int CG, S, iters, parts;   // CG = channel groups (of 8) per workgroup
    int nz;                    // channel splits (gridDim.z): CG * nz * 8 == C
};

struct MbArgs {
    const _Float16* X;      // [B][H][W][Cin]
    const _Float16* Wexp;   // [Ce][32*ksteps] natural rows, zero-padded K
    const _Float16* Wfrag;  // the same weights in MFMA fragment order [Ce/16][ksteps][64][8]
    const float* bexp;
    const float* Wdw;       // [ks*ks][Ce]
    const float* bdw;
    _Float16* out;          // [B][Ho][Wo][Ce]
    float* pool_part;       // [B][tiles][Ce]
    int B, H, W, Cin, Ce, Ho, Wo, pad;
    int ks, stride, tw, ksteps, npair, pb;
    int TH, TWo, tiles_x, tiles_y, CC, CCG, S;
    int wl_off, red_off, lds_bytes, wfr_off;
};

// One 7x7 MBConv block (192 -> 1152 -> cout, depthwise 5x5 or 3x3, stride 1) packed for tail7_kernel.
struct TailBlock {
    const _Float16* wexp;   // [72][6][64][8] expand weights, MFMA fragment order
    const float* bexp;      // [1152]
    const uint32_t* dwp;    // [4][1152][4] dwords: slots 0..14 = depthwise taps as fp16 pairs (slot 3*ky + d; 5x5: (k0,k1),(k2,k3),(k4,0);
                            // 3x3: (k0,k1),(k2,0),0), slot 15 = the bias (fp32 bits); request j of a channel = slots 4j .. 4j+3
    const float* bdw;       // [1152]
    const _Float16* wr_t;   // [18][384][8] squeeze FC: request p of thread (cr, j4) = Wr^T[64p + cr][4 j4 .. +3], Wr^T[64p + 32 + cr][4 j4 .. +3]
                            // (Wr^T = [1152][48], channel-major; unscaled: 1/(49*log2e) is applied in fp32)
    const float* br;        // [48]
    const _Float16* we_t;   // [24][288][8] excite FC: request p of thread t = We^T[2p][4t .. +3], We^T[2p + 1][4t .. +3] (We^T = [48][1152])
    const float* be;        // [1152]
    const _Float16* wproj;  // [cout/16][36][64][8] project weights, MFMA fragment order
    const float* bproj;     // [cout]
    int cout;               // 192 (skip connection, b12..b14) or 320 (b15, no skip; must be the last block)
    int ks;                 // depthwise kernel size: 5 or 3
};
struct TailArgs {
    const _Float16* X;      // [B][49][192] block input (or [B][49][320] when in_wide); unused with pre_D
    _Float16* Y;            // [B][49][cout of the last block]; unused with head_w
    int B, nblk;            // nblk blocks from the table (0..4)
    const TailBlock* blk;   // device table, nblk consecutive rows
    _Float16* dbg_dw;       // optional [B][49][1152]: depthwise output of the last block run (nblk == 1)
    float* dbg_gate;        // optional [B][1152] (or [B][672] for the pre-block)
    float* dbg_clk;         // optional [B][8]: shader cycles per phase (expand, dw, fc1, fc2, gate, project)
    int clk_sections;       // 0: dbg_clk is [B][8] (one block per launch); 1: [B][8 sections][8] -- section 0 = block 11 (front half, SE,
                            // gate, project), 1..4 = blocks 12..15 (expand, dw, fc1, fc2, gate, project), 5 = head, 6 = whole kernel
    // optional pre-block: second half of block 11 (squeeze-excite + project 672 -> 192, no skip) on its depthwise output
    const _Float16* pre_D;      // [B][49][672] or null
    const float* pre_pool;      // [B][672] pool sums (one tile per patch)
    const _Float16* pre_wr_t;   // [672][28]
    const float* pre_br;        // [28+]
    const _Float16* pre_we_t;   // [28][672]
    const float* pre_be;        // [672]
    // ... or the whole of block 11 from its INPUT (pre_X instead of pre_D / pre_pool): expand 112 -> 672 + depthwise 5x5 stride 2 in LDS
    const _Float16* pre_X;      // [B][196][112] block 11's input, or null
    const _Float16* pre_wexp;   // [42][4][64][8] expand weights, MFMA fragment order
    const float* pre_bexp;      // [672]
    const uint32_t* pre_dwp;    // [4][672][4] depthwise taps as fp16 pairs + bias (layout of TailBlock::dwp)
    const float* pre_bdw;       // [672]
    const _Float16* pre_wproj;  // [12][24][64][8] (k-steps 21..23 zero)
    const float* pre_bproj;     // [192]
    // optional head: conv 320 -> 1280 + swish + average pool -> feat
    const _Float16* head_w;     // [80][10][64][8] or null
    const float* head_b;        // [1280]
    float* feat;                // [B][1280]
    float inv_hw;               // 1 / (49 log2 e)
    int in_wide;                // input X is [B][49][320] (head-only launches)
};
int launch_tail7(const TailArgs& a, hipStream_t st);

// Block 1 front half with block 0's SE scale + project folded in (mb1_kernel)
struct Mb1Args {
    const _Float16* X;        // [B][112][112][32] block 0's depthwise output
    const _Float16* pre_w;    // [64][8] block 0's project conv as one MFMA fragment
    const float* pre_b;       // [16]
    const float* pre_gate;    // [B][32] block 0's squeeze-excite gate
    const _Float16* wexp;     // [96][32] expand weights, natural rows, K-permuted (slot 8q+j <- channel 4q+j, j < 4)
    const float* bexp;        // [96]
    const float* wdw;         // [9][96] depthwise taps (fp32, tap-major)
    const float* bdw;         // [96]
    _Float16* D;              // [B][56][56][96], or planar: [3][B * 56 * 56][32]
    int planar;
    float* pool;              // [B][14][96]
    int B;
};
int launch_mb1(const Mb1Args& a, hipStream_t st);

// Front half of a stride-1 MBConv block on 14x28 output tiles (mbt_kernel: b2, b4)
struct MbtArgs {
    const _Float16* X;        // [B][H][H][Cin]
    const _Float16* wexp;     // [Ce/16][ceil(Cin/32)][64][8] expand weights, MFMA fragment order
    const float* bexp;        // [Ce]
    const uint32_t* dwp;      // [15][Ce] depthwise taps as fp16 pairs (layout of TailBlock::dwp)
    const float* bdw;         // [Ce]
    _Float16* D;              // [B][H][H][Ce]
    float* pool;              // [B][tiles][Ce]
    int B, H, Cin, Ce, ks;
    int stride;               // 1 (b2, b4: D is [B][H][H][Ce]) or 2 (b3, b5: D is [B][H/2][H/2][Ce], mbt2_kernel)
    const _Float16* dwtoe;    // optional [Ce/16][ks][2][64][4]: Toeplitz depthwise fragments -> mbt4_kernel (5x5 stride 1 at 28x28)
};
int launch_mbt(const MbtArgs& a, hipStream_t st);
const char* mbt_label(int H, int ks, int stride, int Cin, int Ce, int dw4);   // dw4: with MbtArgs::dwtoe (mbt4_kernel)

// Front half of a 14x14 MBConv block for one patch per workgroup (mid14_kernel)
struct Mid14Args {
    const _Float16* X;        // [B][196][Cin]
    const _Float16* wexp;     // [Ce/16][ceil(Cin/32)][64][8] expand weights, MFMA fragment order (K zero padded)
    const float* bexp;        // [Ce]
    const uint32_t* dwp;      // [4][Ce][4] depthwise taps as fp16 pairs + bias in 16-byte requests (layout of TailBlock::dwp)
    const float* bdw;         // [Ce]
    _Float16* D;              // [B][196][Ce] depthwise output
    float* pool;              // [B][Ce] pool sums
    int B, Cin, Ce, ks;
    int nsplit;               // workgroups per patch (each takes every nsplit-th chunk of 96 channels)
    float* dbg_clk;           // optional [B][8 workgroups][16]: shader cycles of the first chunk's phases (MMC_TAIL_CLK=1)
    const _Float16* dwdiag;   // optional [Ce/16][ks][2][64][4]: Toeplitz depthwise fragments of v_mfma_f32_4x4x4_16B_f16 -> mid14m_kernel
};
int launch_mid14(const Mid14Args& a, hipStream_t st);
const char* mid14_label(int Cin, int ks, int Ce, int dwm);   // dwm: with Mid14Args::dwdiag (mid14m_kernel)

// Squeeze-excite + project conv of one patch per workgroup (proj_patch_kernel)
struct ProjPatchArgs {
    const _Float16* X;        // [B][HW][K] depthwise output
    const float* pool_part;   // [B][nparts][K] depthwise pool partials
    const _Float16* wr_g;     // [CSP/4][proj_patch_fc1_rows(K)][4] squeeze FC (fp16; group of four outputs, channel, output; zero beyond K)
    const float* br;          // [CSP]
    const _Float16* we_t;     // [CSP][K] excite FC (fp16)
    const float* be;          // [K]
    const _Float16* wfrag;    // [N/16 up][K/32 up][64][8] project weights, MFMA fragment order, zero padded
    const float* bias;        // [16 * ceil(N/16)]
    const _Float16* res;      // [B][HW][N] skip input or null
    _Float16* Y;              // [B][HW][N]
    float* dbg_gate;          // optional [B][K]
    float* dbg_clk;           // optional [B][8]: shader cycles of prologue, GEMM
    int B, HW, K, N, CSP, nparts;
    float psc;                // 1 / (HW * log2 e)
};
int launch_proj_patch(const ProjPatchArgs& a, hipStream_t st);
int proj_patch_ksteps(int K);                        // k-steps (of 32) its weight image must be packed with
int proj_patch_fc1_rows(int K);                      // channel rows per output group of ProjPatchArgs::wr_g (64 x the kernel's FC1 iterations)
const char* proj_patch_label(int K, int N, int HW, int res);

// A run of per-patch launches of the 14x14 blocks as ONE launch (chain14_kernel): workgroup b runs the phases one after the other
// on patch b.  Each phase is a mid14m_kernel (nsplit 1) or proj_patch_kernel body with the arguments its own launch would get
// (debug pointers unused); consecutive phases may only exchange rows of their own patch.
enum { CHAIN14_MAX_PHASES = 7 };
struct Chain14Phase {
    int kind;                 // chain14_proj_kind() / chain14_mid_kind()
    union {
        ProjPatchArgs pp;
        Mid14Args mid;
    };
};
struct Chain14Args {
    int B, nph;
    Chain14Phase ph[CHAIN14_MAX_PHASES];
};
int chain14_proj_kind(int K, int N, int HW, int res);   // the phase kind of a proj_patch / mid14m shape, or -1: not in the chain kernel
int chain14_mid_kind(int Cin, int ks, int Ce);
int launch_chain14(const Chain14Args& a, hipStream_t st);

int launch_mbconv_a(const MbArgs& a, hipStream_t st);
const char* mbconv_a_label(const MbArgs& a);     // (these three read the geometry fields only)
const char* mbconv_pre_label(const MbArgs& a);
const char* mbconv_d_label(const MbArgs& a);
// block 1 reading block 0's depthwise output, with block 0's SE scale + project conv folded in
int launch_mbconv_pre(const MbArgs& a, const _Float16* pre_w, const float* pre_b, const float* pre_gate, hipStream_t st);
int launch_mbconv_d(const MbArgs& a, hipStream_t st);   // dot2 depthwise variant (pair-interleaved LDS tile)
int launch_stem(const uint8_t* patches, const _Float16* w, const float* bias, const float* padval, _Float16* out, int B,
                int channels, hipStream_t st);
int launch_stem_dw(const uint8_t* patches, const _Float16* w, const float* bias, const float* padval, const float* Wdw,
                   const float* bdw, _Float16* out, float* pool_part, int B, hipStream_t st);
int launch_pw_gemm(const GemmArgs& a, hipStream_t st);
const char* pw_gemm_label(int mt, int nt, int epi, int gate, int res, int defer_gate);
// SE-scale + project (+ skip) for K <= 64, N <= 32 (pack_pw weights with nt = 2): one patch's pixel fragments streamed per workgroup
int launch_thin_proj(const GemmArgs& a, int patches, hipStream_t st);
const char* thin_proj_label(int ksteps, int res);
int launch_dwconv(const DwArgs& a, hipStream_t st);
const char* dwconv_label(int ks, int stride, int tw);
int launch_se_gate(const float* pool_part, int nparts, int B, int C, int Cs4, const float* WrP, const float* br,
                   const float* WeP, const float* be, float* gate, hipStream_t st);
int launch_se_small(const float* pool_part, int nparts, int B, int C, int Cs, const float* wr, const float* br,
                    const float* we, const float* be, float* gate, hipStream_t st);
int launch_se_wide(const float* pool_part, int nparts, int B, int C, int Cs, const float* wr, const float* br,
                   const float* we_t /* [Cs][C] */, const float* be, float* gate, hipStream_t st);
int launch_mlp_layer(const float* X, int M, int K, const float* W, const float* bias, float* Y, int N, bool relu,
                     hipStream_t st);
int launch_calibrate(const float* logits, int M, int K, const float* a, const float* b, float* proba, int32_t* argmax,
                     hipStream_t st);
// calibration + the k best classes per row (score descending, ties in class order); proba may be NULL; rowbuf: M x K scratch floats,
// needed only when K > 2048 and proba is NULL
int launch_calibrate_topk(const float* logits, int M, int K, const float* a, const float* b, int k, int32_t* idx, float* scores,
                          float* proba, float* rowbuf, hipStream_t st);
// calibration + per row: best class and its score, rank and probability of the true class y[row] (through label_map when given;
// -1 = unknown); the four per-row outputs may be NULL.  Adds into totals[EVAL_TOTALS] = {rows, correct, unknown, non-finite,
// sum of the 2^-32 fixed-point log-loss}, confusion [K][K] and rank_hist [K] (either may be NULL) with integer atomics: the caller
// zeroes them.  scored [M] or NULL: the true class of a row that entered those tables, -1 for an unknown or non-finite row.
// rowbuf: M x K scratch floats, needed only when K > 2048
constexpr int EVAL_TOTALS = 5;
int launch_calibrate_eval(const float* logits, int M, int K, const float* a, const float* b, const int32_t* y, const int32_t* label_map,
                          int n_labels, int32_t* est, float* score, int32_t* rank, float* p_true, long long* totals, long long* confusion,
                          long long* rank_hist, int32_t* scored, float* rowbuf, hipStream_t st);
// behind launch_calibrate_eval on the same chunk (its `scored` and `rank` outputs, on the device): adds every scored row into
// class_rank_hist [K][K] (true class x rank - 1; may be NULL) and, with sim_level [K][K] (uint8 < n_levels, row = true class), into
// hier_hist [kmax][n_levels]: round j of the top-k selection x the largest level among the row's j + 1 best classes.  sim_level and
// hier_hist come together or not at all; integer atomics, the caller zeroes both tables.  rowbuf: M x K scratch floats, needed
// only when K > 2048 and sim_level is given
constexpr int RANK_MAX_K = 16;
int launch_rank_rows(const float* logits, int M, int K, const float* a, const float* b, const int32_t* scored, const int32_t* rank,
                     const uint8_t* sim_level, int n_levels, int kmax, long long* class_rank_hist, long long* hier_hist, float* rowbuf,
                     hipStream_t st);
int launch_crop(const uint8_t* image, int H, int W, const int32_t* rowcols, int n, uint8_t* out, hipStream_t st);
// calibration of the G rows of each point -> their mean per class (left to right in row order, / (float)G) -> the k best classes
// of the mean, chosen as launch_calibrate_topk chooses them.  logits: (P * G) x K, rows p G .. p G + G - 1 = point p.
// idx / scores: P x k; proba: P x K means or NULL; rowbuf: P x K scratch floats, needed only when K > 2048 and proba is NULL
constexpr int VIEWS_MAX = 16;   // view codes 0 .. 15, and at most this many rows per point
int launch_mean_topk(const float* logits, int P, int G, int K, const float* a, const float* b, int k, int32_t* idx, float* scores,
                     float* proba, float* rowbuf, hipStream_t st);
// ---- head ensembles (include/mmc.h, "head ensembles") ----
constexpr int ENSEMBLE_MAX = 16;     // members
constexpr int ENSEMBLE_MAX_K = 2048; // classes: the two LDS rows per wave of the ensemble kernels
constexpr int ENSEMBLE_STATS = 3;    // per point: H(e), mean member entropy, their difference
// one member's Linear layer: Y[M][N] = act(X[M][K] W[N][K]^T + bias), K a multiple of 4 (rows 16-byte aligned), relu 0 / 1
struct MlpGroupMember {
    const float* X;
    const float* W;
    const float* bias;
    float* Y;
    int K, N, relu, pad;
};
struct MlpGroupArgs {
    MlpGroupMember m[ENSEMBLE_MAX];
    int M;   // rows, the same for every member
};
// the layer of members m[0 .. members) in one launch; each output has the bits launch_mlp_layer gives that member alone
int launch_mlp_group(const MlpGroupArgs& g, int members, hipStream_t st);
// the members' Platt parameters (K floats each, device)
struct EnsembleCal {
    const float* a[ENSEMBLE_MAX];
    const float* b[ENSEMBLE_MAX];
};
// logits: member j's rows at logits + j * member_stride, (P * G) x K each.  Per point the mean over views and members, its k best
// classes as launch_calibrate_topk chooses them; proba (P x K means), stats (P x ENSEMBLE_STATS) and votes (P) may be NULL
int launch_ensemble_topk(const float* logits, int P, int G, int K, int Mn, size_t member_stride, const EnsembleCal& cal, int k,
                         int32_t* idx, float* scores, float* proba, float* stats, int32_t* votes, hipStream_t st);
// launch_calibrate_eval on the members' mean row (one row per point), plus stats and votes
int launch_ensemble_eval(const float* logits, int M, int K, int Mn, size_t member_stride, const EnsembleCal& cal, const int32_t* y,
                         const int32_t* label_map, int n_labels, int32_t* est, float* score, int32_t* rank, float* p_true, float* stats,
                         int32_t* votes, long long* totals, long long* confusion, long long* rank_hist, hipStream_t st);
// patch i = view views[i] (masked to 4 bits) of point i (include/mmc.h, "patch views")
int launch_crop_views(const uint8_t* image, int H, int W, const int32_t* rowcols, const uint8_t* views, int n, uint8_t* out,
                      hipStream_t st);
// Patch views, the orientation half: output pixel (i, j) of view v is pixel (by, bx) of the base patch B, so that
// P = rot90(fliplr(B) if f else B, k = r) with r = v & 3, f = (v >> 2) & 1.  Shared by the kernel and the host cut.
__host__ __device__ inline void view_source(int v, int i, int j, int& by, int& bx)
{
    const int r = v & 3, f = (v >> 2) & 1;
    const int y = (r & 1) ? j : i, x = (r & 1) ? i : j;           // r odd transposes
    by = (r & 2) ? 223 - y : y;                                   // r = 2, 3 walk B's rows backwards
    bx = (f ^ ((r ^ (r >> 1)) & 1)) ? 223 - x : x;                // columns backwards for (r, f) in {(0,1), (1,0), (2,0), (3,1)}
}

// ---- grouped validation (metrics.hip) ----
constexpr int GROUP_MAX_BINS = 64;
constexpr int GROUP_MAX_TARGETS = 2 * GROUP_MAX_BINS;            // the sorted positions of every bin's first and last key
constexpr int GROUP_HIST_WORDS = GROUP_MAX_TARGETS * 1024;       // counters of one radix-select level: slots x 2^10 (level 1: 1 x 2^11)
constexpr uint32_t GROUP_KEY_NONE = 0xFFFFFFFFu;                 // the reliability key of a row that is not scored
constexpr int GROUP_MAX_CATEGORIES = 64;                         // categories of mmc_head_evaluate_categories (ids fit the category byte)
constexpr uint8_t GROUP_SEG_NONE = 0xFF;                         // the category byte of a row that enters no category table
// the bins of a category of n rows: n_bins_cat = min(20, max(2, n // 10)) (mermaid_classifier/pyspacer/metrics/calibration.py:137)
#define GROUP_CAT_BINS_MAX 20
#define GROUP_CAT_BINS_MIN 2
#define GROUP_CAT_ROWS_PER_BIN 10
struct GroupSelect {   // device state of the radix select; after launch_group_select: tgt_prefix = the keys at the targets' sorted
                       // positions, slot_prefix[0 .. n_slots) = the distinct ones among them, ascending
    uint32_t n_scored, n_targets, n_slots, pad;
    uint32_t tgt_prefix[GROUP_MAX_TARGETS], tgt_rank[GROUP_MAX_TARGETS], tgt_slot[GROUP_MAX_TARGETS], slot_prefix[GROUP_MAX_TARGETS];
};
struct GroupRowsArgs {
    const int32_t* scored; const int32_t* est; const float* score; const float* p_true;   // one chunk: launch_calibrate_eval's outputs
    int rows; int K; int64_t row0;                       // the chunk holds rows [row0, row0 + rows) of the call
    const int64_t* offsets; int64_t n_images;            // [n_images + 1], offsets[0] = 0 < ... < offsets[n_images] = rows of the call
    const int32_t* source_of_image;                      // [n_images] in [0, sources), or NULL
    int32_t* true_cnt; int32_t* pred_cnt; int32_t* points;   // [n_images][K] x 2, [n_images]
    unsigned long long* cls_tab;                         // [3][K]: support, nll_q32, score_q32 per true class
    unsigned long long* source_conf;                     // [sources][K][K], or NULL
    uint32_t* keys;                                      // [rows of the call]
    const int32_t* category_of_class;                    // [K] in [-1, categories), or NULL: no category bytes
    uint8_t* seg;                                        // [rows of the call]: the category of the row's true class, GROUP_SEG_NONE for an
                                                         // unscored row or a class without a category; NULL without category_of_class
};
// one chunk's scored rows into the integer tables (the caller zeroes them once per call) and its reliability keys
int launch_group_rows(const GroupRowsArgs& a, hipStream_t st);
// the image chunking of the cover reduction (a function of n_images alone); slab of launch_group_cover: chunks x K x 8 doubles
void group_cover_chunks(int64_t n_images, int64_t* per_chunk, int* chunks);
// cov[K][8] = sum t, sum p, sum (p - t), sum (p - t)^2, sum |p - t|, min t, max t, sum (t - mean t)^2 over the images with points > 0
// (t = true_cnt / points, p = pred_cnt / points, fp64, fixed order); *n_used = the number of such images
int launch_group_cover(const int32_t* true_cnt, const int32_t* pred_cnt, const int32_t* points, int64_t n_images, int K, double* slab,
                       double* cov, long long* n_used, hipStream_t st);
// radix select of the bin-edge keys among keys[n] (n_scored = totals[0] - totals[2] - totals[3], read on the device), then
// raw[4][GROUP_MAX_TARGETS]: per distinct edge key e_j the rows equal to it, and count / n_correct / conf_q32 of e_j < key < e_j+1.
// hist: GROUP_HIST_WORDS counters of scratch
int launch_group_select(const uint32_t* keys, int64_t n, const long long* totals, int n_bins, GroupSelect* sel, uint32_t* hist,
                        unsigned long long* raw, hipStream_t st);
// cat_rows[c] = sum of support[k] over the classes with category_of_class[k] == c, cat_bins[c] = its bin count (0 without a row), for
// c < n_categories <= GROUP_MAX_CATEGORIES; both on the device
int launch_group_category_counts(const unsigned long long* support, const int32_t* category_of_class, int K, int n_categories,
                                 long long* cat_rows, int32_t* cat_bins, hipStream_t st);
// launch_group_select over the rows of category c alone: ckeys[r] = seg[r] == c ? keys[r] : GROUP_KEY_NONE (n entries of scratch), the
// targets seeded from cat_rows[c] / cat_bins[c] on the device, then the same select and binned sums into this category's sel / raw
int launch_group_select_category(const uint32_t* keys, const uint8_t* seg, int64_t n, int c, const long long* cat_rows, const int32_t* cat_bins,
                                 uint32_t* ckeys, GroupSelect* sel, uint32_t* hist, unsigned long long* raw, hipStream_t st);

// ---- cover estimation (cover.hip; include/mmc.h "cover estimation") ----
// P: the resident n x K fp32 probabilities; offsets [n_groups + 1]: offsets[0] = 0 <= ... <= offsets[n_groups] = n (device).
constexpr int COVER_SLAB_POINTS = 64;   // points per slab of the E-step: one wave walks one slab
// count / soft [n_groups][K], unusable [n_groups]: int64 tables the caller zeroes; integer atomics only
int launch_cover_count(const float* P, int64_t n, int K, const int64_t* offsets, int64_t n_groups, unsigned long long* count,
                       unsigned long long* soft, unsigned long long* unusable, hipStream_t st);
// pi = train_prior and w = pi / train_prior for every group (pi, w: [n_groups][K] doubles)
int launch_cover_em_init(const double* train_prior, int64_t n_groups, int K, double* pi, double* w, hipStream_t st);
// the E-step: slab s = rows [slab_row0[s], min(slab_row0[s] + COVER_SLAB_POINTS, offsets[slab_group[s] + 1])) of group slab_group[s];
// part [n_slabs][K]: the slab's sum of posteriors under w
int launch_cover_em_pass(const float* P, int K, const int64_t* slab_row0, const int32_t* slab_group, const int64_t* offsets, int64_t n_slabs,
                         const double* w, double* part, hipStream_t st);
// the M-step: group g owns slabs [group_slab0[g], group_slab0[g + 1]); unusable: launch_cover_count's; writes pi and w
int launch_cover_em_reduce(const double* part, const int64_t* group_slab0, const int64_t* offsets, const unsigned long long* unusable,
                           const double* train_prior, double strength, int64_t n_groups, int K, double* pi, double* w, hipStream_t st);
// per point the k best classes of the posterior under w, chosen as launch_calibrate_topk chooses them; idx / scores: n x k
int launch_cover_adapt_topk(const float* P, int64_t n, int K, const int64_t* offsets, int64_t n_groups, const double* w, int k, int32_t* idx,
                            float* scores, hipStream_t st);
