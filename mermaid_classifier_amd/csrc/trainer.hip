// trainer.hip -- mini-batch Adam training of the MLP classifier on precomputed feature vectors (gfx950).
//
// Replaces the arithmetic of TorchMLPClassifier.partial_fit (reference
// mermaid_classifier/pyspacer/torch_classifier.py:226-303: per mini-batch zero_grad -> logits -> weighted
// cross-entropy (mean over sum of weights) + (0.5*alpha/mb) * sum(W^2) -> backward -> torch.optim.Adam.step), as driven
// by the trainer's batch loop (mermaid_classifier/pyspacer/trainer.py:138-145).  fp32 end to end on the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32); every reduction runs in a fixed order (no atomics), so a run is bit-reproducible.
//
// One step on a resident mini-batch H0 [mb][d0]:
//   forward   H(l+1) = relu(H(l) W(l)^T + b(l)), logits = H(L) without relu           tgemm_f32_kernel<TA=0,TB=1>, EPI_BIAS(_RELU)
//   loss      per-row weighted CE, dZ(L) = w(y)/sum_w * (softmax - onehot)             ce_grad_kernel, ce_grad_rows<false>
//             or, per trainer: label smoothing, focal modulation, logit prior          ce_grad_kernel, ce_grad_rows<true>  (mmc_trainer_set_loss)
//   backward  dW(l) = dZ(l+1)^T H(l) + (alpha/mb) W(l)                                 tgemm_f32_kernel<TA=1,TB=0>, EPI_L2
//             db(l) = column sums of dZ(l+1)                                           colsum_kernel
//             dZ(l) = (dZ(l+1) W(l)) * (H(l) > 0)                                      tgemm_f32_kernel<TA=0,TB=0>, EPI_MASK
//   update    Adam exactly in torch's order of operations (lerp, addcmul, addcdiv)     adam_kernel
// Per trainer, off by default (include/mmc.h, "regularisers"; with everything off a step is the launches above and nothing else):
//   dropout   H(l+1) = mask(relu(...)) * 1/(1-p), counter-based Philox masks (philox.h) tgemm_f32_drop_kernel, EPI_BIAS_RELU_DROP
//             dZ(l) = (dZ(l+1) W(l)) * 1/(1-p) * (H(l) > 0): a dropped H is a stored +0  tgemm_f32_mask_scale_kernel, EPI_MASK_SCALE
//             the input's mask on the staged mini-batch, in place                        dropout_rows_kernel
//   mixup     x = lam Xa + oml Xb while the rows of a resident pass are gathered         gather_set_rows_mixed_kernel
//             l = lam l(z, ya) + oml l(z, yb): one softmax, two targets                  ce_grad_mixed_kernel, ce_grad_rows_mixed
// Per trainer, off by default (include/mmc.h, "optimiser options"; a member with none of them runs adam_kernel as ever):
//   schedule  lr_s = lr w(s) d(s) in double on the host, step_size = (float)(lr_s / bc1)  mmc_lr_schedule_at
//   clipping  norm over every gW(l), gb(l); coef = fminf(1, max_norm / (norm + 1e-6))     sumsq_kernel, gnorm_finalize_kernel
//   update    Adam on g * coef, then the shadow s = s + om_d (p - s)                      adam_opt_kernel
// Per pass, off by default (include/mmc.h, "group-robust training"; a member without either array runs ce_grad_kernel as ever):
//   weights   the row's normaliser is s_i = r_i / sum of the masses r_i w(y_i), one rounded product ce_grad_weighted_kernel, ce_grad_rows<., true>
//   group DRO q over the rows' groups moves by exp(eta L_a) per step on the device                 dro_update_kernel
//             dZ(L) and the row losses take c_i = q_a / V_a                                        row_scale_kernel
// Per trainer, off by default (include/mmc.h, "taxonomy-aware loss"; a member without a hierarchy runs the loss kernels above as ever):
//   levels    l_i += w_t sum_l lam_l (-log P_l), P_l the softmax mass of t's node at level l    ce_grad_hier_kernel, ce_grad_rows_hier
//   soft      the base term becomes w_t (-sum_c T[t,c] logp_c); row weights ride the same kernel (mmc_trainer_set_hierarchy)
// Per trainer, off by default (include/mmc.h, "batch normalisation"; a member without it launches none of these and keeps its colsum):
//   forward   Z = H(l) W(l)^T + b(l) by the forward GEMM (EPI_BIAS) to a buffer of its own, then
//             H(l+1) = relu(gamma xhat + beta), xhat = (Z - mu) rstd; the running statistics    bn_forward_kernel
//   backward  dZ(l) holds dA after the masked launch: g_gamma, g_beta, dZ in place              bn_backward_kernel
//   update    gamma, beta of every hidden layer in one more Adam launch; b(l) frozen            adam_kernel / adam_opt_kernel
//   eval      W' = s W, b' = beta + s (b - rm), s = gamma / sqrt(rv + eps), lazily              bn_fold_kernel
//
// Every step is the step of a group of trainers (trainer_group_step): each kind of launch once, one member per blockIdx.z, the
// member's operands in a by-value descriptor array.  A trainer on its own -- the host-fed pass, mmc_trainer_partial_fit_set, the
// eval-mode forward, mmc_trainer_loss_gradient -- is a group of one, so there is one compiled copy of every kernel body and a
// member of a sweep computes the bits it computes alone because it runs the same code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/mmc.h"
#include "kernels.h"
#include "philox.h"
#include "trainer_internal.h"

namespace {

// TEPI_BIAS_RELU_DROP and TEPI_MASK_SCALE are the two epilogues of a member with hidden dropout (mmc_trainer_set_dropout)
enum { TEPI_NONE = 0, TEPI_BIAS_RELU = 1, TEPI_BIAS = 2, TEPI_MASK = 3, TEPI_L2 = 4, TEPI_BIAS_RELU_DROP = 5, TEPI_MASK_SCALE = 6 };

// C[M][N] = op(A)[M][K] . op(B)[K][N] (+ epilogue).  TA: A is stored [K][M]; TB: B is stored [N][K].
// 64x64 output tile per 256-thread workgroup, K in steps of 16 through LDS (k-major tiles, so every transpose flavour is
// index arithmetic at staging time); wave w owns the 32x32 quadrant (w>>1, w&1) as 2x2 MFMA fragments.
//
// Every kernel of a step is a __device__ body with one __global__ caller, which picks its member's descriptor by blockIdx.z.
// LDS is declared by the kernel and handed in, so a kernel that switches between two epilogues holds one pair of tiles.
// Which multiply-add pairs are fused is part of the arithmetic, and the compiler does not decide it alike for every caller of a body
// (left alone it once fused v * beta2 + ... of adam_elems in one of two callers only).  So the bodies compile with contraction off
// and spell out the fusions these kernels have always had: fmaf where they fuse, plain operators where they round twice.
// VARIANT tags the instantiations of the kernels that exist for dropout alone (1; everything else 0).  hipcc emits other address
// arithmetic for a body that two kernels share, so without the tag adding those kernels would change the code of the kernels a pass
// without dropout launches; with it their assembly is what it was before dropout existed.  The arithmetic on values is the same
// source under either tag, so a member computes the same bits whichever kernel runs it.
template <bool TA, bool TB, int EPI, int VARIANT = 0>
__device__ __forceinline__ void tgemm_f32_tile(float (&As)[16][68], float (&Bs)[16][68], int tile_m, int tile_n,
                                               const float* __restrict__ A, const float* __restrict__ B,
                                               float* __restrict__ C, int M, int N, int K,
                                               const float* __restrict__ aux,   // bias[N] | mask[M][N] | W[M][N]
                                               float scale,                     // EPI_L2: alpha / mb; EPI_MASK_SCALE: 1 / (1 - p)
                                               DropMask drop = DropMask{})      // EPI_BIAS_RELU_DROP alone reads it
{
#pragma clang fp contract(off)   // the one fused operation (EPI_L2) is written as fmaf
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = tile_m * 64, n0 = tile_n * 64;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int li = lane & 15, lq = lane >> 4;
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 16) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + 256 * r;
            {
                const int m = TA ? (idx & 63) : (idx >> 4), k = TA ? (idx >> 6) : (idx & 15);
                const int gm = m0 + m, gk = k0 + k;
                float v = 0.f;
                if (gm < M && gk < K) v = TA ? A[(size_t)gk * M + gm] : A[(size_t)gm * K + gk];
                As[k][m] = v;
            }
            {
                const int n = TB ? (idx >> 4) : (idx & 63), k = TB ? (idx & 15) : (idx >> 6);
                const int gn = n0 + n, gk = k0 + k;
                float v = 0.f;
                if (gn < N && gk < K) v = TB ? B[(size_t)gn * K + gk] : B[(size_t)gk * N + gn];
                Bs[k][n] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; kk += 4) {
            float av[2], bv[2];
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                av[f] = As[kk + lq][wm + f * 16 + li];
                bv[f] = Bs[kk + lq][wn + f * 16 + li];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }
    // lane (li, lq) holds C[m0 + wm + 16a + 4 lq + r][n0 + wn + 16b + li]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + 16 * a + 4 * lq + r, n = n0 + wn + 16 * b + li;
                if (m >= M || n >= N) continue;
                float v = acc[a][b][r];
                if (EPI == TEPI_BIAS_RELU) v = fmaxf(v + aux[n], 0.f);
                if (EPI == TEPI_BIAS) v = v + aux[n];
                if (EPI == TEPI_MASK) v = aux[(size_t)m * N + n] > 0.f ? v : 0.f;
                // a dropped activation was stored as +0, so H > 0 is "alive and kept": no stored mask, no second draw
                if (EPI == TEPI_MASK_SCALE) v = aux[(size_t)m * N + n] > 0.f ? v * scale : 0.f;
                if (EPI == TEPI_BIAS_RELU_DROP) {
                    v = fmaxf(v + aux[n], 0.f);
                    v = dropout_keep(drop, (uint64_t)m * (uint64_t)N + (uint64_t)n) ? v * drop.scale : 0.f;
                }
                if (EPI == TEPI_L2) v = fmaf(scale, aux[(size_t)m * N + n], v);
                C[(size_t)m * N + n] = v;
            }
}

// ---- the kernels: one member per blockIdx.z; the grid is the largest member's and a workgroup outside its own member's extent
// leaves before its first barrier (the test reads kernel arguments and block indices only: block-uniform).
struct GemmDesc {
    const float *A, *B;
    float* C;
    const float* aux;
    int M, N, K, epi;
    float scale;
};
struct GemmGroup { GemmDesc d[MMC_TRAINER_GROUP_MAX]; };
// the forward launch of a layer in which at least one member drops: the members' mask parameters beside their descriptors
struct GemmDropGroup {
    GemmDesc d[MMC_TRAINER_GROUP_MAX];
    DropMask r[MMC_TRAINER_GROUP_MAX];
};
// by-value kernel arguments: every group struct of this file has to stay within the 4 KB the runtime passes
static_assert(sizeof(GemmGroup) <= 4096 && sizeof(GemmDropGroup) <= 4096, "kernel-argument limit");

// EPI0 / EPI1: the epilogues the members of one launch can have (forward: hidden layer or a member's last; otherwise one kind)
template <bool TA, bool TB, int EPI0, int EPI1>
__global__ __launch_bounds__(256) void tgemm_f32_kernel(const GemmGroup g)
{
    __shared__ float As[16][68];
    __shared__ float Bs[16][68];
    const GemmDesc& d = g.d[blockIdx.z];
    if ((int)blockIdx.x * 64 >= d.M || (int)blockIdx.y * 64 >= d.N) return;
    if (EPI0 == EPI1 || d.epi == EPI0)
        tgemm_f32_tile<TA, TB, EPI0>(As, Bs, blockIdx.x, blockIdx.y, d.A, d.B, d.C, d.M, d.N, d.K, d.aux, d.scale);
    else
        tgemm_f32_tile<TA, TB, EPI1>(As, Bs, blockIdx.x, blockIdx.y, d.A, d.B, d.C, d.M, d.N, d.K, d.aux, d.scale);
}

// The forward of a layer when a member of the launch drops its hidden activations: the two epilogues above and the dropping one.
// Launched only then, so a pass without dropout runs tgemm_f32_kernel alone.
__global__ __launch_bounds__(256) void tgemm_f32_drop_kernel(const GemmDropGroup g)
{
    __shared__ float As[16][68];
    __shared__ float Bs[16][68];
    const GemmDesc& d = g.d[blockIdx.z];
    if ((int)blockIdx.x * 64 >= d.M || (int)blockIdx.y * 64 >= d.N) return;
    const DropMask& r = g.r[blockIdx.z];
    if (d.epi == TEPI_BIAS_RELU_DROP)
        tgemm_f32_tile<false, true, TEPI_BIAS_RELU_DROP, 1>(As, Bs, blockIdx.x, blockIdx.y, d.A, d.B, d.C, d.M, d.N, d.K, d.aux, d.scale, r);
    else if (d.epi == TEPI_BIAS_RELU)
        tgemm_f32_tile<false, true, TEPI_BIAS_RELU, 1>(As, Bs, blockIdx.x, blockIdx.y, d.A, d.B, d.C, d.M, d.N, d.K, d.aux, d.scale, r);
    else
        tgemm_f32_tile<false, true, TEPI_BIAS, 1>(As, Bs, blockIdx.x, blockIdx.y, d.A, d.B, d.C, d.M, d.N, d.K, d.aux, d.scale, r);
}

// The dZ launch of a layer when a member of it dropped that layer's input in the forward: EPI_MASK for the others, the scaled mask
// for the dropping ones.
__global__ __launch_bounds__(256) void tgemm_f32_mask_scale_kernel(const GemmGroup g)
{
    __shared__ float As[16][68];
    __shared__ float Bs[16][68];
    const GemmDesc& d = g.d[blockIdx.z];
    if ((int)blockIdx.x * 64 >= d.M || (int)blockIdx.y * 64 >= d.N) return;
    if (d.epi == TEPI_MASK_SCALE)
        tgemm_f32_tile<false, false, TEPI_MASK_SCALE, 1>(As, Bs, blockIdx.x, blockIdx.y, d.A, d.B, d.C, d.M, d.N, d.K, d.aux, d.scale);
    else
        tgemm_f32_tile<false, false, TEPI_MASK, 1>(As, Bs, blockIdx.x, blockIdx.y, d.A, d.B, d.C, d.M, d.N, d.K, d.aux, d.scale);
}

// Input dropout: X[m][n] of the member's mini-batch becomes X * scale or +0 by the mask of site 0, in place in the trainer's own
// staging (a copy of the caller's or the set's rows, read by this step alone).  Grid-stride; the mask does not depend on the grid.
struct DropRowsDesc {
    float* X;
    int M, N;
    DropMask mask;
};
struct DropRowsGroup { DropRowsDesc d[MMC_TRAINER_GROUP_MAX]; };
static_assert(sizeof(DropRowsGroup) <= 4096, "kernel-argument limit");

__global__ __launch_bounds__(256) void dropout_rows_kernel(const DropRowsGroup g)
{
#pragma clang fp contract(off)
    const DropRowsDesc& d = g.d[blockIdx.z];
    const size_t total = (size_t)d.M * (size_t)d.N;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256)
        d.X[e] = dropout_keep(d.mask, (uint64_t)e) ? d.X[e] * d.mask.scale : 0.f;
}

// The loss formulation of a trainer (mmc_trainer_set_loss): the fp32 scalars of the general instantiation below, made from doubles
// on the host as the other hyper-parameters are.  All defaults (no smoothing, no focusing, no prior) select the plain instantiation.
struct CeLoss {
    const float* prior;   // [K] offset added to the logits inside the loss only, or null
    float om_eps;         // (float)(1.0 - label_smoothing)
    float eps_k;          // (float)(label_smoothing / K)
    float gamma;          // (float)focal_gamma: 0 or in [1, 8]
    float w_total;        // sum of the class weights (K without class weights)
};

// a per-lane partial over the whole wave, the same value in every lane (commutative butterfly: a fixed order, no atomics)
__device__ __forceinline__ float wave_sum(float v)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One wave per row: log-softmax, weighted negative log-likelihood, gradient of the weighted-mean loss w.r.t. the logits.
// GENERAL = false: F.cross_entropy(logits, y, weight=w) = sum_i w[y_i] * nll_i / sum_i w[y_i]   (torch_classifier.py:278)
// GENERAL = true:  label smoothing, focal modulation and a logit prior (include/mmc.h, mmc_trainer_set_loss); with u = z + prior,
//   t = y_i, p = softmax(u), q = 1 - p_t taken as sum_{c != t} e_c / sum_c e_c (no cancellation), pw = q^(gamma-1), m = pw q:
//   l_i      = om_eps w_t m nll + eps_k sum_c w_c (-logp_c)
//   dl_i/dz_c = om_eps w_t f (p_c - [c == t]) + eps_k (p_c w_total - w_c),   f = m + gamma p_t pw nll   (gamma = 0: m = f = 1)
//   The two extra row sums are lane-strided sums and the butterfly of the softmax denominator.  Everything is finite on a finite
//   row: q = 0 (p_t rounds to 1) gives m = 0 and pw in {0, 1}; p_t = 0 leaves f = m.
// ROWS (ce_grad_weighted_kernel alone): the row's normaliser is s_i = rw[row] * inv_wsum, one rounded product, wherever the others
//   read inv_wsum (include/mmc.h, "group-robust training"); rw null: inv_wsum itself.
template <bool GENERAL, bool ROWS = false>
__device__ __forceinline__ void ce_grad_rows(int block, const float* __restrict__ logits, const int32_t* __restrict__ y, int M, int K,
                                             const float* __restrict__ cw,   // [K] or null
                                             float inv_wsum, float* __restrict__ dlogits, float* __restrict__ row_loss, const CeLoss& ls,
                                             const float* __restrict__ rw = nullptr)
{
#pragma clang fp contract(off)   // nothing here has ever been fused
    const int lane = threadIdx.x & 63;
    const int row = block * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    if (ROWS && rw) inv_wsum = rw[row] * inv_wsum;
    const float* z = logits + (size_t)row * K;
    if (GENERAL) {
        const float* pr = ls.prior;
        const int yi = y[row];
        float mx = -INFINITY;
        for (int c = lane; c < K; c += 64) mx = fmaxf(mx, pr ? z[c] + pr[c] : z[c]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        float s = 0.f, so = 0.f;   // sum_c e_c; sum_{c != t} e_c
        for (int c = lane; c < K; c += 64) {
            const float e = expf((pr ? z[c] + pr[c] : z[c]) - mx);
            s += e;
            so += c == yi ? 0.f : e;
        }
        s = wave_sum(s);
        so = wave_sum(so);
        const float w = cw ? cw[yi] : 1.0f;
        const float lse = logf(s);
        const bool smooth = ls.eps_k != 0.f;
        float sw = 0.f;            // sum_c w_c logp_c
        if (smooth) {
            for (int c = lane; c < K; c += 64) {
                const float lp = (pr ? z[c] + pr[c] : z[c]) - mx - lse;
                sw += cw ? cw[c] * lp : lp;
            }
            sw = wave_sum(sw);
        }
        const float ut = pr ? z[yi] + pr[yi] : z[yi];
        const float nll = lse - (ut - mx);
        float m = 1.0f, f = 1.0f;
        if (ls.gamma != 0.f) {
            const float q = so / s;
            const float pt = expf(ut - mx - lse);
            const float pw = powf(q, ls.gamma - 1.0f);
            m = pw * q;
            f = m + ls.gamma * pt * pw * nll;
        }
        const float a = ls.om_eps * w;
        const float af = a * f;
        for (int c = lane; c < K; c += 64) {
            const float p = expf((pr ? z[c] + pr[c] : z[c]) - mx - lse);
            float d = af * (p - (c == yi ? 1.0f : 0.0f));
            if (smooth) d = d + ls.eps_k * (p * ls.w_total - (cw ? cw[c] : 1.0f));
            dlogits[(size_t)row * K + c] = inv_wsum * d;
        }
        if (lane == 0) {
            float l = a * m * nll;
            if (smooth) l = l - ls.eps_k * sw;
            row_loss[row] = l * inv_wsum;
        }
        return;
    }
    float mx = -INFINITY;
    for (int c = lane; c < K; c += 64) mx = fmaxf(mx, z[c]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float s = 0.f;
    for (int c = lane; c < K; c += 64) s += expf(z[c] - mx);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    const int yi = y[row];
    const float w = cw ? cw[yi] : 1.0f;
    const float lse = logf(s);
    const float g = w * inv_wsum;
    for (int c = lane; c < K; c += 64) {
        const float p = expf(z[c] - mx - lse);
        dlogits[(size_t)row * K + c] = g * (p - (c == yi ? 1.0f : 0.0f));
    }
    if (lane == 0) row_loss[row] = w * (lse - (z[yi] - mx)) * inv_wsum;
}

struct CeDesc {
    const float* logits;
    const int32_t* y;
    const float* cw;
    float *dlogits, *row_loss;
    int M, K;
    float inv_wsum;
    int general;   // which instantiation this member runs: a group may mix plain and general members
    CeLoss loss;
};
struct CeGroup { CeDesc d[MMC_TRAINER_GROUP_MAX]; };

__global__ __launch_bounds__(256) void ce_grad_kernel(const CeGroup g)
{
    const CeDesc& d = g.d[blockIdx.z];
    if ((int)blockIdx.x * 4 >= d.M) return;
    if (d.general)
        ce_grad_rows<true>(blockIdx.x, d.logits, d.y, d.M, d.K, d.cw, d.inv_wsum, d.dlogits, d.row_loss, d.loss);
    else
        ce_grad_rows<false>(blockIdx.x, d.logits, d.y, d.M, d.K, d.cw, d.inv_wsum, d.dlogits, d.row_loss, d.loss);
}

// The loss stage of a mixed row (mmc_trainer_partial_fit_set_mixed): one softmax, two targets a = y[row], b = y2[row].
//   l_i = lam l(z, a) + oml l(z, b),   dl_i/dz = lam dl(a)/dz + oml dl(b)/dz,   oml = 1.0f - lam
// with l the row term of ce_grad_rows above -- the general form, which at eps = gamma = 0 and no prior is the plain weighted CE.
// Each target's term is formed as ce_grad_rows<true> forms it; the combination is two rounded products and one rounded add.
__device__ __forceinline__ void ce_grad_rows_mixed(int block, const float* __restrict__ logits, const int32_t* __restrict__ y,
                                                   const int32_t* __restrict__ y2, int M, int K, const float* __restrict__ cw,
                                                   float inv_wsum, float lam, float oml, float* __restrict__ dlogits,
                                                   float* __restrict__ row_loss, const CeLoss& ls)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int row = block * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* z = logits + (size_t)row * K;
    const float* pr = ls.prior;
    const int ya = y[row], yb = y2[row];
    float mx = -INFINITY;
    for (int c = lane; c < K; c += 64) mx = fmaxf(mx, pr ? z[c] + pr[c] : z[c]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float s = 0.f, soa = 0.f, sob = 0.f;   // sum_c e_c; sum_{c != a} e_c; sum_{c != b} e_c
    for (int c = lane; c < K; c += 64) {
        const float e = expf((pr ? z[c] + pr[c] : z[c]) - mx);
        s += e;
        soa += c == ya ? 0.f : e;
        sob += c == yb ? 0.f : e;
    }
    s = wave_sum(s);
    soa = wave_sum(soa);
    sob = wave_sum(sob);
    const float lse = logf(s);
    const bool smooth = ls.eps_k != 0.f;
    float sw = 0.f;                        // sum_c w_c logp_c
    if (smooth) {
        for (int c = lane; c < K; c += 64) {
            const float lp = (pr ? z[c] + pr[c] : z[c]) - mx - lse;
            sw += cw ? cw[c] * lp : lp;
        }
        sw = wave_sum(sw);
    }
    float a2[2], af2[2], l2[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int yi = k ? yb : ya;
        const float so = k ? sob : soa;
        const float w = cw ? cw[yi] : 1.0f;
        const float ut = pr ? z[yi] + pr[yi] : z[yi];
        const float nll = lse - (ut - mx);
        float m = 1.0f, f = 1.0f;
        if (ls.gamma != 0.f) {
            const float q = so / s;
            const float pt = expf(ut - mx - lse);
            const float pw = powf(q, ls.gamma - 1.0f);
            m = pw * q;
            f = m + ls.gamma * pt * pw * nll;
        }
        a2[k] = ls.om_eps * w;
        af2[k] = a2[k] * f;
        float l = a2[k] * m * nll;
        if (smooth) l = l - ls.eps_k * sw;
        l2[k] = l;
    }
    for (int c = lane; c < K; c += 64) {
        const float p = expf((pr ? z[c] + pr[c] : z[c]) - mx - lse);
        float da = af2[0] * (p - (c == ya ? 1.0f : 0.0f));
        float db = af2[1] * (p - (c == yb ? 1.0f : 0.0f));
        if (smooth) {
            const float sm = ls.eps_k * (p * ls.w_total - (cw ? cw[c] : 1.0f));
            da = da + sm;
            db = db + sm;
        }
        dlogits[(size_t)row * K + c] = inv_wsum * (lam * da + oml * db);
    }
    if (lane == 0) row_loss[row] = (lam * l2[0] + oml * l2[1]) * inv_wsum;
}

struct CeMixDesc {
    const float* logits;
    const int32_t *y, *y2;
    const float* cw;
    float *dlogits, *row_loss;
    int M, K;
    float inv_wsum, lam, oml;
    CeLoss loss;
};
struct CeMixGroup { CeMixDesc d[MMC_TRAINER_GROUP_MAX]; };
static_assert(sizeof(CeGroup) <= 4096 && sizeof(CeMixGroup) <= 4096, "kernel-argument limit");

// the mixed members of a step; the others go through ce_grad_kernel as ever
__global__ __launch_bounds__(256) void ce_grad_mixed_kernel(const CeMixGroup g)
{
    const CeMixDesc& d = g.d[blockIdx.z];
    if ((int)blockIdx.x * 4 >= d.M) return;
    ce_grad_rows_mixed(blockIdx.x, d.logits, d.y, d.y2, d.M, d.K, d.cw, d.inv_wsum, d.lam, d.oml, d.dlogits, d.row_loss, d.loss);
}

// ---- group-robust training (include/mmc.h): the loss stage of a member with per-row weights or group DRO.  The other members of
// the same step keep ce_grad_kernel / ce_grad_mixed_kernel.
struct CeRowDesc {
    CeDesc c;          // inv_wsum: g = (float)(1 / sum of the row masses), or 1.0f for a member with groups
    const float* rw;   // the weights of the mini-batch's positions, or null (all 1)
};
struct CeRowGroup { CeRowDesc d[MMC_TRAINER_GROUP_MAX]; };
static_assert(sizeof(CeRowGroup) <= 4096, "kernel-argument limit");

__global__ __launch_bounds__(256) void ce_grad_weighted_kernel(const CeRowGroup g)
{
    const CeRowDesc& d = g.d[blockIdx.z];
    if ((int)blockIdx.x * 4 >= d.c.M) return;
    if (d.c.general)
        ce_grad_rows<true, true>(blockIdx.x, d.c.logits, d.c.y, d.c.M, d.c.K, d.c.cw, d.c.inv_wsum, d.c.dlogits, d.c.row_loss, d.c.loss, d.rw);
    else
        ce_grad_rows<false, true>(blockIdx.x, d.c.logits, d.c.y, d.c.M, d.c.K, d.c.cw, d.c.inv_wsum, d.c.dlogits, d.c.row_loss, d.c.loss, d.rw);
}

// ---- taxonomy-aware loss (include/mmc.h): the loss stage of a member with a hierarchy (mmc_trainer_set_hierarchy), with or without
// row weights.  A body of its own: the members without a hierarchy keep ce_grad_kernel / ce_grad_weighted_kernel and their code.
struct HierLoss {
    const int32_t* level;   // [n_levels][K] node ids, negative = no node; null when n_levels == 0
    const float* T;         // [K][K] soft targets, or null
    int n_levels;
    float lam[MMC_HIER_MAX_LEVELS];
};

// One wave per row, classes lane-strided, every row reduction a lane-strided sum (or max) and the xor butterfly.
//   base   with T:    b = w_t (-sum_c T[t,c] logp_c),  db/dz_c = w_t (p_c sum_c' T[t,c'] - T[t,c]); row t of T is read coalesced
//          without T: the general form, operation for operation as ce_grad_rows<true> forms it
//   level  for every level l at which t has a node: m_l = max of u over the node, lS_l = logf(sum over the node of expf(u_c - m_l)),
//          the four levels' maxima in one loop and one round of butterflies, their sums in another (independent chains in flight);
//          h += lam_l ((mx + lse) - (m_l + lS_l));  the gradient loop adds lam_l (p_c - [c in node] expf((u_c - m_l) - lS_l))
//   row    l_i = (base + w_t h) s_i,  dl_i/dz_c = s_i (db_c + w_t hd_c),  s_i = rw ? rw[row] * inv_wsum : inv_wsum
// Finite on any finite row: the node holds t, so m_l is finite and its sum is at least 1; nothing divides.
__device__ __forceinline__ void ce_grad_rows_hier(int block, const float* __restrict__ logits, const int32_t* __restrict__ y, int M, int K,
                                                  const float* __restrict__ cw, float inv_wsum, float* __restrict__ dlogits,
                                                  float* __restrict__ row_loss, const CeLoss& ls, const HierLoss& hl,
                                                  const float* __restrict__ rw)
{
#pragma clang fp contract(off)   // nothing here is fused
    const int lane = threadIdx.x & 63;
    const int row = block * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    if (rw) inv_wsum = rw[row] * inv_wsum;
    const float* z = logits + (size_t)row * K;
    const float* pr = ls.prior;
    const int yi = y[row];
    float mx = -INFINITY;
    for (int c = lane; c < K; c += 64) mx = fmaxf(mx, pr ? z[c] + pr[c] : z[c]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float s = 0.f, so = 0.f;   // sum_c e_c; sum_{c != t} e_c
    for (int c = lane; c < K; c += 64) {
        const float e = expf((pr ? z[c] + pr[c] : z[c]) - mx);
        s += e;
        so += c == yi ? 0.f : e;
    }
    s = wave_sum(s);
    so = wave_sum(so);
    const float w = cw ? cw[yi] : 1.0f;
    const float lse = logf(s);
    const float* Tt = hl.T ? hl.T + (size_t)yi * K : nullptr;
    const bool smooth = ls.eps_k != 0.f;
    float st = 0.f, sl = 0.f;   // with T: sum_c T[t,c]; sum_c T[t,c] logp_c.  Without, sl: sum_c w_c logp_c of the smoothing term
    float a = 0.f, af = 0.f, lb;
    if (Tt) {
        for (int c = lane; c < K; c += 64) {
            const float lp = (pr ? z[c] + pr[c] : z[c]) - mx - lse;
            st += Tt[c];
            sl += Tt[c] * lp;
        }
        st = wave_sum(st);
        sl = wave_sum(sl);
        lb = -(w * sl);
    } else {
        if (smooth) {
            for (int c = lane; c < K; c += 64) {
                const float lp = (pr ? z[c] + pr[c] : z[c]) - mx - lse;
                sl += cw ? cw[c] * lp : lp;
            }
            sl = wave_sum(sl);
        }
        const float ut = pr ? z[yi] + pr[yi] : z[yi];
        const float nll = lse - (ut - mx);
        float m = 1.0f, f = 1.0f;
        if (ls.gamma != 0.f) {
            const float q = so / s;
            const float pt = expf(ut - mx - lse);
            const float pw = powf(q, ls.gamma - 1.0f);
            m = pw * q;
            f = m + ls.gamma * pt * pw * nll;
        }
        a = ls.om_eps * w;
        af = a * f;
        lb = a * m * nll;
        if (smooth) lb = lb - ls.eps_k * sl;
    }
    // the levels: the true node's id, its maximum and the log of its sum against that maximum; h = sum_l lam_l (-log P_l)
    const float top = mx + lse;
    int gt[MMC_HIER_MAX_LEVELS];
    float ml[MMC_HIER_MAX_LEVELS], lS[MMC_HIER_MAX_LEVELS];
    float h = 0.f;
    // the levels' reductions side by side: four independent butterflies in flight, each level's values formed as if it were alone.
    // A level without a node for t (gt < 0; past n_levels too) loads nothing and carries -inf / 0 through the butterflies, unread.
#pragma unroll
    for (int l = 0; l < MMC_HIER_MAX_LEVELS; ++l) {
        gt[l] = l < hl.n_levels ? hl.level[(size_t)l * K + yi] : -1;
        ml[l] = -INFINITY;
        lS[l] = 0.f;
    }
    for (int c = lane; c < K; c += 64) {
        const float u = pr ? z[c] + pr[c] : z[c];
#pragma unroll
        for (int l = 0; l < MMC_HIER_MAX_LEVELS; ++l)
            if (gt[l] >= 0 && hl.level[(size_t)l * K + c] == gt[l]) ml[l] = fmaxf(ml[l], u);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (int l = 0; l < MMC_HIER_MAX_LEVELS; ++l) ml[l] = fmaxf(ml[l], __shfl_xor(ml[l], o));
    for (int c = lane; c < K; c += 64) {
        const float u = pr ? z[c] + pr[c] : z[c];
#pragma unroll
        for (int l = 0; l < MMC_HIER_MAX_LEVELS; ++l)
            if (gt[l] >= 0) lS[l] += hl.level[(size_t)l * K + c] == gt[l] ? expf(u - ml[l]) : 0.f;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (int l = 0; l < MMC_HIER_MAX_LEVELS; ++l) lS[l] += __shfl_xor(lS[l], o);
#pragma unroll
    for (int l = 0; l < MMC_HIER_MAX_LEVELS; ++l)
        if (gt[l] >= 0) {
            lS[l] = logf(lS[l]);
            h = h + hl.lam[l] * (top - (ml[l] + lS[l]));
        }
    for (int c = lane; c < K; c += 64) {
        const float u = pr ? z[c] + pr[c] : z[c];
        const float p = expf(u - mx - lse);
        float d;
        if (Tt) {
            d = w * (p * st - Tt[c]);
        } else {
            d = af * (p - (c == yi ? 1.0f : 0.0f));
            if (smooth) d = d + ls.eps_k * (p * ls.w_total - (cw ? cw[c] : 1.0f));
        }
        float hd = 0.f;
#pragma unroll
        for (int l = 0; l < MMC_HIER_MAX_LEVELS; ++l)
            if (gt[l] >= 0) {
                const float pin = hl.level[(size_t)l * K + c] == gt[l] ? expf((u - ml[l]) - lS[l]) : 0.f;
                hd = hd + hl.lam[l] * (p - pin);
            }
        d = d + w * hd;
        dlogits[(size_t)row * K + c] = inv_wsum * d;
    }
    if (lane == 0) row_loss[row] = (lb + w * h) * inv_wsum;
}

struct CeHierDesc {
    CeDesc c;          // inv_wsum as in CeDesc, or as in CeRowDesc for a member with row weights or groups
    const float* rw;   // the weights of the mini-batch's positions, or null
    HierLoss h;
};
struct CeHierGroup { CeHierDesc d[MMC_TRAINER_GROUP_MAX]; };
static_assert(sizeof(CeHierGroup) <= 4096, "kernel-argument limit");

__global__ __launch_bounds__(256) void ce_grad_hier_kernel(const CeHierGroup g)
{
    const CeHierDesc& d = g.d[blockIdx.z];
    if ((int)blockIdx.x * 4 >= d.c.M) return;
    ce_grad_rows_hier(blockIdx.x, d.c.logits, d.c.y, d.c.M, d.c.K, d.c.cw, d.c.inv_wsum, d.c.dlogits, d.c.row_loss, d.c.loss, d.h, d.rw);
}

// The group DRO update of a member's step, one workgroup of 1024 threads: from R_i = row_loss[i] (normaliser r_i) and the groups
// a_i it forms S_a, moves and renormalises logq, and leaves every row's scale c_i = (float)(exp(logq_a) / V_a).  All in double.
//   S_a   thread = group: GW = ceil(G / 64) waves cover the groups once, so the 16 waves make NS = 16 / GW slices of rows.  The rows
//         go through LDS in tiles of kDroTile; slice s takes rows [s per, (s + 1) per) of each tile, per = ceil(tile rows / NS),
//         and adds R_i (or +0.0) to its group's register in position order, tile after tile; the slices' sums are added in slice
//         order.  The order is a function of M and G alone: no atomics, and nothing depends on who trains beside the member.
//   logq  logq_a += eta (S_a / V_a) where V_a > 0; lse = mx + log(sum_b exp(logq_b - mx)) with mx the maximum and the sum taken by
//         one thread in index order; logq_a -= lse.
// G <= 1024 = the workgroup, so per-group work is one thread each.  Latency-bound: G = 1024 scans every row in every wave and adds
// 1024 terms serially (profiles/group_dro.txt).
constexpr int kDroTile = 2048;
struct DroDesc {
    const float* row_loss;   // [M] R_i
    const int32_t* group;    // [M] a_i in [0, G) (checked on the host)
    const double* V;         // [G] mass of every group in this mini-batch
    double* logq;            // [G] in / out
    float* scale;            // [M] c_i
    double* group_loss;      // [G] L_a, NaN where V_a = 0; or null
    int M, G;
    double eta;
};
struct DroGroup { DroDesc d[MMC_TRAINER_GROUP_MAX]; };
static_assert(sizeof(DroGroup) <= 4096, "kernel-argument limit");

__global__ __launch_bounds__(1024) void dro_update_kernel(const DroGroup g)
{
#pragma clang fp contract(off)
    __shared__ double Rs[kDroTile];
    __shared__ int As[kDroTile];
    __shared__ double part[1024];
    __shared__ double lse_s;
    const DroDesc& d = g.d[blockIdx.z];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = d.G, M = d.M;
    const int GW = (G + 63) >> 6, NS = 16 / GW;
    const int slice = wave / GW, grp = (wave % GW) * 64 + lane;
    double acc = 0.0;
    for (int r0 = 0; r0 < M; r0 += kDroTile) {
        const int rows = M - r0 < kDroTile ? M - r0 : kDroTile;
        for (int i = tid; i < rows; i += 1024) {
            Rs[i] = (double)d.row_loss[r0 + i];
            As[i] = d.group[r0 + i];
        }
        __syncthreads();
        if (slice < NS) {
            const int per = (rows + NS - 1) / NS;
            const int b = slice * per, e = b + per < rows ? b + per : rows;
            int i = b;
            for (; i + 4 <= e; i += 4) {   // four rows' loads in flight; the adds stay in position order
                const int a0 = As[i], a1 = As[i + 1], a2 = As[i + 2], a3 = As[i + 3];
                const double r0 = Rs[i], r1 = Rs[i + 1], r2 = Rs[i + 2], r3 = Rs[i + 3];
                acc += a0 == grp ? r0 : 0.0;
                acc += a1 == grp ? r1 : 0.0;
                acc += a2 == grp ? r2 : 0.0;
                acc += a3 == grp ? r3 : 0.0;
            }
            for (; i < e; ++i) {
                const double r0 = Rs[i];
                acc += As[i] == grp ? r0 : 0.0;
            }
        }
        __syncthreads();
    }
    if (slice < NS && grp < G) part[slice * G + grp] = acc;   // NS G <= (16 / GW) (64 GW) = 1024
    __syncthreads();
    double lqa = 0.0, Va = 0.0;
    if (tid < G) {
        double S = 0.0;
        for (int s = 0; s < NS; ++s) S += part[s * G + tid];
        Va = d.V[tid];
        lqa = d.logq[tid];
        double L = __builtin_nan("");
        if (Va > 0.0) {
            L = S / Va;
            lqa = lqa + d.eta * L;
        }
        if (d.group_loss) d.group_loss[tid] = L;
    }
    __syncthreads();
    part[tid] = tid < G ? lqa : -INFINITY;
    __syncthreads();
    for (int o = 512; o >= 1; o >>= 1) {
        if (tid < o) part[tid] = fmax(part[tid], part[tid + o]);
        __syncthreads();
    }
    const double mx = part[0];
    __syncthreads();
    part[tid] = tid < G ? exp(lqa - mx) : 0.0;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
#pragma unroll 16
        for (int b = 0; b < G; ++b) s += part[b];
        lse_s = mx + log(s);
    }
    __syncthreads();
    if (tid < G) {
        lqa = lqa - lse_s;
        d.logq[tid] = lqa;
        part[tid] = Va > 0.0 ? exp(lqa) / Va : 0.0;
    }
    __syncthreads();
    for (int i = tid; i < M; i += 1024) d.scale[i] = (float)part[d.group[i]];
}

// dlogits[i][:] = c_i dlogits[i][:], row_loss[i] = c_i row_loss[i]: one rounded fp32 product per element.  One wave per row.
struct RowScaleDesc {
    float *dlogits, *row_loss;
    const float* scale;
    int M, K;
};
struct RowScaleGroup { RowScaleDesc d[MMC_TRAINER_GROUP_MAX]; };
static_assert(sizeof(RowScaleGroup) <= 4096, "kernel-argument limit");

__global__ __launch_bounds__(256) void row_scale_kernel(const RowScaleGroup g)
{
#pragma clang fp contract(off)
    const RowScaleDesc& d = g.d[blockIdx.z];
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= d.M) return;
    const float c = d.scale[row];
    float* z = d.dlogits + (size_t)row * d.K;
    for (int k = lane; k < d.K; k += 64) z[k] = c * z[k];
    if (lane == 0) d.row_loss[row] = c * d.row_loss[row];
}

// db[n] = sum_m dZ[m][n]; thread per column, rows in order (four chains)
__device__ __forceinline__ void colsum_cols(int block, const float* __restrict__ dZ, int M, int N, float* __restrict__ db)
{
    const int n = block * 256 + threadIdx.x;
    if (n >= N) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int m = 0;
    for (; m + 3 < M; m += 4) {
        s0 += dZ[(size_t)m * N + n];
        s1 += dZ[(size_t)(m + 1) * N + n];
        s2 += dZ[(size_t)(m + 2) * N + n];
        s3 += dZ[(size_t)(m + 3) * N + n];
    }
    for (; m < M; ++m) s0 += dZ[(size_t)m * N + n];
    db[n] = (s0 + s1) + (s2 + s3);
}

struct ColsumDesc {
    const float* dZ;
    float* db;
    int M, N;
};
struct ColsumGroup { ColsumDesc d[MMC_TRAINER_GROUP_MAX]; };
static_assert(sizeof(ColsumGroup) <= 4096, "kernel-argument limit");

__global__ __launch_bounds__(256) void colsum_kernel(const ColsumGroup g)
{
    const ColsumDesc& d = g.d[blockIdx.z];
    if ((int)blockIdx.x * 256 >= d.N) return;
    colsum_cols(blockIdx.x, d.dZ, d.M, d.N, d.db);
}

// partial[blockIdx.x] = sum of x[i]^2 over this block's grid-stride slice (fixed order: per-thread chain, then LDS tree)
__device__ __forceinline__ void sumsq_slice(float (&red)[256], const float* __restrict__ x, size_t n, float* __restrict__ partial)
{
#pragma clang fp contract(off)
    float s = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) s = fmaf(x[i], x[i], s);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

struct SumsqDesc {
    const float* x;
    float* partial;
    size_t n;
};
struct SumsqGroup { SumsqDesc d[MMC_TRAINER_GROUP_MAX]; };
static_assert(sizeof(SumsqGroup) <= 4096, "kernel-argument limit");

// gridDim.x is 256 blocks whatever the group, so a member's slices and partials do not depend on who trains beside it
__global__ __launch_bounds__(256) void sumsq_kernel(const SumsqGroup g)
{
    __shared__ float red[256];
    const SumsqDesc& d = g.d[blockIdx.z];
    sumsq_slice(red, d.x, d.n, d.partial);
}

// loss_out[0] = sum(row_loss[0..M)) + reg_scale * sum(partials[0..P))   (one workgroup, fixed order)
__device__ __forceinline__ void loss_finalize_one(float (&red)[256], const float* __restrict__ row_loss, int M,
                                                  const float* __restrict__ partials, int P, float reg_scale, float* __restrict__ loss_out)
{
#pragma clang fp contract(off)
    float s = 0.f, q = 0.f;
    for (int i = threadIdx.x; i < M; i += 256) s += row_loss[i];
    for (int i = threadIdx.x; i < P; i += 256) q += partials[i];
    red[threadIdx.x] = fmaf(reg_scale, q, s);
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_out[0] = red[0];
}

struct LossDesc {
    const float *row_loss, *partials;
    float* loss_out;
    int M, P;
    float reg_scale;
};
struct LossGroup { LossDesc d[MMC_TRAINER_GROUP_MAX]; };
static_assert(sizeof(LossGroup) <= 4096, "kernel-argument limit");

__global__ __launch_bounds__(256) void loss_finalize_kernel(const LossGroup g)
{
    __shared__ float red[256];
    const LossDesc& d = g.d[blockIdx.z];
    loss_finalize_one(red, d.row_loss, d.M, d.partials, d.P, d.reg_scale, d.loss_out);
}

// torch.optim.Adam (single-tensor path), in its order of operations:
//   exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
//   denom = exp_avg_sq.sqrt() / sqrt(1 - beta2^t) + eps;  param.addcdiv_(exp_avg, denom, value=-(lr / (1 - beta1^t)))
__device__ __forceinline__ void adam_elems(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                           float* __restrict__ v, size_t n, float om_beta1, float beta2, float om_beta2, float eps,
                                           float step_size, float bc2_sqrt)
{
#pragma clang fp contract(off)   // two roundings each in mi, vi and denom; the parameter update is one fused multiply-add
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    // om_beta = (float)(1.0 - (double)beta): torch forms 1 - beta in double and casts the scalar, which is not 1.0f - (float)beta
    const float mi = m[i] + om_beta1 * (gi - m[i]);
    const float vi = v[i] * beta2 + om_beta2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = fmaf(-step_size, mi / denom, p[i]);
}

struct AdamDesc {
    float* p;
    const float* g;
    float *m, *v;
    size_t n;
    float om_beta1, beta2, om_beta2, eps, step_size, bc2_sqrt;
};
struct AdamGroup { AdamDesc d[MMC_TRAINER_GROUP_MAX]; };
static_assert(sizeof(AdamGroup) <= 4096, "kernel-argument limit");

__global__ __launch_bounds__(256) void adam_kernel(const AdamGroup g)
{
    const AdamDesc& d = g.d[blockIdx.z];
    adam_elems(d.p, d.g, d.m, d.v, d.n, d.om_beta1, d.beta2, d.om_beta2, d.eps, d.step_size, d.bc2_sqrt);
}

// ---- optimiser options (include/mmc.h, "optimiser options"): the kernels of a member that clips its gradient or averages its weights.
// A member with neither goes through adam_kernel above, whose code these do not share, so that launch stays what it was.

// The member's gradient norm from the 2L x 256 partials that sumsq_kernel left of its gW[l] / gb[l] (tensor k = 2l, 2l + 1 at
// partials[256 k ..]), summed in a fixed order: thread i takes partials[i], [i + 256], ... in order, then the LDS tree.
//   norm = sqrtf(total),  coef = fminf(1.0f, max_norm / (norm + 1e-6f))     torch.nn.utils.clip_grad_norm_, error_if_nonfinite=False
// torch clamps with clamp(max=1), which hands a NaN on where fminf would drop it: a NaN norm gives a NaN coefficient here too, and
// an infinite one gives 0.  Nothing is hidden: the Adam stage multiplies by what is written.
struct GnormDesc {
    const float* partials;
    float *coef, *norm_out;
    int P;
    float max_norm;
};
struct GnormGroup { GnormDesc d[MMC_TRAINER_GROUP_MAX]; };
static_assert(sizeof(GnormGroup) <= 4096, "kernel-argument limit");

__global__ __launch_bounds__(256) void gnorm_finalize_kernel(const GnormGroup g)
{
#pragma clang fp contract(off)
    __shared__ float red[256];
    const GnormDesc& d = g.d[blockIdx.z];
    float s = 0.f;
    for (int i = threadIdx.x; i < d.P; i += 256) s += d.partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = sqrtf(red[0]);
        const float q = d.max_norm / (norm + 1e-6f);
        float c = fminf(1.0f, q);
        if (q != q) c = q;
        d.coef[0] = c;
        d.norm_out[0] = norm;
    }
}

// adam_elems on gi = g[i] * *coef (one rounding; coef null: g[i] itself), then the shadow of the averaged weights from the
// parameter just written: s = s + om_d (p_new - s), two roundings like exp_avg (shadow null: none).
struct AdamOptDesc {
    float* p;
    const float* g;
    float *m, *v;
    size_t n;
    float om_beta1, beta2, om_beta2, eps, step_size, bc2_sqrt;
    const float* coef;
    float* shadow;
    float om_d;
};
struct AdamOptGroup { AdamOptDesc d[MMC_TRAINER_GROUP_MAX]; };
static_assert(sizeof(AdamOptGroup) <= 4096, "kernel-argument limit");

__global__ __launch_bounds__(256) void adam_opt_kernel(const AdamOptGroup g)
{
#pragma clang fp contract(off)   // as adam_elems: the parameter update is the one fused multiply-add
    const AdamOptDesc& d = g.d[blockIdx.z];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n) return;
    float gi = d.g[i];
    if (d.coef) gi = gi * d.coef[0];
    const float mi = d.m[i] + d.om_beta1 * (gi - d.m[i]);
    const float vi = d.v[i] * d.beta2 + d.om_beta2 * gi * gi;
    d.m[i] = mi;
    d.v[i] = vi;
    const float denom = sqrtf(vi) / d.bc2_sqrt + d.eps;
    const float pn = fmaf(-d.step_size, mi / denom, d.p[i]);
    d.p[i] = pn;
    if (d.shadow) {
        const float si = d.shadow[i];
        d.shadow[i] = si + d.om_d * (pn - si);
    }
}

// Xo[i][:] = Xn[order[i]][:], yo[i] = yn[order[i]]: the visiting order of a pass applied on the device (one float4 per thread)
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ Xn, const int32_t* __restrict__ yn,
                                                          const int64_t* __restrict__ order, int64_t n, int d4, float* __restrict__ Xo,
                                                          int32_t* __restrict__ yo)
{
    const int64_t i = blockIdx.x;
    const int64_t src = order[i];
    const float4* s = reinterpret_cast<const float4*>(Xn + (size_t)src * d4 * 4);
    float4* d = reinterpret_cast<float4*>(Xo + (size_t)i * d4 * 4);
    for (int k = threadIdx.x; k < d4; k += 256) d[k] = s[k];
    if (threadIdx.x == 0) yo[i] = yn[src];
    (void)n;
}

// A chunk of a pass over a resident feature set (mmc_trainer_partial_fit_set): Xo[i][:] = Xs[src(i)][:], yo[i] = ys[src(i)] with
// src(i) = visit[i], or first + i without a visiting order.  One wave per row, four rows per workgroup.  Any width: V4 moves 16-byte
// lanes (dim % 4 == 0: every row of either matrix then starts on a 16-byte boundary), otherwise dwords.
template <bool V4>
__global__ __launch_bounds__(256) void gather_set_rows_kernel(const float* __restrict__ Xs, const int32_t* __restrict__ ys,
                                                              const int64_t* __restrict__ visit, int64_t first, int rows, int dim,
                                                              float* __restrict__ Xo, int32_t* __restrict__ yo)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int64_t src = visit ? visit[i] : first + i;
    const float* s = Xs + (size_t)src * dim;
    float* d = Xo + (size_t)i * dim;
    if (V4) {
        const float4* s4 = reinterpret_cast<const float4*>(s);
        float4* d4 = reinterpret_cast<float4*>(d);
        for (int k = lane; k < dim / 4; k += 64) d4[k] = s4[k];
    } else {
        for (int k = lane; k < dim; k += 64) d[k] = s[k];
    }
    if (lane == 0) yo[i] = ys[src];
}

// The mixing form of gather_set_rows_kernel (mmc_trainer_partial_fit_set_mixed): position i of the chunk, in the chunk's
// mini-batch i / mb, becomes lam Xs[a] + oml Xs[b] with a = src(i), b = partner[i] and oml = 1.0f - lam[i / mb]: two rounded
// products and one rounded add per element (no fma), so the row is what numpy fp32 makes of it.  Both labels are kept.
template <bool V4>
__global__ __launch_bounds__(256) void gather_set_rows_mixed_kernel(const float* __restrict__ Xs, const int32_t* __restrict__ ys,
                                                                    const int64_t* __restrict__ visit, int64_t first,
                                                                    const int64_t* __restrict__ partner, const float* __restrict__ lam,
                                                                    int mb, int rows, int dim, float* __restrict__ Xo,
                                                                    int32_t* __restrict__ yo, int32_t* __restrict__ y2o)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int64_t a = visit ? visit[i] : first + i, b = partner[i];
    const float la = lam[i / mb], lb = 1.0f - la;
    const float *sa = Xs + (size_t)a * dim, *sb = Xs + (size_t)b * dim;
    float* d = Xo + (size_t)i * dim;
    if (V4) {
        const float4 *a4 = reinterpret_cast<const float4*>(sa), *b4 = reinterpret_cast<const float4*>(sb);
        float4* d4 = reinterpret_cast<float4*>(d);
        for (int k = lane; k < dim / 4; k += 64) {
            const float4 u = a4[k], v = b4[k];
            float4 o;
            o.x = la * u.x + lb * v.x;
            o.y = la * u.y + lb * v.y;
            o.z = la * u.z + lb * v.z;
            o.w = la * u.w + lb * v.w;
            d4[k] = o;
        }
    } else {
        for (int k = lane; k < dim; k += 64) d[k] = la * sa[k] + lb * sb[k];
    }
    if (lane == 0) {
        yo[i] = ys[a];
        y2o[i] = ys[b];
    }
}

// ---- batch normalisation (include/mmc.h, "batch normalisation"): the kernels of a member with mmc_trainer_set_batch_norm.  A member
// without it launches none of them.  Both step kernels share one shape: a workgroup of 256 threads takes 64 columns, thread
// (c, q) = (tid & 63, tid >> 6) column c of them and row quarter q, rows [q per, (q + 1) per) with per = ceil(M / 4).  A thread adds
// its rows in order on four chains, s = (s0 + s1) + (s2 + s3); the quarters meet in LDS as (p0 + p1) + (p2 + p3), which every thread
// of the column reads back, so all four hold the same bits.  The order is a function of (M, N) alone: no atomics, and nothing
// depends on the grid (a workgroup past its member's columns leaves before the first barrier) or on who shares the launch.
// Loads in flight: a wave's 64 lanes read 64 consecutive floats of one row (256 B, coalesced); the reductions keep four rows'
// loads per thread in flight (eight in the backward, which reads dA and Z), the element-wise passes are unrolled by four too.  At
// mb = 200, N = 500 that is 8 workgroups x 4 waves x 4 x 256 B = 32 KB requested at once on 400 KB that sit in L2 after the GEMM:
// the kernel is latency-bound at that size and the quarters are what spreads it over 32 waves (one thread per column: 8).
struct BnFwdDesc {
    const float* Z;              // [M][N] H W^T + b of the layer
    const float *gamma, *beta;   // [N]
    float* H;                    // [M][N] relu(gamma xhat + beta)
    float *mu, *rstd;            // [N] the mini-batch's mean and 1 / sqrt(v + eps), kept for the backward
    float *rmean, *rvar;         // [N] running statistics, or null (mmc_trainer_norm_stage leaves them alone)
    float* var;                  // [N] the biased variance v, or null
    int M, N;
    float eps, mom, om_mom, unbias;   // (float) of eps, momentum, 1 - momentum, M / (M - 1), each formed in double
};
struct BnFwdGroup { BnFwdDesc d[MMC_TRAINER_GROUP_MAX]; };
struct BnBwdDesc {
    float* dA;                   // [M][N] in: gradient w.r.t. gamma xhat + beta; out: gradient w.r.t. Z
    const float *Z, *mu, *rstd, *gamma;
    float *ggamma, *gbeta;       // [N]
    int M, N;
};
struct BnBwdGroup { BnBwdDesc d[MMC_TRAINER_GROUP_MAX]; };
// the fold of one trainer: one descriptor per hidden layer (n_layers <= 16, so at most 15)
struct BnFoldDesc {
    const float *W, *b, *gamma, *beta, *rmean, *rvar;
    float *Wf, *bf;
    int N, K;
    float eps;
};
struct BnFoldGroup { BnFoldDesc d[MMC_TRAINER_GROUP_MAX]; };
static_assert(sizeof(BnFwdGroup) <= 4096 && sizeof(BnBwdGroup) <= 4096 && sizeof(BnFoldGroup) <= 4096, "kernel-argument limit");

// mu = mean of the column, v = mean of (z - mu)^2 (two passes: E[z^2] - mu^2 cancels on a column of mean 1000 and deviation 0.1),
// xhat = (z - mu) rstd, H = relu(gamma xhat + beta); rm = om_mom rm + mom mu, rv = om_mom rv + mom (v unbias).  Nothing is fused.
__global__ __launch_bounds__(256) void bn_forward_kernel(const BnFwdGroup g)
{
#pragma clang fp contract(off)
    __shared__ float part[4][64];
    const BnFwdDesc& d = g.d[blockIdx.z];
    if ((int)blockIdx.x * 64 >= d.N) return;
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + c;
    const int M = d.M;
    const size_t N = (size_t)d.N;
    const bool live = n < d.N;
    const int per = (M + 3) >> 2;
    const int b = q * per < M ? q * per : M, e = b + per < M ? b + per : M;
    const float* z = d.Z + (live ? n : 0);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (live) {
        int m = b;
        for (; m + 3 < e; m += 4) {
            s0 += z[(size_t)m * N];
            s1 += z[(size_t)(m + 1) * N];
            s2 += z[(size_t)(m + 2) * N];
            s3 += z[(size_t)(m + 3) * N];
        }
        for (; m < e; ++m) s0 += z[(size_t)m * N];
    }
    part[q][c] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    const float mu = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) / (float)M;
    __syncthreads();
    s0 = s1 = s2 = s3 = 0.f;
    if (live) {
        int m = b;
        for (; m + 3 < e; m += 4) {
            const float d0 = z[(size_t)m * N] - mu, d1 = z[(size_t)(m + 1) * N] - mu;
            const float d2 = z[(size_t)(m + 2) * N] - mu, d3 = z[(size_t)(m + 3) * N] - mu;
            s0 += d0 * d0;
            s1 += d1 * d1;
            s2 += d2 * d2;
            s3 += d3 * d3;
        }
        for (; m < e; ++m) {
            const float d0 = z[(size_t)m * N] - mu;
            s0 += d0 * d0;
        }
    }
    part[q][c] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (!live) return;   // past the last barrier
    const float v = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) / (float)M;
    const float rstd = 1.0f / sqrtf(v + d.eps);
    const float ga = d.gamma[n], be = d.beta[n];
    float* h = d.H + n;
#pragma unroll 4
    for (int m = b; m < e; ++m) {
        const float xh = (z[(size_t)m * N] - mu) * rstd;
        h[(size_t)m * N] = fmaxf(ga * xh + be, 0.f);
    }
    if (q == 0) {
        d.mu[n] = mu;
        d.rstd[n] = rstd;
        if (d.var) d.var[n] = v;
        if (d.rmean) {
            d.rmean[n] = d.om_mom * d.rmean[n] + d.mom * mu;
            d.rvar[n] = d.om_mom * d.rvar[n] + d.mom * (v * d.unbias);
        }
    }
}

// gbeta = sum_m dA, ggamma = sum_m dA xhat, dZ = (gamma rstd / M) ((M dA - gbeta) - xhat ggamma), in place.  Nothing is fused.
__global__ __launch_bounds__(256) void bn_backward_kernel(const BnBwdGroup g)
{
#pragma clang fp contract(off)
    __shared__ float pb[4][64];
    __shared__ float pg[4][64];
    const BnBwdDesc& d = g.d[blockIdx.z];
    if ((int)blockIdx.x * 64 >= d.N) return;
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + c;
    const int M = d.M;
    const size_t N = (size_t)d.N;
    const bool live = n < d.N;
    const int per = (M + 3) >> 2;
    const int b = q * per < M ? q * per : M, e = b + per < M ? b + per : M;
    const float* z = d.Z + (live ? n : 0);
    float* a = d.dA + (live ? n : 0);
    const float mu = live ? d.mu[n] : 0.f, rstd = live ? d.rstd[n] : 0.f;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
    if (live) {
        int m = b;
        for (; m + 3 < e; m += 4) {
            const float a0 = a[(size_t)m * N], a1 = a[(size_t)(m + 1) * N], a2 = a[(size_t)(m + 2) * N], a3 = a[(size_t)(m + 3) * N];
            const float x0 = (z[(size_t)m * N] - mu) * rstd, x1 = (z[(size_t)(m + 1) * N] - mu) * rstd;
            const float x2 = (z[(size_t)(m + 2) * N] - mu) * rstd, x3 = (z[(size_t)(m + 3) * N] - mu) * rstd;
            b0 += a0;
            b1 += a1;
            b2 += a2;
            b3 += a3;
            g0 += a0 * x0;
            g1 += a1 * x1;
            g2 += a2 * x2;
            g3 += a3 * x3;
        }
        for (; m < e; ++m) {
            const float a0 = a[(size_t)m * N];
            const float x0 = (z[(size_t)m * N] - mu) * rstd;
            b0 += a0;
            g0 += a0 * x0;
        }
    }
    pb[q][c] = (b0 + b1) + (b2 + b3);
    pg[q][c] = (g0 + g1) + (g2 + g3);
    __syncthreads();
    if (!live) return;   // past the last barrier
    const float gb = (pb[0][c] + pb[1][c]) + (pb[2][c] + pb[3][c]);
    const float gg = (pg[0][c] + pg[1][c]) + (pg[2][c] + pg[3][c]);
    const float mf = (float)M;
    const float k = (d.gamma[n] * rstd) / mf;
#pragma unroll 4
    for (int m = b; m < e; ++m) {
        const float xh = (z[(size_t)m * N] - mu) * rstd;
        a[(size_t)m * N] = k * ((mf * a[(size_t)m * N] - gb) - xh * gg);
    }
    if (q == 0) {
        d.ggamma[n] = gg;
        d.gbeta[n] = gb;
    }
}

// s = gamma / sqrt(rv + eps); W'[j][:] = s W[j][:], b'[j] = beta + s (b[j] - rm[j]).  Row j of layer blockIdx.z per workgroup.
__global__ __launch_bounds__(256) void bn_fold_kernel(const BnFoldGroup g)
{
#pragma clang fp contract(off)
    const BnFoldDesc& d = g.d[blockIdx.z];
    const int j = blockIdx.x;
    if (j >= d.N) return;
    const float s = d.gamma[j] / sqrtf(d.rvar[j] + d.eps);
    const float* w = d.W + (size_t)j * d.K;
    float* wf = d.Wf + (size_t)j * d.K;
    for (int k = threadIdx.x; k < d.K; k += 256) wf[k] = s * w[k];
    if (threadIdx.x == 0) d.bf[j] = d.beta[j] + s * (d.b[j] - d.rmean[j]);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
struct mmc_trainer {
    int device = 0, L = 0, K = 0;
    std::vector<int> dims;
    std::vector<DevBuf<float>> W, b, gW, gb, mW, vW, mb, vb;
    std::vector<DevBuf<float>> Hbuf, dZbuf;             // the activations and their gradients of layers 1..L ([0] stays empty)
    std::vector<float*> H;                              // views: H[0] = mini-batch input, H[l+1] = layer l's output; size L+1
    std::vector<float*> dZ;                             // views: dZ[l] = gradient w.r.t. layer l-1's pre-activation (size L+1, [0] unused)
    DevBuf<float> cw;                                   // class weights or empty
    DevBuf<float> X, row_loss, partials, losses;
    DevBuf<int32_t> y;
    DevBuf<float> Xn;               // natural-order staging of a pass (device-side shuffle)
    DevBuf<int32_t> yn;
    DevBuf<int64_t> order;
    DevBuf<int64_t> visit;          // visiting order of a pass over a resident feature set
    double lr = 1e-3, beta1 = 0.9, beta2 = 0.999, eps = 1e-8, alpha = 1e-4;   // kept in double: torch derives its fp32 scalars from python floats
    long long t = 0;                                    // Adam step count
    std::vector<float> cw_host;
    // loss formulation (mmc_trainer_set_loss); all defaults = the plain weighted cross-entropy and its instantiation of the kernel
    double label_smoothing = 0.0, focal_gamma = 0.0;
    DevBuf<float> prior;                                // logit prior [K] or empty
    bool general = false;
    float w_total = 0.f;                                // the float of the double sum of the class weights in class order; K without
    DevBuf<char> scratch;                               // trainer_scratch (calib.hip's evaluation buffers)
    // regularisers (mmc_trainer_set_dropout; the plan of a mixed pass): all off = today's launches
    double p_input = 0.0, p_hidden = 0.0;
    uint64_t drop_seed = 0;
    uint32_t thresh_input = 0, thresh_hidden = 0;       // (uint32)floor(p 2^32); 0 = off
    float scale_input = 1.f, scale_hidden = 1.f;        // (float)(1.0 / (1.0 - p))
    DevBuf<int32_t> y2;                                 // the partner's label of every staged row of a mixed pass
    DevBuf<int64_t> partner;                            // device copy of a mixed pass's partner rows
    DevBuf<float> lam;                                  // device copy of its per-mini-batch lam
    // optimiser options (mmc_trainer_set_lr_schedule / _set_grad_clip / _set_ema): all off = today's launches
    int lr_kind = MMC_LR_CONSTANT;
    long long warmup_steps = 0, total_steps = 0;
    double final_ratio = 0.0;
    double max_norm = 0.0;                              // 0 = no clipping
    DevBuf<float> gpartials;                            // [2 * 16 + 1][256] partial sums of squares of gW[l] (2l), gb[l] (2l + 1), bn_g (2L)
    DevBuf<float> coef;                                 // the step's clipping coefficient
    DevBuf<float> gnorm;                                // pre-clip norm of every step of a pass, beside losses
    int gnorm_steps = 0;                                // steps of the last pass that wrote gnorm
    double ema_decay = 0.0;                             // 0 = no averaged weights
    std::vector<DevBuf<float>> sW, sb;                  // the shadow: averaged weights (empty without)
    int eval_which = MMC_WEIGHTS_RAW;                   // what the eval-mode forward reads
    // group-robust training (mmc_trainer_set_group_dro; the arrays of a weighted pass): all off = today's launches
    int n_groups = 0;                                   // 0 = no group DRO
    double dro_eta = 0.0;
    DevBuf<double> logq;                                // [n_groups] log q, normalised; lives across steps and passes
    DevBuf<float> row_w;                                // device copy of a weighted pass's row weights, by position
    DevBuf<int32_t> row_g;                              // and of its groups
    DevBuf<double> group_mass;                          // [steps][n_groups] V_a of every mini-batch of the pass
    DevBuf<float> row_scale;                            // [mb] c_i of the step
    // taxonomy-aware loss (mmc_trainer_set_hierarchy): nothing set = today's launches
    int hier_levels = 0;
    float hier_lam[MMC_HIER_MAX_LEVELS] = {0.f, 0.f, 0.f, 0.f};
    DevBuf<int32_t> hier_ids;                           // [hier_levels][K] node ids or empty
    DevBuf<float> hier_T;                               // [K][K] soft targets or empty
    bool hier = false;                                  // hier_levels > 0 or soft targets: the member takes ce_grad_hier_kernel
    // batch normalisation (mmc_trainer_set_batch_norm): off = today's launches.  Hidden layer h (0 .. L-2) owns [bn_off[h],
    // bn_off[h] + 2 dims[h+1]) of every bn_* array: gamma then beta in bn_p (bn_g, bn_m, bn_v alike, so Adam and the clipping norm
    // take all of them in one launch each), running mean then variance in bn_run, the step's mean then rstd in bn_stat.
    bool bn = false;
    double bn_eps = 1e-5, bn_mom = 0.1;
    std::vector<int64_t> bn_off;
    int64_t bn_total = 0;                               // 2 x the sum of the hidden widths
    DevBuf<float> bn_p, bn_g, bn_m, bn_v, bn_run, bn_stat;
    std::vector<DevBuf<float>> Zbuf;                    // [l + 1]: Z of hidden layer l, [mb][dims[l + 1]] (the backward reads it)
    std::vector<DevBuf<float>> fW, fb;                  // the folded hidden layers, what the eval-mode forward reads
    bool fold_stale = true;                             // a step or a state upload since the last fold
    float* bn_ptr(const DevBuf<float>& a, int h, int second) const { return a.p + bn_off[h] + (second ? dims[h + 1] : 0); }
};

#define T_K(expr)                                                                   \
    do {                                                                            \
        int r_ = (expr);                                                            \
        if (r_ != 0) return mmc_fail(MMC_ERR_HIP, "%s failed (%d)", #expr, r_);     \
    } while (0)

extern "C" void mmc_trainer_destroy(mmc_trainer* t)
{
    if (!t) return;
    hipSetDevice(t->device);
    delete t;
}

extern "C" int mmc_trainer_create(const float* const* W, const float* const* b, const int* dims, int n_layers, double lr, double beta1,
                                  double beta2, double eps, double alpha, const float* class_weight, int device, mmc_trainer** out)
{
    if (!out) return mmc_fail(MMC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!W || !b || !dims) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    if (n_layers < 1 || n_layers > 16) return mmc_fail(MMC_ERR_ARG, "n_layers %d out of range [1,16]", n_layers);
    for (int l = 0; l <= n_layers; ++l)
        if (dims[l] < 1) return mmc_fail(MMC_ERR_ARG, "dims[%d]=%d must be positive", l, dims[l]);
    if (!(lr > 0.) || !(beta1 >= 0. && beta1 < 1.) || !(beta2 >= 0. && beta2 < 1.) || !(eps >= 0.) || !(alpha >= 0.))
        return mmc_fail(MMC_ERR_ARG, "bad optimizer hyper-parameter (lr %g, betas %g %g, eps %g, alpha %g)", lr, beta1, beta2, eps, alpha);
    const int K = dims[n_layers];
    if (class_weight)
        for (int c = 0; c < K; ++c)
            if (!(class_weight[c] >= 0.f)) return mmc_fail(MMC_ERR_ARG, "class_weight[%d] = %g is negative", c, class_weight[c]);
    if (int r = check_device(device)) return r;
    HIP_TRY(hipSetDevice(device));
    mmc_trainer* t = new mmc_trainer();
    t->device = device; t->L = n_layers; t->K = K;
    t->dims.assign(dims, dims + n_layers + 1);
    t->lr = lr; t->beta1 = beta1; t->beta2 = beta2; t->eps = eps; t->alpha = alpha;
    auto up = [&](std::vector<DevBuf<float>>& dst, const float* src, size_t n, bool zero) -> bool {
        DevBuf<float> d;
        if (!d.alloc((int64_t)n)) return false;
        if ((zero ? hipMemset(d, 0, n * 4) : hipMemcpy(d, src, n * 4, hipMemcpyHostToDevice)) != hipSuccess) return false;
        dst.push_back(std::move(d));
        return true;
    };
    bool ok = true;
    for (int l = 0; l < n_layers && ok; ++l) {
        const size_t nw = (size_t)dims[l + 1] * dims[l], nb = (size_t)dims[l + 1];
        ok = up(t->W, W[l], nw, false) && up(t->b, b[l], nb, false) && up(t->gW, nullptr, nw, true) && up(t->gb, nullptr, nb, true) &&
             up(t->mW, nullptr, nw, true) && up(t->vW, nullptr, nw, true) && up(t->mb, nullptr, nb, true) && up(t->vb, nullptr, nb, true);
    }
    if (ok && class_weight) {
        ok = t->cw.alloc(K) && hipMemcpy(t->cw, class_weight, (size_t)K * 4, hipMemcpyHostToDevice) == hipSuccess;
        t->cw_host.assign(class_weight, class_weight + K);
    }
    double wtot = (double)K;
    if (class_weight) {
        wtot = 0.0;
        for (int c = 0; c < K; ++c) wtot += (double)class_weight[c];
    }
    t->w_total = (float)wtot;
    if (ok) ok = t->partials.alloc(256 * 16);
    if (!ok) {
        mmc_trainer_destroy(t);
        return mmc_fail(MMC_ERR_NOMEM, "hipMalloc/hipMemcpy failed while creating the trainer");
    }
    t->Hbuf.resize(n_layers + 1);
    t->dZbuf.resize(n_layers + 1);
    t->H.assign(n_layers + 1, nullptr);
    t->dZ.assign(n_layers + 1, nullptr);
    *out = t;
    return MMC_OK;
}

// the kernel's fp32 scalars of the trainer's loss options, each the float of a double expression (include/mmc.h)
static CeLoss trainer_ce_loss(const mmc_trainer* t)
{
    return CeLoss{t->prior, (float)(1.0 - t->label_smoothing), (float)(t->label_smoothing / (double)t->K), (float)t->focal_gamma, t->w_total};
}

extern "C" int mmc_trainer_set_loss(mmc_trainer* t, double label_smoothing, double focal_gamma, const float* logit_prior)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!(label_smoothing >= 0.0 && label_smoothing < 1.0))
        return mmc_fail(MMC_ERR_ARG, "label_smoothing = %g outside [0, 1)", label_smoothing);
    if (!(focal_gamma == 0.0 || (focal_gamma >= 1.0 && focal_gamma <= 8.0)))
        return mmc_fail(MMC_ERR_ARG, "focal_gamma = %g is neither 0 nor in [1, 8]", focal_gamma);
    if (logit_prior)
        for (int c = 0; c < t->K; ++c)
            if (!std::isfinite(logit_prior[c])) return mmc_fail(MMC_ERR_ARG, "logit_prior[%d] = %g is not finite", c, logit_prior[c]);
    if (t->hier_T.p && (label_smoothing != 0.0 || focal_gamma != 0.0))
        return mmc_fail(MMC_ERR_ARG, "label_smoothing = %g / focal_gamma = %g on a trainer with soft targets (mmc_trainer_set_hierarchy)",
                        label_smoothing, focal_gamma);
    HIP_TRY(hipSetDevice(t->device));
    // passes synchronise their stream before they return, so nothing in flight reads the prior that is replaced here
    DevBuf<float> prior;
    if (logit_prior) {
        if (!prior.alloc(t->K)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc failed for the logit prior (%d classes)", t->K);
        hipError_t e = hipMemcpy(prior, logit_prior, (size_t)t->K * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return mmc_fail(MMC_ERR_HIP, "uploading the logit prior: %s", hipGetErrorString(e));
    }
    t->prior = std::move(prior);
    t->label_smoothing = label_smoothing;
    t->focal_gamma = focal_gamma;
    t->general = label_smoothing != 0.0 || focal_gamma != 0.0 || t->prior.p != nullptr;
    return MMC_OK;
}

// ---- taxonomy-aware loss (include/mmc.h) ------------------------------------------------------------------------------------
extern "C" int mmc_trainer_set_hierarchy(mmc_trainer* t, int n_levels, const int32_t* level_of_class, const double* level_weight,
                                         const float* soft_targets)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (n_levels < 0 || n_levels > MMC_HIER_MAX_LEVELS) return mmc_fail(MMC_ERR_ARG, "n_levels = %d outside [0, %d]", n_levels, MMC_HIER_MAX_LEVELS);
    if (n_levels > 0 && (!level_of_class || !level_weight)) return mmc_fail(MMC_ERR_ARG, "n_levels = %d needs level_of_class and level_weight", n_levels);
    const int K = t->K;
    float lam[MMC_HIER_MAX_LEVELS] = {0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < n_levels; ++l) {
        if (!(level_weight[l] >= 0.0 && std::isfinite(level_weight[l]) && std::isfinite((float)level_weight[l])))
            return mmc_fail(MMC_ERR_ARG, "level_weight[%d] = %g is negative or not finite", l, level_weight[l]);
        lam[l] = (float)level_weight[l];
    }
    if (soft_targets) {
        for (int r = 0; r < K; ++r) {
            double sum = 0.0;
            for (int c = 0; c < K; ++c) {
                const float v = soft_targets[(size_t)r * K + c];
                if (!(v >= 0.f && std::isfinite(v)))
                    return mmc_fail(MMC_ERR_ARG, "soft_targets[%d][%d] = %g is negative or not finite", r, c, (double)v);
                sum += (double)v;
            }
            if (!(std::fabs(sum - 1.0) <= 1e-5)) return mmc_fail(MMC_ERR_ARG, "row %d of soft_targets sums to %.9g, not 1", r, sum);
        }
        if (t->label_smoothing != 0.0 || t->focal_gamma != 0.0)
            return mmc_fail(MMC_ERR_ARG, "soft_targets on a trainer with label_smoothing = %g / focal_gamma = %g (mmc_trainer_set_loss)",
                            t->label_smoothing, t->focal_gamma);
    }
    HIP_TRY(hipSetDevice(t->device));
    // passes synchronise their stream before they return, so nothing in flight reads what is replaced here
    DevBuf<int32_t> ids;
    DevBuf<float> T;
    if (n_levels) {
        if (!ids.alloc((int64_t)n_levels * K)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc failed for the level ids (%d levels, %d classes)", n_levels, K);
        hipError_t e = hipMemcpy(ids, level_of_class, (size_t)n_levels * K * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return mmc_fail(MMC_ERR_HIP, "uploading the level ids: %s", hipGetErrorString(e));
    }
    if (soft_targets) {
        if (!T.alloc((int64_t)K * K)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc failed for the soft targets (%d classes)", K);
        hipError_t e = hipMemcpy(T, soft_targets, (size_t)K * K * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return mmc_fail(MMC_ERR_HIP, "uploading the soft targets: %s", hipGetErrorString(e));
    }
    t->hier_ids = std::move(ids);
    t->hier_T = std::move(T);
    t->hier_levels = n_levels;
    std::copy(lam, lam + MMC_HIER_MAX_LEVELS, t->hier_lam);
    t->hier = n_levels > 0 || t->hier_T.p != nullptr;
    return MMC_OK;
}

static HierLoss trainer_hier_loss(const mmc_trainer* t)
{
    HierLoss h{t->hier_ids, t->hier_T, t->hier_levels, {0.f, 0.f, 0.f, 0.f}};
    std::copy(t->hier_lam, t->hier_lam + MMC_HIER_MAX_LEVELS, h.lam);
    return h;
}

extern "C" int mmc_trainer_set_dropout(mmc_trainer* t, double p_input, double p_hidden, uint64_t seed)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!(std::isfinite(p_input) && p_input >= 0.0 && p_input <= 0.9)) return mmc_fail(MMC_ERR_ARG, "p_input = %g outside [0, 0.9]", p_input);
    if (!(std::isfinite(p_hidden) && p_hidden >= 0.0 && p_hidden <= 0.9)) return mmc_fail(MMC_ERR_ARG, "p_hidden = %g outside [0, 0.9]", p_hidden);
    if (t->bn && p_hidden > 0.0)
        return mmc_fail(MMC_ERR_ARG, "p_hidden = %g on a trainer with batch normalisation (mmc_trainer_set_batch_norm)", p_hidden);
    t->p_input = p_input;
    t->p_hidden = p_hidden;
    t->drop_seed = seed;
    t->thresh_input = (uint32_t)std::floor(p_input * 4294967296.0);
    t->thresh_hidden = (uint32_t)std::floor(p_hidden * 4294967296.0);
    t->scale_input = (float)(1.0 / (1.0 - p_input));
    t->scale_hidden = (float)(1.0 / (1.0 - p_hidden));
    return MMC_OK;
}

// ---- optimiser options (include/mmc.h) ----------------------------------------------------------------------------------
// lr_s of the 1-based step s: a pure function of the step count, all in double
extern "C" int mmc_lr_schedule_at(double lr, int kind, long long warmup_steps, long long total_steps, double final_ratio, long long step,
                                  double* out)
{
    if (!out) return mmc_fail(MMC_ERR_ARG, "out is NULL");
    if (kind != MMC_LR_CONSTANT && kind != MMC_LR_LINEAR && kind != MMC_LR_COSINE)
        return mmc_fail(MMC_ERR_ARG, "kind = %d is not MMC_LR_CONSTANT, MMC_LR_LINEAR or MMC_LR_COSINE", kind);
    if (warmup_steps < 0) return mmc_fail(MMC_ERR_ARG, "warmup_steps = %lld is negative", warmup_steps);
    if (kind != MMC_LR_CONSTANT && !(total_steps > warmup_steps))
        return mmc_fail(MMC_ERR_ARG, "a decaying schedule needs total_steps > warmup_steps (got %lld, %lld)", total_steps, warmup_steps);
    if (!(final_ratio >= 0.0 && final_ratio <= 1.0)) return mmc_fail(MMC_ERR_ARG, "final_ratio = %g outside [0, 1]", final_ratio);
    const double s = (double)step, wu = (double)warmup_steps;
    const double w = warmup_steps > 0 ? std::min(1.0, s / wu) : 1.0;
    const double u = std::min(1.0, std::max(0.0, (s - wu) / (double)std::max(1LL, total_steps - warmup_steps)));
    const double r = final_ratio;
    double d = 1.0;
    if (kind == MMC_LR_LINEAR) d = 1.0 - (1.0 - r) * u;
    if (kind == MMC_LR_COSINE) d = r + (1.0 - r) * 0.5 * (1.0 + std::cos(3.14159265358979323846 * u));   // the double nearest pi
    *out = lr * w * d;
    return MMC_OK;
}

static double trainer_lr_at(const mmc_trainer* t, long long step)
{
    double lr = t->lr;
    mmc_lr_schedule_at(t->lr, t->lr_kind, t->warmup_steps, t->total_steps, t->final_ratio, step, &lr);   // the options were checked when set
    return lr;
}

extern "C" int mmc_trainer_set_lr_schedule(mmc_trainer* t, int kind, long long warmup_steps, long long total_steps, double final_ratio)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    double probe = 0.0;
    int r = mmc_lr_schedule_at(t->lr, kind, warmup_steps, total_steps, final_ratio, 1, &probe);
    if (r) return r;
    t->lr_kind = kind;
    t->warmup_steps = warmup_steps;
    t->total_steps = total_steps;
    t->final_ratio = final_ratio;
    return MMC_OK;
}

extern "C" int mmc_trainer_lr_at(mmc_trainer* t, long long step, double* lr)
{
    if (!t || !lr) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    return mmc_lr_schedule_at(t->lr, t->lr_kind, t->warmup_steps, t->total_steps, t->final_ratio, step, lr);
}

extern "C" int mmc_trainer_set_grad_clip(mmc_trainer* t, double max_norm)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!(max_norm == 0.0 || (max_norm > 0.0 && std::isfinite(max_norm) && std::isfinite((float)max_norm) && (float)max_norm > 0.f)))
        return mmc_fail(MMC_ERR_ARG, "max_norm = %g is neither 0 nor a positive finite fp32 value", max_norm);
    if (max_norm != 0.0 && !t->gpartials) {
        HIP_TRY(hipSetDevice(t->device));
        DevBuf<float> gp, cf;
        if (!gp.alloc((2 * 16 + 1) * 256) || !cf.alloc(1)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc failed for the gradient-norm partials");
        t->gpartials = std::move(gp);
        t->coef = std::move(cf);
    }
    t->max_norm = max_norm;
    t->gnorm_steps = 0;
    return MMC_OK;
}

extern "C" int mmc_trainer_grad_norms(mmc_trainer* t, float* out, int capacity, int* steps)
{
    if (!t || !steps) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    if (capacity < 0 || (capacity > 0 && !out)) return mmc_fail(MMC_ERR_ARG, "capacity = %d with out %s", capacity, out ? "set" : "NULL");
    *steps = t->gnorm_steps;
    const int n = std::min(capacity, t->gnorm_steps);
    if (n > 0) {
        HIP_TRY(hipSetDevice(t->device));
        HIP_TRY(hipMemcpy(out, t->gnorm, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    return MMC_OK;
}

extern "C" int mmc_trainer_set_ema(mmc_trainer* t, double decay)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!(decay == 0.0 || (decay > 0.0 && decay < 1.0))) return mmc_fail(MMC_ERR_ARG, "decay = %g is neither 0 nor in (0, 1)", decay);
    if (t->bn && decay != 0.0)
        return mmc_fail(MMC_ERR_ARG, "decay = %g on a trainer with batch normalisation (mmc_trainer_set_batch_norm)", decay);
    HIP_TRY(hipSetDevice(t->device));
    if (decay == 0.0) {
        t->sW.clear();
        t->sb.clear();
        t->eval_which = MMC_WEIGHTS_RAW;
    } else if (t->sW.empty()) {   // passes synchronise their stream before they return: the parameters copied here are settled
        std::vector<DevBuf<float>> sW(t->L), sb(t->L);
        bool ok = true;
        auto dup = [&](DevBuf<float>& dst, const float* src, size_t n) -> bool {
            return dst.alloc((int64_t)n) && hipMemcpy(dst, src, n * 4, hipMemcpyDeviceToDevice) == hipSuccess;
        };
        for (int l = 0; l < t->L && ok; ++l)
            ok = dup(sW[l], t->W[l], (size_t)t->dims[l + 1] * t->dims[l]) && dup(sb[l], t->b[l], (size_t)t->dims[l + 1]);
        if (!ok) {
            (void)hipGetLastError();
            return mmc_fail(MMC_ERR_NOMEM, "hipMalloc/hipMemcpy failed for the averaged weights");
        }
        t->sW = std::move(sW);
        t->sb = std::move(sb);
    }
    t->ema_decay = decay;
    return MMC_OK;
}

extern "C" int mmc_trainer_ema_state(mmc_trainer* t, int set, float* const* W, float* const* b)
{
    if (!t || !W || !b) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    if (t->sW.empty()) return mmc_fail(MMC_ERR_ARG, "the trainer keeps no averaged weights (mmc_trainer_set_ema)");
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipDeviceSynchronize());
    for (int l = 0; l < t->L; ++l) {
        const size_t nw = (size_t)t->dims[l + 1] * t->dims[l] * 4, nb = (size_t)t->dims[l + 1] * 4;
        if (set) { HIP_TRY(hipMemcpy(t->sW[l], W[l], nw, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(t->sb[l], b[l], nb, hipMemcpyHostToDevice)); }
        else { HIP_TRY(hipMemcpy(W[l], t->sW[l], nw, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(b[l], t->sb[l], nb, hipMemcpyDeviceToHost)); }
    }
    return MMC_OK;
}

extern "C" int mmc_trainer_eval_weights(mmc_trainer* t, int which)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (which != MMC_WEIGHTS_RAW && which != MMC_WEIGHTS_AVERAGED)
        return mmc_fail(MMC_ERR_ARG, "which = %d is neither MMC_WEIGHTS_RAW nor MMC_WEIGHTS_AVERAGED", which);
    if (which == MMC_WEIGHTS_AVERAGED && t->sW.empty())
        return mmc_fail(MMC_ERR_ARG, "the trainer keeps no averaged weights (mmc_trainer_set_ema)");
    t->eval_which = which;
    return MMC_OK;
}

extern "C" int mmc_trainer_optimizer_options(mmc_trainer* t, int* lr_kind, long long* warmup_steps, long long* total_steps,
                                             double* final_ratio, double* max_norm, double* ema_decay, int* eval_which)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (lr_kind) *lr_kind = t->lr_kind;
    if (warmup_steps) *warmup_steps = t->warmup_steps;
    if (total_steps) *total_steps = t->total_steps;
    if (final_ratio) *final_ratio = t->final_ratio;
    if (max_norm) *max_norm = t->max_norm;
    if (ema_decay) *ema_decay = t->ema_decay;
    if (eval_which) *eval_which = t->eval_which;
    return MMC_OK;
}

// ---- group-robust training (include/mmc.h) -------------------------------------------------------------------------------
// lse = mx + log(sum_b exp(logq_b - mx)), the sum in index order: the host form of dro_update_kernel's normaliser
static double logq_lse(const double* logq, int G)
{
    double mx = logq[0];
    for (int a = 1; a < G; ++a) mx = std::max(mx, logq[a]);
    double s = 0.0;
    for (int a = 0; a < G; ++a) s += std::exp(logq[a] - mx);
    return mx + std::log(s);
}

extern "C" int mmc_trainer_set_group_dro(mmc_trainer* t, int n_groups, double eta)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (n_groups < 0 || n_groups > MMC_DRO_MAX_GROUPS) return mmc_fail(MMC_ERR_ARG, "n_groups = %d outside [0, %d]", n_groups, MMC_DRO_MAX_GROUPS);
    if (!(eta >= 0.0 && eta <= 10.0)) return mmc_fail(MMC_ERR_ARG, "eta = %g outside [0, 10]", eta);
    HIP_TRY(hipSetDevice(t->device));
    DevBuf<double> logq;
    if (n_groups) {   // passes synchronise their stream before they return, so nothing in flight reads the state that is replaced here
        if (!logq.alloc(n_groups)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc failed for the group distribution (%d groups)", n_groups);
        const std::vector<double> uniform((size_t)n_groups, -std::log((double)n_groups));
        hipError_t e = hipMemcpy(logq, uniform.data(), (size_t)n_groups * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) return mmc_fail(MMC_ERR_HIP, "uploading the group distribution: %s", hipGetErrorString(e));
    }
    t->logq = std::move(logq);
    t->n_groups = n_groups;
    t->dro_eta = eta;
    return MMC_OK;
}

extern "C" int mmc_trainer_group_dro_state(mmc_trainer* t, int set, double* log_q)
{
    if (!t || !log_q) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    if (!t->n_groups) return mmc_fail(MMC_ERR_ARG, "the trainer keeps no group distribution (mmc_trainer_set_group_dro)");
    const int G = t->n_groups;
    HIP_TRY(hipSetDevice(t->device));
    if (!set) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(log_q, t->logq, (size_t)G * 8, hipMemcpyDeviceToHost));
        return MMC_OK;
    }
    for (int a = 0; a < G; ++a)
        if (!std::isfinite(log_q[a])) return mmc_fail(MMC_ERR_ARG, "log_q[%d] = %g is not finite", a, log_q[a]);
    // a state that is normalised already (what a read returns: |lse| at rounding level) goes back as it is, so a resume continues
    // on the bits it left; anything else is renormalised
    std::vector<double> q(log_q, log_q + G);
    const double lse = logq_lse(q.data(), G);
    if (std::fabs(lse) > 0x1p-40)
        for (int a = 0; a < G; ++a) q[a] = q[a] - lse;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(t->logq, q.data(), (size_t)G * 8, hipMemcpyHostToDevice));
    return MMC_OK;
}

// ---- batch normalisation (include/mmc.h) -----------------------------------------------------------------------------------
extern "C" int mmc_trainer_set_batch_norm(mmc_trainer* t, int enable, double eps, double momentum)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    HIP_TRY(hipSetDevice(t->device));
    if (!enable) {   // passes synchronise their stream before they return: nothing in flight reads what is freed here
        t->bn = false;
        t->bn_p.reset(); t->bn_g.reset(); t->bn_m.reset(); t->bn_v.reset(); t->bn_run.reset(); t->bn_stat.reset();
        t->Zbuf.clear(); t->fW.clear(); t->fb.clear();
        t->bn_off.clear();
        t->bn_total = 0;
        return MMC_OK;
    }
    if (!(eps > 0.0 && std::isfinite(eps) && (float)eps > 0.f)) return mmc_fail(MMC_ERR_ARG, "eps = %g is not a positive finite fp32 value", eps);
    if (!(momentum > 0.0 && momentum <= 1.0)) return mmc_fail(MMC_ERR_ARG, "momentum = %g outside (0, 1]", momentum);
    if (t->p_hidden > 0.0)
        return mmc_fail(MMC_ERR_ARG, "batch normalisation on a trainer with hidden dropout p_hidden = %g (mmc_trainer_set_dropout)", t->p_hidden);
    if (!t->sW.empty())
        return mmc_fail(MMC_ERR_ARG, "batch normalisation on a trainer with averaged weights, decay = %g (mmc_trainer_set_ema)", t->ema_decay);
    if (!(t->eps > 0.0))
        return mmc_fail(MMC_ERR_ARG, "batch normalisation freezes the hidden biases at a zero gradient, which needs Adam's eps > 0 (got %g)", t->eps);
    if (t->bn) {   // already on: the state stays, the two scalars move
        t->bn_eps = eps;
        t->bn_mom = momentum;
        t->fold_stale = true;
        return MMC_OK;
    }
    const int H = t->L - 1;
    std::vector<int64_t> off(H);
    int64_t total = 0;
    for (int h = 0; h < H; ++h) {
        off[h] = total;
        total += 2 * (int64_t)t->dims[h + 1];
    }
    DevBuf<float> p, g, m, v, run, stat;
    std::vector<DevBuf<float>> fW(H), fb(H);
    if (total) {
        bool ok = p.alloc(total) && g.alloc(total) && m.alloc(total) && v.alloc(total) && run.alloc(total) && stat.alloc(total);
        for (int h = 0; h < H && ok; ++h) ok = fW[h].alloc((int64_t)t->dims[h + 1] * t->dims[h]) && fb[h].alloc(t->dims[h + 1]);
        if (!ok) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc failed for the batch-normalisation state (%lld values)", (long long)total);
        // gamma = 1, beta = 0; running mean 0, running variance 1: the same pattern in both arrays
        std::vector<float> init((size_t)total, 0.f);
        for (int h = 0; h < H; ++h) {
            std::fill(init.begin() + off[h], init.begin() + off[h] + t->dims[h + 1], 1.f);
            std::fill(init.begin() + off[h] + t->dims[h + 1], init.begin() + off[h] + 2 * t->dims[h + 1], 0.f);
        }
        HIP_TRY(hipMemcpy(p, init.data(), (size_t)total * 4, hipMemcpyHostToDevice));
        for (int h = 0; h < H; ++h) {   // the running statistics: mean first (0), variance second (1)
            std::fill(init.begin() + off[h], init.begin() + off[h] + t->dims[h + 1], 0.f);
            std::fill(init.begin() + off[h] + t->dims[h + 1], init.begin() + off[h] + 2 * t->dims[h + 1], 1.f);
        }
        HIP_TRY(hipMemcpy(run, init.data(), (size_t)total * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(g, 0, (size_t)total * 4));
        HIP_TRY(hipMemset(m, 0, (size_t)total * 4));
        HIP_TRY(hipMemset(v, 0, (size_t)total * 4));
        HIP_TRY(hipMemset(stat, 0, (size_t)total * 4));
        // the bias of a normalised layer cancels: its gradient is zero from here on (no colsum launch writes it)
        for (int h = 0; h < H; ++h) HIP_TRY(hipMemset(t->gb[h], 0, (size_t)t->dims[h + 1] * 4));
    }
    t->bn_p = std::move(p); t->bn_g = std::move(g); t->bn_m = std::move(m); t->bn_v = std::move(v);
    t->bn_run = std::move(run); t->bn_stat = std::move(stat);
    t->fW = std::move(fW); t->fb = std::move(fb);
    t->Zbuf.clear();
    t->Zbuf.resize(t->L + 1);
    t->bn_off = std::move(off);
    t->bn_total = total;
    t->bn_eps = eps;
    t->bn_mom = momentum;
    t->bn = true;
    t->fold_stale = true;
    return MMC_OK;
}

extern "C" int mmc_trainer_batch_norm_state(mmc_trainer* t, int set, float* const* gamma, float* const* beta, float* const* running_mean,
                                            float* const* running_var, float* const* adam_m_gamma, float* const* adam_v_gamma,
                                            float* const* adam_m_beta, float* const* adam_v_beta)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!gamma || !beta || !running_mean || !running_var || !adam_m_gamma || !adam_v_gamma || !adam_m_beta || !adam_v_beta)
        return mmc_fail(MMC_ERR_ARG, "NULL argument");
    if (!t->bn) return mmc_fail(MMC_ERR_ARG, "the trainer has no batch normalisation (mmc_trainer_set_batch_norm)");
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipDeviceSynchronize());
    for (int h = 0; h < t->L - 1; ++h) {
        const size_t nb = (size_t)t->dims[h + 1] * 4;
        float* host[8] = {gamma[h], beta[h], running_mean[h], running_var[h], adam_m_gamma[h], adam_m_beta[h], adam_v_gamma[h], adam_v_beta[h]};
        float* dev[8] = {t->bn_ptr(t->bn_p, h, 0), t->bn_ptr(t->bn_p, h, 1), t->bn_ptr(t->bn_run, h, 0), t->bn_ptr(t->bn_run, h, 1),
                         t->bn_ptr(t->bn_m, h, 0), t->bn_ptr(t->bn_m, h, 1), t->bn_ptr(t->bn_v, h, 0), t->bn_ptr(t->bn_v, h, 1)};
        for (int a = 0; a < 8; ++a) {
            if (!host[a]) return mmc_fail(MMC_ERR_ARG, "NULL array for hidden layer %d", h);
            if (set) HIP_TRY(hipMemcpy(dev[a], host[a], nb, hipMemcpyHostToDevice));
            else HIP_TRY(hipMemcpy(host[a], dev[a], nb, hipMemcpyDeviceToHost));
        }
    }
    if (set) t->fold_stale = true;
    return MMC_OK;
}

// W' / b' of the hidden layers from the current gamma, beta and running statistics, on `st`; nothing when the fold is current
static int trainer_refresh_fold(mmc_trainer* t, hipStream_t st)
{
    if (!t->bn || !t->fold_stale) return 0;
    const int H = t->L - 1;
    if (H > 0) {
        BnFoldGroup g;
        int nmax = 0;
        for (int h = 0; h < H; ++h) {
            g.d[h] = BnFoldDesc{t->W[h], t->b[h], t->bn_ptr(t->bn_p, h, 0), t->bn_ptr(t->bn_p, h, 1), t->bn_ptr(t->bn_run, h, 0),
                                t->bn_ptr(t->bn_run, h, 1), t->fW[h], t->fb[h], t->dims[h + 1], t->dims[h], (float)t->bn_eps};
            nmax = std::max(nmax, t->dims[h + 1]);
        }
        hipLaunchKernelGGL(bn_fold_kernel, dim3(nmax, 1, H), dim3(256), 0, st, g);
        HIP_TRY(hipGetLastError());
    }
    t->fold_stale = false;
    return 0;
}

extern "C" int mmc_trainer_folded_params(mmc_trainer* t, float* const* W, float* const* b)
{
    if (!t || !W || !b) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    if (!t->bn) return mmc_trainer_get_params(t, W, b);
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipDeviceSynchronize());
    if (int r = trainer_refresh_fold(t, nullptr)) return r;
    HIP_TRY(hipDeviceSynchronize());
    for (int l = 0; l < t->L; ++l) {
        const bool folded = l < t->L - 1;
        HIP_TRY(hipMemcpy(W[l], folded ? t->fW[l].p : t->W[l].p, (size_t)t->dims[l + 1] * t->dims[l] * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(b[l], folded ? t->fb[l].p : t->b[l].p, (size_t)t->dims[l + 1] * 4, hipMemcpyDeviceToHost));
    }
    return MMC_OK;
}

// A mini-batch of one row has no variance: a pass of a normalised trainer whose mini-batch, or whose last one, holds fewer than two
// rows is refused where minibatch_wsums refuses, before anything is uploaded or launched.
static int check_bn_minibatches(const char* who, const mmc_trainer* t, int64_t n, int mb)
{
    if (!t->bn) return 0;
    const int64_t last = n - (n - 1) / mb * mb;
    if (mb < 2 || last < 2)
        return mmc_fail(MMC_ERR_ARG, "%sbatch normalisation needs at least 2 rows in every mini-batch: %lld rows in mini-batches of %d leave one of %lld",
                        who, (long long)n, mb, (long long)(mb < 2 ? mb : last));
    return 0;
}

static int trainer_reserve(mmc_trainer* t, int64_t n, int mb, int steps)
{
    int r;
    if (t->bn)
        for (int l = 1; l < t->L; ++l)
            if ((r = t->Zbuf[l].reserve((int64_t)mb * t->dims[l]))) return r;
    if (t->max_norm > 0.0) {
        if (steps > t->gnorm.cap) t->gnorm_steps = 0;   // (the norms of the last pass go with the old block)
        if ((r = t->gnorm.reserve(steps))) return r;
    }
    if ((r = t->X.reserve(n * t->dims[0])) || (r = t->y.reserve(n))) return r;
    for (int l = 1; l <= t->L; ++l) {
        if ((r = t->Hbuf[l].reserve((int64_t)mb * t->dims[l])) || (r = t->dZbuf[l].reserve((int64_t)mb * t->dims[l]))) return r;
        t->H[l] = t->Hbuf[l];
        t->dZ[l] = t->dZbuf[l];
    }
    if ((r = t->row_loss.reserve(mb)) || (r = t->losses.reserve(steps))) return r;
    return 0;
}

// ---- the step ------------------------------------------------------------------------------------------------------------
namespace {

// one trainer's part in a step: its mini-batch is rows [off, off + cur) of its staging X / y, its loss goes to losses[slot]
struct StepMember {
    mmc_trainer* t;
    int64_t off;
    int cur;
    float inv_wsum;   // 1 / sum of the mini-batch's class weights (of a mixed one: of lam w[ya] + oml w[yb])
    int slot;
    bool mixed;       // the rows were mixed: t->y2 holds the partners' labels, the loss stage takes two targets
    float lam;
    // group-robust training: a weighted member takes ce_grad_weighted_kernel; inv_wsum is then 1 / sum of the row masses, or 1.0f
    // with groups, whose rows dro_update_kernel and row_scale_kernel normalise
    bool weighted = false;
    const float* rw = nullptr;      // device: the weights of the mini-batch's positions, or null (all 1)
    const int32_t* rg = nullptr;    // device: their groups, or null (row weights only)
    const double* V = nullptr;      // device: [n_groups] the groups' masses in this mini-batch
};

template <bool TA, bool TB, int EPI0, int EPI1>
int launch_tgemm(const GemmGroup& g, int cnt, hipStream_t st)
{
    int tm = 0, tn = 0;
    for (int i = 0; i < cnt; ++i) {
        tm = std::max(tm, (g.d[i].M + 63) / 64);
        tn = std::max(tn, (g.d[i].N + 63) / 64);
    }
    hipLaunchKernelGGL((tgemm_f32_kernel<TA, TB, EPI0, EPI1>), dim3(tm, tn, cnt), dim3(256), 0, st, g);
    return (int)hipGetLastError();
}

// layer l of the forward on mb rows of t->H[l]
GemmDesc forward_desc(const mmc_trainer* t, int l, int mb)
{
    return GemmDesc{t->H[l], t->W[l], t->H[l + 1], t->b[l], mb, t->dims[l + 1], t->dims[l], l == t->L - 1 ? TEPI_BIAS : TEPI_BIAS_RELU, 0.f};
}

// the masks of site `site` of t at its current step count; hidden sites share p_hidden
DropMask drop_mask(const mmc_trainer* t, int site)
{
    return DropMask{site ? t->thresh_hidden : t->thresh_input, (uint32_t)t->drop_seed, (uint32_t)(t->drop_seed >> 32), (uint32_t)t->t,
                    (uint32_t)site, site ? t->scale_hidden : t->scale_input};
}

// the loss stage on mb rows of logits: which instantiation runs is a function of the trainer's options alone
CeDesc ce_desc(const mmc_trainer* t, const float* logits, const int32_t* y, int mb, float inv_wsum)
{
    return CeDesc{logits, y, t->cw, t->dZ[t->L], t->row_loss, mb, t->K, inv_wsum, t->general ? 1 : 0, trainer_ce_loss(t)};
}

// One optimizer step of every member in `act`: each kind of launch once, the member as blockIdx.z.  A member takes part in the
// launches of the layers it has, in the order forward, loss, regularised loss, backward from the last layer, Adam.
int trainer_group_step(const StepMember* act, int cnt, hipStream_t st)
{
    int Lmax = 0;
    for (int i = 0; i < cnt; ++i) {
        mmc_trainer* t = act[i].t;
        t->H[0] = t->X + (size_t)act[i].off * t->dims[0];
        Lmax = std::max(Lmax, t->L);
    }
    {   // input dropout: the mask of site 0 on the members' staged rows, before layer 0 (and after the mixing of a mixed pass)
        DropRowsGroup g;
        int k = 0;
        size_t emax = 0;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            if (!t->thresh_input) continue;
            g.d[k++] = DropRowsDesc{t->H[0], act[i].cur, t->dims[0], drop_mask(t, 0)};
            emax = std::max(emax, (size_t)act[i].cur * t->dims[0]);
        }
        if (k) hipLaunchKernelGGL(dropout_rows_kernel, dim3((unsigned)std::min<size_t>((emax + 255) / 256, 4096), 1, k), dim3(256), 0, st, g);
    }
    for (int l = 0; l < Lmax; ++l) {
        GemmDropGroup g;
        BnFwdGroup gn;
        int k = 0, tm = 0, tn = 0, kn = 0, nn = 0;
        bool drops = false;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            if (l >= t->L) continue;
            g.d[k] = forward_desc(t, l, act[i].cur);
            g.r[k] = DropMask{};
            if (t->thresh_hidden && l < t->L - 1) {   // the last layer never drops
                g.d[k].epi = TEPI_BIAS_RELU_DROP;
                g.r[k] = drop_mask(t, l + 1);
                drops = true;
            }
            if (t->bn && l < t->L - 1) {   // a normalised layer: Z = H W^T + b to a buffer of its own, bn_forward_kernel makes H(l+1)
                g.d[k].C = t->Zbuf[l + 1];
                g.d[k].epi = TEPI_BIAS;
                const int no = t->dims[l + 1], mb = act[i].cur;
                gn.d[kn++] = BnFwdDesc{t->Zbuf[l + 1], t->bn_ptr(t->bn_p, l, 0), t->bn_ptr(t->bn_p, l, 1), t->H[l + 1],
                                       t->bn_ptr(t->bn_stat, l, 0), t->bn_ptr(t->bn_stat, l, 1), t->bn_ptr(t->bn_run, l, 0),
                                       t->bn_ptr(t->bn_run, l, 1), nullptr, mb, no, (float)t->bn_eps, (float)t->bn_mom,
                                       (float)(1.0 - t->bn_mom), (float)((double)mb / ((double)mb - 1.0))};
                nn = std::max(nn, no);
            }
            tm = std::max(tm, (g.d[k].M + 63) / 64);
            tn = std::max(tn, (g.d[k].N + 63) / 64);
            ++k;
        }
        if (drops) {
            hipLaunchKernelGGL(tgemm_f32_drop_kernel, dim3(tm, tn, k), dim3(256), 0, st, g);
            T_K((int)hipGetLastError());
        } else {
            GemmGroup plain;
            std::copy(g.d, g.d + k, plain.d);
            T_K((launch_tgemm<false, true, TEPI_BIAS_RELU, TEPI_BIAS>(plain, k, st)));
        }
        if (kn) hipLaunchKernelGGL(bn_forward_kernel, dim3((nn + 63) / 64, 1, kn), dim3(256), 0, st, gn);
    }
    {
        CeGroup g;
        CeMixGroup gm;
        CeRowGroup gr;
        DroGroup gd;
        RowScaleGroup gs;
        CeHierGroup gh;
        int k = 0, km = 0, kr = 0, kd = 0, kh = 0, mmax = 0, mmax_mixed = 0, mmax_rows = 0, mmax_dro = 0, mmax_hier = 0;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            if (t->hier) {   // a hierarchy: one kernel with or without row weights (a mixed pass was refused before the first launch)
                gh.d[kh++] = CeHierDesc{ce_desc(t, t->H[t->L], t->y + act[i].off, act[i].cur, act[i].inv_wsum),
                                        act[i].weighted ? act[i].rw : nullptr, trainer_hier_loss(t)};
                mmax_hier = std::max(mmax_hier, act[i].cur);
            }
            if (act[i].weighted) {
                if (!t->hier) {
                    gr.d[kr++] = CeRowDesc{ce_desc(t, t->H[t->L], t->y + act[i].off, act[i].cur, act[i].inv_wsum), act[i].rw};
                    mmax_rows = std::max(mmax_rows, act[i].cur);
                }
                if (act[i].rg) {
                    gd.d[kd] = DroDesc{t->row_loss, act[i].rg, act[i].V, t->logq, t->row_scale, nullptr, act[i].cur, t->n_groups, t->dro_eta};
                    gs.d[kd] = RowScaleDesc{t->dZ[t->L], t->row_loss, t->row_scale, act[i].cur, t->K};
                    ++kd;
                    mmax_dro = std::max(mmax_dro, act[i].cur);
                }
            } else if (act[i].mixed) {
                gm.d[km++] = CeMixDesc{t->H[t->L], t->y + act[i].off, t->y2 + act[i].off, t->cw, t->dZ[t->L], t->row_loss, act[i].cur, t->K,
                                       act[i].inv_wsum, act[i].lam, 1.0f - act[i].lam, trainer_ce_loss(t)};
                mmax_mixed = std::max(mmax_mixed, act[i].cur);
            } else if (!t->hier) {
                g.d[k++] = ce_desc(t, t->H[t->L], t->y + act[i].off, act[i].cur, act[i].inv_wsum);
                mmax = std::max(mmax, act[i].cur);
            }
        }
        if (k) hipLaunchKernelGGL(ce_grad_kernel, dim3((mmax + 3) / 4, 1, k), dim3(256), 0, st, g);
        if (km) hipLaunchKernelGGL(ce_grad_mixed_kernel, dim3((mmax_mixed + 3) / 4, 1, km), dim3(256), 0, st, gm);
        if (kr) hipLaunchKernelGGL(ce_grad_weighted_kernel, dim3((mmax_rows + 3) / 4, 1, kr), dim3(256), 0, st, gr);
        if (kh) hipLaunchKernelGGL(ce_grad_hier_kernel, dim3((mmax_hier + 3) / 4, 1, kh), dim3(256), 0, st, gh);
        if (kd) {   // the groups' members: q moves on the device, then every row takes its group's share
            hipLaunchKernelGGL(dro_update_kernel, dim3(1, 1, kd), dim3(1024), 0, st, gd);
            hipLaunchKernelGGL(row_scale_kernel, dim3((mmax_dro + 3) / 4, 1, kd), dim3(256), 0, st, gs);
        }
    }
    // regularised loss of this mini-batch (before the update): data + (0.5 alpha / mb) sum W^2
    for (int l = 0; l < Lmax; ++l) {
        SumsqGroup g;
        int k = 0;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            if (l < t->L) g.d[k++] = SumsqDesc{t->W[l], t->partials + 256 * l, (size_t)t->dims[l + 1] * t->dims[l]};
        }
        hipLaunchKernelGGL(sumsq_kernel, dim3(256, 1, k), dim3(256), 0, st, g);
    }
    {
        LossGroup g;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            g.d[i] = LossDesc{t->row_loss, t->partials, t->losses + act[i].slot, act[i].cur, 256 * t->L,
                              (float)(0.5 * t->alpha / (double)act[i].cur)};
        }
        hipLaunchKernelGGL(loss_finalize_kernel, dim3(1, 1, cnt), dim3(256), 0, st, g);
    }
    for (int l = Lmax - 1; l >= 0; --l) {
        GemmGroup gw, gz;
        ColsumGroup gc;
        BnBwdGroup gn;
        int k = 0, kz = 0, nmax = 0, kc = 0, kn = 0, nn = 0;
        bool drops = false;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            if (l >= t->L) continue;
            const int no = t->dims[l + 1], ni = t->dims[l], mb = act[i].cur;
            gw.d[k] = GemmDesc{t->dZ[l + 1], t->H[l], t->gW[l], t->W[l], no, ni, mb, TEPI_L2, (float)(t->alpha / (double)mb)};
            ++k;
            if (!(t->bn && l < t->L - 1)) {   // the bias of a normalised layer is frozen: gb[l] stays the zeros it was filled with
                gc.d[kc++] = ColsumDesc{t->dZ[l + 1], t->gb[l], mb, no};
                nmax = std::max(nmax, no);
            }
            if (t->bn && l > 0) {   // dZ[l] is dA of hidden layer l - 1 once this iteration's mask launch has run: make it dZ in place
                gn.d[kn++] = BnBwdDesc{t->dZ[l], t->Zbuf[l], t->bn_ptr(t->bn_stat, l - 1, 0), t->bn_ptr(t->bn_stat, l - 1, 1),
                                       t->bn_ptr(t->bn_p, l - 1, 0), t->bn_ptr(t->bn_g, l - 1, 0), t->bn_ptr(t->bn_g, l - 1, 1), mb, ni};
                nn = std::max(nn, ni);
            }
            if (l > 0) {
                gz.d[kz] = GemmDesc{t->dZ[l + 1], t->W[l], t->dZ[l], t->H[l], mb, ni, no, TEPI_MASK, 0.f};
                if (t->thresh_hidden) {   // H(l) was dropped in the forward: the kept elements carry the scale back
                    gz.d[kz].epi = TEPI_MASK_SCALE;
                    gz.d[kz].scale = t->scale_hidden;
                    drops = true;
                }
                ++kz;
            }
        }
        T_K((launch_tgemm<true, false, TEPI_L2, TEPI_L2>(gw, k, st)));
        if (kc) hipLaunchKernelGGL(colsum_kernel, dim3((nmax + 255) / 256, 1, kc), dim3(256), 0, st, gc);
        if (kz && drops) {
            int tm = 0, tn = 0;
            for (int i = 0; i < kz; ++i) {
                tm = std::max(tm, (gz.d[i].M + 63) / 64);
                tn = std::max(tn, (gz.d[i].N + 63) / 64);
            }
            hipLaunchKernelGGL(tgemm_f32_mask_scale_kernel, dim3(tm, tn, kz), dim3(256), 0, st, gz);
            T_K((int)hipGetLastError());
        } else if (kz) {
            T_K((launch_tgemm<false, false, TEPI_MASK, TEPI_MASK>(gz, kz, st)));
        }
        if (kn) hipLaunchKernelGGL(bn_backward_kernel, dim3((nn + 63) / 64, 1, kn), dim3(256), 0, st, gn);
    }
    // gradient clipping: the clipping members' norm over every gW[l] / gb[l] (the L2 term is in gW), their coefficient to device
    // memory; the Adam stage reads it there, so nothing waits on the host
    bool clips = false;
    for (int i = 0; i < cnt; ++i) clips = clips || act[i].t->max_norm > 0.0;
    if (clips) {
        for (int l = 0; l < Lmax; ++l) {
            SumsqGroup gw, gb;
            int k = 0;
            for (int i = 0; i < cnt; ++i) {
                const mmc_trainer* t = act[i].t;
                if (!(t->max_norm > 0.0) || l >= t->L) continue;
                gw.d[k] = SumsqDesc{t->gW[l], t->gpartials + 256 * (2 * l), (size_t)t->dims[l + 1] * t->dims[l]};
                gb.d[k] = SumsqDesc{t->gb[l], t->gpartials + 256 * (2 * l + 1), (size_t)t->dims[l + 1]};
                ++k;
            }
            if (!k) continue;
            hipLaunchKernelGGL(sumsq_kernel, dim3(256, 1, k), dim3(256), 0, st, gw);
            hipLaunchKernelGGL(sumsq_kernel, dim3(256, 1, k), dim3(256), 0, st, gb);
        }
        {   // the normalised members' g_gamma / g_beta of every hidden layer: one more tensor, its partials after the layers'
            SumsqGroup gn;
            int kn = 0;
            for (int i = 0; i < cnt; ++i) {
                const mmc_trainer* t = act[i].t;
                if (t->max_norm > 0.0 && t->bn && t->bn_total)
                    gn.d[kn++] = SumsqDesc{t->bn_g, t->gpartials + 256 * (2 * t->L), (size_t)t->bn_total};
            }
            if (kn) hipLaunchKernelGGL(sumsq_kernel, dim3(256, 1, kn), dim3(256), 0, st, gn);
        }
        GnormGroup g;
        int k = 0;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            if (t->max_norm > 0.0)
                g.d[k++] = GnormDesc{t->gpartials, t->coef, t->gnorm + act[i].slot, 256 * (2 * t->L + (t->bn && t->bn_total ? 1 : 0)),
                                     (float)t->max_norm};
        }
        hipLaunchKernelGGL(gnorm_finalize_kernel, dim3(1, 1, k), dim3(256), 0, st, g);
    }
    float step_size[MMC_TRAINER_GROUP_MAX], bc2_sqrt[MMC_TRAINER_GROUP_MAX];
    for (int i = 0; i < cnt; ++i) {
        mmc_trainer* t = act[i].t;
        ++t->t;
        const double bc1 = 1.0 - std::pow(t->beta1, (double)t->t), bc2 = 1.0 - std::pow(t->beta2, (double)t->t);
        step_size[i] = (float)(trainer_lr_at(t, t->t) / bc1);
        bc2_sqrt[i] = (float)std::sqrt(bc2);
    }
    // the members that neither clip nor average go through adam_kernel, the others through adam_opt_kernel
    for (int l = 0; l < Lmax; ++l) {
        AdamGroup gw, gb;
        AdamOptGroup ow, ob;
        int k = 0, ko = 0;
        size_t wmax = 0, bmax = 0, owmax = 0, obmax = 0;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            if (l >= t->L) continue;
            const size_t nw = (size_t)t->dims[l + 1] * t->dims[l], nb = (size_t)t->dims[l + 1];
            const float om1 = (float)(1.0 - t->beta1), om2 = (float)(1.0 - t->beta2), b2f = (float)t->beta2, epsf = (float)t->eps;
            const bool ema = !t->sW.empty();
            if (t->max_norm > 0.0 || ema) {
                const float* coef = t->max_norm > 0.0 ? t->coef : nullptr;
                const float om_d = (float)(1.0 - t->ema_decay);
                ow.d[ko] = AdamOptDesc{t->W[l], t->gW[l], t->mW[l], t->vW[l], nw, om1, b2f, om2, epsf, step_size[i], bc2_sqrt[i],
                                       coef, ema ? t->sW[l] : nullptr, om_d};
                ob.d[ko] = AdamOptDesc{t->b[l], t->gb[l], t->mb[l], t->vb[l], nb, om1, b2f, om2, epsf, step_size[i], bc2_sqrt[i],
                                       coef, ema ? t->sb[l] : nullptr, om_d};
                ++ko;
                owmax = std::max(owmax, nw);
                obmax = std::max(obmax, nb);
                continue;
            }
            gw.d[k] = AdamDesc{t->W[l], t->gW[l], t->mW[l], t->vW[l], nw, om1, b2f, om2, epsf, step_size[i], bc2_sqrt[i]};
            gb.d[k] = AdamDesc{t->b[l], t->gb[l], t->mb[l], t->vb[l], nb, om1, b2f, om2, epsf, step_size[i], bc2_sqrt[i]};
            ++k;
            wmax = std::max(wmax, nw);
            bmax = std::max(bmax, nb);
        }
        if (k) {
            hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((wmax + 255) / 256), 1, k), dim3(256), 0, st, gw);
            hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((bmax + 255) / 256), 1, k), dim3(256), 0, st, gb);
        }
        if (ko) {
            hipLaunchKernelGGL(adam_opt_kernel, dim3((unsigned)((owmax + 255) / 256), 1, ko), dim3(256), 0, st, ow);
            hipLaunchKernelGGL(adam_opt_kernel, dim3((unsigned)((obmax + 255) / 256), 1, ko), dim3(256), 0, st, ob);
        }
    }
    {   // gamma and beta of the normalised members, every hidden layer at once: further descriptors of the same two kernels
        AdamGroup gn;
        AdamOptGroup on;
        int k = 0, ko = 0;
        size_t nmax = 0, onmax = 0;
        for (int i = 0; i < cnt; ++i) {
            mmc_trainer* t = act[i].t;
            if (!t->bn) continue;
            t->fold_stale = true;
            if (!t->bn_total) continue;
            const size_t n = (size_t)t->bn_total;
            const float om1 = (float)(1.0 - t->beta1), om2 = (float)(1.0 - t->beta2), b2f = (float)t->beta2, epsf = (float)t->eps;
            if (t->max_norm > 0.0) {
                on.d[ko++] = AdamOptDesc{t->bn_p, t->bn_g, t->bn_m, t->bn_v, n, om1, b2f, om2, epsf, step_size[i], bc2_sqrt[i], t->coef, nullptr, 0.f};
                onmax = std::max(onmax, n);
            } else {
                gn.d[k++] = AdamDesc{t->bn_p, t->bn_g, t->bn_m, t->bn_v, n, om1, b2f, om2, epsf, step_size[i], bc2_sqrt[i]};
                nmax = std::max(nmax, n);
            }
        }
        if (k) hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((nmax + 255) / 256), 1, k), dim3(256), 0, st, gn);
        if (ko) hipLaunchKernelGGL(adam_opt_kernel, dim3((unsigned)((onmax + 255) / 256), 1, ko), dim3(256), 0, st, on);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mmc_fail(MMC_ERR_HIP, "trainer step launch failed: %s", hipGetErrorString(e));
    return 0;
}

// rows of the mini-batch that starts at row `start` of a pass over n rows
int batch_rows(int64_t n, int64_t start, int mb) { return (int)((n - start) < mb ? (n - start) : mb); }

// wsums[s] = the class-weight sum of mini-batch s (the mean reduction of the weighted CE), whose i-th row carries the label
// y[idx ? idx[i] : i]; a mini-batch without weight is rejected.  Every pass calls this before it uploads or launches anything, so
// a rejected pass leaves the weights, the Adam moments and the step counter exactly as they were.
int minibatch_wsums(const char* who, const mmc_trainer* t, const int32_t* y, const int64_t* idx, int64_t n, int mb, std::vector<double>* wsums)
{
    const int steps = (int)((n + mb - 1) / mb);
    wsums->resize(steps);
    for (int s = 0; s < steps; ++s) {
        const int64_t start = (int64_t)s * mb;
        const int cur = batch_rows(n, start, mb);
        double wsum = 0.0;
        if (t->cw) { for (int i = 0; i < cur; ++i) wsum += t->cw_host[y[idx ? idx[start + i] : start + i]]; } else wsum = cur;
        if (!(wsum > 0.0)) return mmc_fail(MMC_ERR_ARG, "%smini-batch %d has zero total class weight", who, s);
        (*wsums)[s] = wsum;
    }
    return 0;
}

// minibatch_wsums of a mixed pass: position i carries lam w[ya] + oml w[yb] with ya = y[visit[i]], yb = y[partner[i]] and
// oml = 1.0f - lam[s], summed in double in row order
int minibatch_wsums_mixed(const char* who, const mmc_trainer* t, const int32_t* y, const int64_t* visit, const int64_t* partner,
                          const float* lam, int64_t n, int mb, std::vector<double>* wsums)
{
    const int steps = (int)((n + mb - 1) / mb);
    wsums->resize(steps);
    for (int s = 0; s < steps; ++s) {
        const int64_t start = (int64_t)s * mb;
        const int cur = batch_rows(n, start, mb);
        const double la = (double)lam[s], lb = (double)(1.0f - lam[s]);
        double wsum = 0.0;
        for (int i = 0; i < cur; ++i) {
            const double wa = t->cw ? (double)t->cw_host[y[visit ? visit[start + i] : start + i]] : 1.0;
            const double wb = t->cw ? (double)t->cw_host[y[partner[start + i]]] : 1.0;
            wsum += la * wa + lb * wb;
        }
        if (!(wsum > 0.0)) return mmc_fail(MMC_ERR_ARG, "%smini-batch %d has zero total mixed class weight", who, s);
        (*wsums)[s] = wsum;
    }
    return 0;
}

// minibatch_wsums of a weighted pass (include/mmc.h, "group-robust training"): position i carries the mass
// v_i = (double)rw[i] (double)w[y_i] (rw null: 1), summed in double in position order -- into wsums[s] without groups, into
// vmass[s G + rg[i]] with them (wsums[s] is then 1: the loss stage runs with g = 1).  Rejects a weight that is negative or not
// finite, a group outside [0, G), a mini-batch without mass or in which no group has mass.
int minibatch_masses(const char* who, const mmc_trainer* t, const int32_t* y, const int64_t* idx, const float* rw, const int32_t* rg, int G,
                     int64_t n, int mb, std::vector<double>* wsums, std::vector<double>* vmass)
{
    const int steps = (int)((n + mb - 1) / mb);
    for (int64_t i = 0; i < n; ++i) {
        if (rw && !(rw[i] >= 0.f && std::isfinite(rw[i])))
            return mmc_fail(MMC_ERR_ARG, "%srow_weight[%lld] = %g is negative or not finite", who, (long long)i, (double)rw[i]);
        if (rg && (rg[i] < 0 || rg[i] >= G))
            return mmc_fail(MMC_ERR_ARG, "%srow_group[%lld] = %d outside [0, %d)", who, (long long)i, rg[i], G);
    }
    wsums->assign(steps, 1.0);
    if (rg) vmass->assign((size_t)steps * G, 0.0);
    for (int s = 0; s < steps; ++s) {
        const int64_t start = (int64_t)s * mb;
        const int cur = batch_rows(n, start, mb);
        double wsum = 0.0;
        double* V = rg ? vmass->data() + (size_t)s * G : nullptr;
        for (int i = 0; i < cur; ++i) {
            const double w = t->cw ? (double)t->cw_host[y[idx ? idx[start + i] : start + i]] : 1.0;
            const double v = (rw ? (double)rw[start + i] : 1.0) * w;
            if (rg) V[rg[start + i]] += v; else wsum += v;
        }
        if (rg) {
            bool any = false;
            for (int a = 0; a < G; ++a) any = any || V[a] > 0.0;
            if (!any) return mmc_fail(MMC_ERR_ARG, "%sno group of mini-batch %d has mass", who, s);
        } else {
            if (!(wsum > 0.0)) return mmc_fail(MMC_ERR_ARG, "%smini-batch %d has zero total mass", who, s);
            (*wsums)[s] = wsum;
        }
    }
    return 0;
}

// torch_classifier.py:293-298: sum of loss.item() * mb_size over the steps, over n
double pass_avg_loss(const std::vector<float>& h, int mb, int64_t n)
{
    double tot = 0.0;
    for (size_t s = 0; s < h.size(); ++s) tot += (double)h[s] * (double)batch_rows(n, (int64_t)s * mb, mb);
    return tot / (double)n;
}

}  // namespace

// `order` (n int64 row indices, or NULL = rows are already in visiting order): the shuffle of torch_classifier.py:251-257 applied
// on the device -- the natural-order matrix is uploaded as it is and a gather kernel builds the visiting order (when the
// feature width is a multiple of 4; otherwise, and without `order`, the rows are taken as given).
extern "C" int mmc_trainer_partial_fit_ordered(mmc_trainer* t, const float* X, const int32_t* y, const int64_t* order, int64_t n,
                                               int batch_size, double* avg_loss, void* hip_stream)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!X || !y) return mmc_fail(MMC_ERR_ARG, "X/y is NULL");
    if (n < 1) return mmc_fail(MMC_ERR_ARG, "n = %lld must be positive", (long long)n);
    if (batch_size < 1) return mmc_fail(MMC_ERR_ARG, "batch_size = %d must be positive", batch_size);
    if (order && (t->dims[0] & 3)) return mmc_fail(MMC_ERR_ARG, "device-side ordering needs a feature width that is a multiple of 4 (got %d)", t->dims[0]);
    for (int64_t i = 0; i < n; ++i) {
        if (y[i] < 0 || y[i] >= t->K) return mmc_fail(MMC_ERR_ARG, "label index y[%lld] = %d outside [0, %d)", (long long)i, y[i], t->K);
        if (order && (order[i] < 0 || order[i] >= n)) return mmc_fail(MMC_ERR_ARG, "order[%lld] = %lld outside [0, %lld)", (long long)i, (long long)order[i], (long long)n);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(t->device));
    const int mb = (int)(batch_size < n ? batch_size : n);
    std::vector<double> wsums;
    int r = check_bn_minibatches("", t, n, mb);
    if (r) return r;
    if ((r = minibatch_wsums("", t, y, order, n, mb, &wsums))) return r;
    const int steps = (int)wsums.size();
    if ((r = trainer_reserve(t, n, mb, steps))) return r;
    if (order) {
        if ((r = t->Xn.reserve(n * t->dims[0])) || (r = t->yn.reserve(n)) || (r = t->order.reserve(n))) return r;
        HIP_TRY(hipMemcpyAsync(t->Xn, X, (size_t)n * t->dims[0] * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t->yn, y, (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t->order, order, (size_t)n * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)n), dim3(256), 0, st, t->Xn, t->yn, t->order, n, t->dims[0] / 4, t->X, t->y);
    } else {
        HIP_TRY(hipMemcpyAsync(t->X, X, (size_t)n * t->dims[0] * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t->y, y, (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    for (int s = 0; s < steps; ++s) {
        const int64_t start = (int64_t)s * mb;
        const StepMember one{t, start, batch_rows(n, start, mb), (float)(1.0 / wsums[s]), s, false, 0.f};
        if ((r = trainer_group_step(&one, 1, st))) return r;
    }
    t->gnorm_steps = t->max_norm > 0.0 ? steps : 0;
    std::vector<float> h(steps);
    HIP_TRY(hipMemcpyAsync(h.data(), t->losses, (size_t)steps * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (avg_loss) *avg_loss = pass_avg_loss(h, mb, n);
    return MMC_OK;
}

extern "C" int mmc_trainer_partial_fit(mmc_trainer* t, const float* X, const int32_t* y, int64_t n, int batch_size, double* avg_loss,
                                       void* hip_stream)
{
    return mmc_trainer_partial_fit_ordered(t, X, y, nullptr, n, batch_size, avg_loss, hip_stream);
}

// ---- passes over a resident feature set -----------------------------------------------------------------------------------
namespace {

// how one trainer takes one pass over rows of a set: mini-batch, steps, its chunks of whole mini-batches, every step's weight sum
struct SetPass {
    mmc_trainer* t = nullptr;
    const int64_t* visit = nullptr;
    const int64_t* partner = nullptr;   // a mixed pass: partner rows and one lam per mini-batch (both or neither)
    const float* lam = nullptr;
    const float* row_weight = nullptr;  // a weighted pass: either or both, by position
    const int32_t* row_group = nullptr;
    int64_t n = 0;
    int mb = 0, steps = 0;
    int64_t chunk = 0, steps_per_chunk = 0, stage_rows = 0;
    std::vector<double> wsums;
    std::vector<double> vmass;          // [steps][n_groups] of a pass with groups
};

// `who` prefixes the message: "" for the solo call, "member 3: " for a member of a group
int check_set_pass(const char* who, const mmc_trainer* t, const mmc_featureset* fs, const int64_t* visit, int64_t n, int batch_size)
{
    if (fs->dim != t->dims[0]) return mmc_fail(MMC_ERR_ARG, "%sfeature set has %d columns, trainer expects %d", who, fs->dim, t->dims[0]);
    if (fs->K != t->K) return mmc_fail(MMC_ERR_ARG, "%sfeature set has %d classes, trainer %d", who, fs->K, t->K);
    if (fs->device != t->device) return mmc_fail(MMC_ERR_ARG, "%sfeature set is on device %d, trainer on device %d", who, fs->device, t->device);
    if (n < 1) return mmc_fail(MMC_ERR_ARG, "%sn = %lld must be positive", who, (long long)n);
    if (batch_size < 1) return mmc_fail(MMC_ERR_ARG, "%sbatch_size = %d must be positive", who, batch_size);
    if (!visit && n != fs->n) return mmc_fail(MMC_ERR_ARG, "%swithout a visiting order n must be the set's %lld rows (got %lld)", who, (long long)fs->n, (long long)n);
    if (visit)
        for (int64_t i = 0; i < n; ++i)
            if (visit[i] < 0 || visit[i] >= fs->n)
                return mmc_fail(MMC_ERR_ARG, "%svisit[%lld] = %lld outside [0, %lld)", who, (long long)i, (long long)visit[i], (long long)fs->n);
    return 0;
}

// the plan of a mixed pass: both arrays or neither, every partner a row of the set, every lam in [0, 1]
int check_mix_plan(const char* who, const mmc_featureset* fs, const int64_t* partner, const float* lam, int64_t n, int batch_size)
{
    if (!partner && !lam) return 0;
    if (!partner || !lam) return mmc_fail(MMC_ERR_ARG, "%spartner and lam go together: only %s was given", who, partner ? "partner" : "lam");
    for (int64_t i = 0; i < n; ++i)
        if (partner[i] < 0 || partner[i] >= fs->n)
            return mmc_fail(MMC_ERR_ARG, "%spartner[%lld] = %lld outside [0, %lld)", who, (long long)i, (long long)partner[i], (long long)fs->n);
    const int64_t mb = batch_size < n ? batch_size : n, steps = (n + mb - 1) / mb;
    for (int64_t s = 0; s < steps; ++s)
        if (!(lam[s] >= 0.f && lam[s] <= 1.f)) return mmc_fail(MMC_ERR_ARG, "%slam[%lld] = %g outside [0, 1]", who, (long long)s, (double)lam[s]);
    return 0;
}

int train_chunk_bound(int64_t* bound)
{
    *bound = MMC_TRAIN_CHUNK_ROWS_DEFAULT;
    if (const char* env = std::getenv("MMC_TRAIN_CHUNK_ROWS")) {
        char* end = nullptr;
        const long long v = std::strtoll(env, &end, 10);
        if (end == env || *end || v < 1) return mmc_fail(MMC_ERR_ARG, "MMC_TRAIN_CHUNK_ROWS = '%s' is not a positive integer", env);
        *bound = v;
    }
    return 0;
}

int plan_set_pass(const char* who, mmc_trainer* t, const mmc_featureset* fs, const int64_t* visit, const int64_t* partner,
                  const float* lam, const float* row_weight, const int32_t* row_group, int64_t n, int batch_size, int64_t bound, SetPass* p)
{
    const int mb = (int)(batch_size < n ? batch_size : n);
    if ((n + mb - 1) / mb > (int64_t)1 << 30) return mmc_fail(MMC_ERR_ARG, "%s%lld rows in mini-batches of %d: too many steps for one pass", who, (long long)n, mb);
    p->t = t; p->visit = visit; p->partner = partner; p->lam = lam; p->n = n;
    p->row_weight = row_weight; p->row_group = row_group;
    p->mb = mb;
    p->steps = (int)((n + mb - 1) / mb);
    // the largest multiple of the mini-batch not above the bound, at least one mini-batch, and no more than a gather's grid / `rows` hold
    int64_t chunk = bound / mb * mb;
    if (chunk < mb) chunk = mb;
    const int64_t chunk_max = ((int64_t)1 << 30) / mb * mb;
    if (chunk > chunk_max) chunk = chunk_max;
    p->chunk = chunk;
    p->steps_per_chunk = chunk / mb;
    p->stage_rows = chunk < n ? chunk : n;
    if (partner) return minibatch_wsums_mixed(who, t, fs->y_host.data(), visit, partner, lam, n, mb, &p->wsums);
    if (row_weight || row_group)
        return minibatch_masses(who, t, fs->y_host.data(), visit, row_weight, row_group, t->n_groups, n, mb, &p->wsums, &p->vmass);
    return minibatch_wsums(who, t, fs->y_host.data(), visit, n, mb, &p->wsums);
}

// the trainer's staging, activations and loss slots for the pass, and its device copy of the visiting order (not yet uploaded)
int reserve_set_pass(const SetPass& p)
{
    mmc_trainer* t = p.t;
    int r = trainer_reserve(t, p.stage_rows, p.mb, p.steps);
    if (r) return r;
    if (p.visit && (r = t->visit.reserve(p.n))) return r;
    if (p.partner && ((r = t->y2.reserve(p.stage_rows)) || (r = t->partner.reserve(p.n)) || (r = t->lam.reserve(p.steps)))) return r;
    if (p.row_weight && (r = t->row_w.reserve(p.n))) return r;
    if (p.row_group && ((r = t->row_g.reserve(p.n)) || (r = t->group_mass.reserve((int64_t)p.steps * t->n_groups)) || (r = t->row_scale.reserve(p.mb))))
        return r;
    return 0;
}

// rows [c0, c0 + rows) of the pass into the staging t->X / t->y
int gather_chunk(mmc_trainer* t, const mmc_featureset* fs, bool visited, bool mixed, int mb, int64_t c0, int rows, hipStream_t st)
{
    const int64_t* vis = visited ? t->visit + c0 : nullptr;
    if (mixed) {   // c0 is a multiple of mb: the chunk's first mini-batch is c0 / mb of the pass
        const int64_t* par = t->partner + c0;
        const float* lam = t->lam + c0 / mb;
        if (fs->dim & 3)
            hipLaunchKernelGGL(gather_set_rows_mixed_kernel<false>, dim3((rows + 3) / 4), dim3(256), 0, st, fs->X, fs->y, vis, c0, par, lam, mb,
                               rows, fs->dim, t->X, t->y, t->y2);
        else
            hipLaunchKernelGGL(gather_set_rows_mixed_kernel<true>, dim3((rows + 3) / 4), dim3(256), 0, st, fs->X, fs->y, vis, c0, par, lam, mb,
                               rows, fs->dim, t->X, t->y, t->y2);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (fs->dim & 3)
        hipLaunchKernelGGL(gather_set_rows_kernel<false>, dim3((rows + 3) / 4), dim3(256), 0, st, fs->X, fs->y, vis, c0, rows, fs->dim, t->X, t->y);
    else
        hipLaunchKernelGGL(gather_set_rows_kernel<true>, dim3((rows + 3) / 4), dim3(256), 0, st, fs->X, fs->y, vis, c0, rows, fs->dim, t->X, t->y);
    HIP_TRY(hipGetLastError());
    return 0;
}

// One pass of `count` trainers over rows of `fs`, step s of every member's pass issued together: position i of member m visits row
// visit[m][i].  Nothing but the visiting orders is uploaded.  A member's visited rows and labels are gathered into its mini-batch
// staging (t->X / t->y) a chunk of whole mini-batches at a time, and that chunk's steps follow on the same stream, so the steps
// run the kernels of the host-fed pass on the same values: same bits.  `grouped` is the entry point's way of naming a member and of
// reporting a failed reservation; the solo entry is a group of one that names nobody.
int set_pass(bool grouped, mmc_trainer* const* trainers, int count, mmc_featureset* fs, const int64_t* const* visit,
             const int64_t* const* partner, const float* const* lam, const float* const* row_weight, const int32_t* const* row_group,
             const int64_t* n, const int* batch_size, double* avg_loss, hipStream_t st)
{
    std::vector<SetPass> mem(count);
    char who[MMC_TRAINER_GROUP_MAX][32];
    int r = 0;
    for (int m = 0; m < count; ++m) {
        who[m][0] = 0;
        if (grouped) std::snprintf(who[m], sizeof who[m], "member %d: ", m);
        if ((r = check_set_pass(who[m], trainers[m], fs, visit[m], n[m], batch_size[m]))) return r;
        if ((r = check_mix_plan(who[m], fs, partner ? partner[m] : nullptr, lam ? lam[m] : nullptr, n[m], batch_size[m]))) return r;
        if ((r = check_bn_minibatches(who[m], trainers[m], n[m], (int)(batch_size[m] < n[m] ? batch_size[m] : n[m])))) return r;
        const bool weighted = (row_weight && row_weight[m]) || (row_group && row_group[m]);
        if (weighted && partner && partner[m]) return mmc_fail(MMC_ERR_ARG, "%sa mixed pass takes no row weights or groups", who[m]);
        if (partner && partner[m] && trainers[m]->hier)
            return mmc_fail(MMC_ERR_ARG, "%sa mixed pass takes no hierarchy (mmc_trainer_set_hierarchy)", who[m]);
        if (row_group && row_group[m] && !trainers[m]->n_groups)
            return mmc_fail(MMC_ERR_ARG, "%srow_group needs mmc_trainer_set_group_dro(n_groups > 0) on the trainer", who[m]);
    }
    int64_t bound = 0;
    if ((r = train_chunk_bound(&bound))) return r;
    int max_steps = 0;
    for (int m = 0; m < count; ++m) {
        if ((r = plan_set_pass(who[m], trainers[m], fs, visit[m], partner ? partner[m] : nullptr, lam ? lam[m] : nullptr,
                               row_weight ? row_weight[m] : nullptr, row_group ? row_group[m] : nullptr, n[m], batch_size[m], bound, &mem[m])))
            return r;
        max_steps = std::max(max_steps, mem[m].steps);
    }
    HIP_TRY(hipSetDevice(fs->device));
    // every member's buffers before the first launch: a pass that cannot be staged changes no member
    for (int m = 0; m < count; ++m)
        if ((r = reserve_set_pass(mem[m]))) {
            if (!grouped) return r;
            (void)hipGetLastError();
            return mmc_fail(MMC_ERR_NOMEM, "member %d: could not allocate the buffers of its pass (%lld staged rows, mini-batch %d)", m,
                            (long long)mem[m].stage_rows, mem[m].mb);
        }
    for (int m = 0; m < count; ++m)
        if (mem[m].visit) HIP_TRY(hipMemcpyAsync(mem[m].t->visit, mem[m].visit, (size_t)mem[m].n * 8, hipMemcpyHostToDevice, st));
    for (int m = 0; m < count; ++m)
        if (mem[m].partner) {
            HIP_TRY(hipMemcpyAsync(mem[m].t->partner, mem[m].partner, (size_t)mem[m].n * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(mem[m].t->lam, mem[m].lam, (size_t)mem[m].steps * 4, hipMemcpyHostToDevice, st));
        }
    for (int m = 0; m < count; ++m) {
        const SetPass& p = mem[m];
        if (p.row_weight) HIP_TRY(hipMemcpyAsync(p.t->row_w, p.row_weight, (size_t)p.n * 4, hipMemcpyHostToDevice, st));
        if (p.row_group) {
            HIP_TRY(hipMemcpyAsync(p.t->row_g, p.row_group, (size_t)p.n * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(p.t->group_mass, p.vmass.data(), p.vmass.size() * 8, hipMemcpyHostToDevice, st));
        }
    }
    StepMember act[MMC_TRAINER_GROUP_MAX];
    for (int s = 0; s < max_steps; ++s) {
        int cnt = 0;
        for (int m = 0; m < count; ++m) {
            const SetPass& p = mem[m];
            if (s >= p.steps) continue;   // this member's pass is over
            const int64_t start = (int64_t)s * p.mb, c0 = s / p.steps_per_chunk * p.chunk;
            if (start == c0) {            // its first step of a chunk: stage the chunk's rows first
                const int rows = (int)((p.n - c0) < p.chunk ? (p.n - c0) : p.chunk);
                if ((r = gather_chunk(p.t, fs, p.visit != nullptr, p.partner != nullptr, p.mb, c0, rows, st))) return r;
            }
            act[cnt] = StepMember{p.t, start - c0, batch_rows(p.n, start, p.mb), (float)(1.0 / p.wsums[s]), s, p.partner != nullptr,
                                  p.partner ? p.lam[s] : 0.f};
            if (p.row_weight || p.row_group) {   // the pass's arrays are indexed by position of the pass, not of the chunk
                act[cnt].weighted = true;
                act[cnt].rw = p.row_weight ? p.t->row_w + start : nullptr;
                act[cnt].rg = p.row_group ? p.t->row_g + start : nullptr;
                act[cnt].V = p.row_group ? p.t->group_mass + (size_t)s * p.t->n_groups : nullptr;
            }
            ++cnt;
        }
        if ((r = trainer_group_step(act, cnt, st))) return r;
    }
    for (int m = 0; m < count; ++m) mem[m].t->gnorm_steps = mem[m].t->max_norm > 0.0 ? mem[m].steps : 0;
    std::vector<std::vector<float>> h(count);
    for (int m = 0; m < count; ++m) {
        h[m].resize(mem[m].steps);
        HIP_TRY(hipMemcpyAsync(h[m].data(), mem[m].t->losses, (size_t)mem[m].steps * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (avg_loss)
        for (int m = 0; m < count; ++m) avg_loss[m] = pass_avg_loss(h[m], mem[m].mb, mem[m].n);
    return MMC_OK;
}

}  // namespace

// The pass of mmc_trainer_partial_fit_ordered over rows that are already on the device: a group of one (include/mmc.h).
extern "C" int mmc_trainer_partial_fit_set(mmc_trainer* t, mmc_featureset* fs, const int64_t* visit, int64_t n, int batch_size,
                                           double* avg_loss, void* hip_stream)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!fs) return mmc_fail(MMC_ERR_ARG, "feature set handle is NULL");
    return set_pass(false, &t, 1, fs, &visit, nullptr, nullptr, nullptr, nullptr, &n, &batch_size, avg_loss, static_cast<hipStream_t>(hip_stream));
}

// mmc_trainer_partial_fit_set on mixed rows (include/mmc.h, "regularisers"); NULL partner and lam: that call itself.
extern "C" int mmc_trainer_partial_fit_set_mixed(mmc_trainer* t, mmc_featureset* fs, const int64_t* visit, const int64_t* partner,
                                                 const float* lam, int64_t n, int batch_size, double* avg_loss, void* hip_stream)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!fs) return mmc_fail(MMC_ERR_ARG, "feature set handle is NULL");
    return set_pass(false, &t, 1, fs, &visit, &partner, &lam, nullptr, nullptr, &n, &batch_size, avg_loss, static_cast<hipStream_t>(hip_stream));
}

// mmc_trainer_partial_fit_set for `count` trainers over one set in the launches of one pass (include/mmc.h).
extern "C" int mmc_trainer_group_partial_fit_set(mmc_trainer* const* trainers, int count, mmc_featureset* fs, const int64_t* const* visit,
                                                 const int64_t* n, const int* batch_size, double* avg_loss, void* hip_stream)
{
    return mmc_trainer_group_partial_fit_set_mixed(trainers, count, fs, visit, nullptr, nullptr, n, batch_size, avg_loss, hip_stream);
}

// The grouped pass with a mixing plan per member (include/mmc.h, "regularisers"): partner / lam are arrays of `count` pointers, or
// NULL for a pass in which nobody is mixed; a member whose two entries are NULL is not mixed.
extern "C" int mmc_trainer_group_partial_fit_set_mixed(mmc_trainer* const* trainers, int count, mmc_featureset* fs,
                                                       const int64_t* const* visit, const int64_t* const* partner, const float* const* lam,
                                                       const int64_t* n, const int* batch_size, double* avg_loss, void* hip_stream)
{
    if (avg_loss && count >= 1 && count <= MMC_TRAINER_GROUP_MAX)
        for (int m = 0; m < count; ++m) avg_loss[m] = 0.0;
    if (!trainers || !visit || !n || !batch_size) return mmc_fail(MMC_ERR_ARG, "trainers / visit / n / batch_size is NULL");
    if (count < 1 || count > MMC_TRAINER_GROUP_MAX) return mmc_fail(MMC_ERR_ARG, "count = %d outside [1, %d]", count, MMC_TRAINER_GROUP_MAX);
    for (int m = 0; m < count; ++m) {
        if (!trainers[m]) return mmc_fail(MMC_ERR_ARG, "member %d: trainer handle is NULL", m);
        for (int o = 0; o < m; ++o)
            if (trainers[o] == trainers[m]) return mmc_fail(MMC_ERR_ARG, "member %d is the same trainer as member %d", m, o);
    }
    if (!fs) return mmc_fail(MMC_ERR_ARG, "feature set handle is NULL");
    if (!partner != !lam) return mmc_fail(MMC_ERR_ARG, "partner and lam go together: only %s was given", partner ? "partner" : "lam");
    return set_pass(true, trainers, count, fs, visit, partner, lam, nullptr, nullptr, n, batch_size, avg_loss, static_cast<hipStream_t>(hip_stream));
}

// mmc_trainer_partial_fit_set with per-row weights and / or groups (include/mmc.h, "group-robust training"); both NULL: that call.
extern "C" int mmc_trainer_partial_fit_set_weighted(mmc_trainer* t, mmc_featureset* fs, const int64_t* visit, const float* row_weight,
                                                    const int32_t* row_group, int64_t n, int batch_size, double* avg_loss, void* hip_stream)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!fs) return mmc_fail(MMC_ERR_ARG, "feature set handle is NULL");
    return set_pass(false, &t, 1, fs, &visit, nullptr, nullptr, &row_weight, &row_group, &n, &batch_size, avg_loss,
                    static_cast<hipStream_t>(hip_stream));
}

// The grouped pass with weights and groups per member: arrays of `count` pointers, or NULL; a member whose two entries are NULL
// takes the plain kernels.
extern "C" int mmc_trainer_group_partial_fit_set_weighted(mmc_trainer* const* trainers, int count, mmc_featureset* fs,
                                                          const int64_t* const* visit, const float* const* row_weight,
                                                          const int32_t* const* row_group, const int64_t* n, const int* batch_size,
                                                          double* avg_loss, void* hip_stream)
{
    if (avg_loss && count >= 1 && count <= MMC_TRAINER_GROUP_MAX)
        for (int m = 0; m < count; ++m) avg_loss[m] = 0.0;
    if (!trainers || !visit || !n || !batch_size) return mmc_fail(MMC_ERR_ARG, "trainers / visit / n / batch_size is NULL");
    if (count < 1 || count > MMC_TRAINER_GROUP_MAX) return mmc_fail(MMC_ERR_ARG, "count = %d outside [1, %d]", count, MMC_TRAINER_GROUP_MAX);
    for (int m = 0; m < count; ++m) {
        if (!trainers[m]) return mmc_fail(MMC_ERR_ARG, "member %d: trainer handle is NULL", m);
        for (int o = 0; o < m; ++o)
            if (trainers[o] == trainers[m]) return mmc_fail(MMC_ERR_ARG, "member %d is the same trainer as member %d", m, o);
    }
    if (!fs) return mmc_fail(MMC_ERR_ARG, "feature set handle is NULL");
    return set_pass(true, trainers, count, fs, visit, nullptr, nullptr, row_weight, row_group, n, batch_size, avg_loss,
                    static_cast<hipStream_t>(hip_stream));
}

extern "C" int mmc_trainer_get_params(mmc_trainer* t, float* const* W, float* const* b)
{
    if (!t || !W || !b) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipDeviceSynchronize());
    for (int l = 0; l < t->L; ++l) {
        HIP_TRY(hipMemcpy(W[l], t->W[l], (size_t)t->dims[l + 1] * t->dims[l] * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(b[l], t->b[l], (size_t)t->dims[l + 1] * 4, hipMemcpyDeviceToHost));
    }
    return MMC_OK;
}

// Optimizer state for pickling (torch_classifier.py:404-415 serialises module + optimizer state dicts):
// which = 0: exp_avg, 1: exp_avg_sq.  `set` != 0 uploads instead.  *step is read / written alike.
extern "C" int mmc_trainer_adam_state(mmc_trainer* t, int which, int set, float* const* W, float* const* b, long long* step)
{
    if (!t || !W || !b || !step) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    if (which != 0 && which != 1) return mmc_fail(MMC_ERR_ARG, "which must be 0 (exp_avg) or 1 (exp_avg_sq)");
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipDeviceSynchronize());
    for (int l = 0; l < t->L; ++l) {
        float* dw = which == 0 ? t->mW[l] : t->vW[l];
        float* db = which == 0 ? t->mb[l] : t->vb[l];
        const size_t nw = (size_t)t->dims[l + 1] * t->dims[l] * 4, nb = (size_t)t->dims[l + 1] * 4;
        if (set) { HIP_TRY(hipMemcpy(dw, W[l], nw, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(db, b[l], nb, hipMemcpyHostToDevice)); }
        else { HIP_TRY(hipMemcpy(W[l], dw, nw, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(b[l], db, nb, hipMemcpyDeviceToHost)); }
    }
    if (set) t->t = *step; else *step = t->t;
    return MMC_OK;
}

// forward of the current parameters (eval mode) on n <= kTrainerForwardRows host rows: uploads X into the trainer's input buffer
// and leaves the logits [n][K] in its last activation buffer (valid until the next call on `t`)
int trainer_forward(mmc_trainer* t, const float* X, int n, hipStream_t st, const float** logits)
{
    if (n < 1 || n > kTrainerForwardRows) return mmc_fail(MMC_ERR_ARG, "trainer_forward: n = %d outside [1, %d]", n, kTrainerForwardRows);
    HIP_TRY(hipSetDevice(t->device));
    int r = trainer_reserve(t, n, n, 1);
    if (r) return r;
    HIP_TRY(hipMemcpyAsync(t->X, X, (size_t)n * t->dims[0] * 4, hipMemcpyHostToDevice, st));
    return trainer_forward_device(t, t->X, n, st, logits);
}

int trainer_forward_device(mmc_trainer* t, const float* X_dev, int n, hipStream_t st, const float** logits)
{
    if (n < 1 || n > kTrainerForwardRows) return mmc_fail(MMC_ERR_ARG, "trainer_forward: n = %d outside [1, %d]", n, kTrainerForwardRows);
    HIP_TRY(hipSetDevice(t->device));
    int r = trainer_reserve(t, 0, n, 1);   // activations only: the input is read where it lies
    if (r) return r;
    t->H[0] = const_cast<float*>(X_dev);
    if ((r = trainer_refresh_fold(t, st))) return r;   // a normalised trainer: W' / b' of its hidden layers, if a step has moved them
    for (int l = 0; l < t->L; ++l) {
        GemmGroup g;
        g.d[0] = forward_desc(t, l, n);
        if (t->eval_which == MMC_WEIGHTS_AVERAGED) {   // mmc_trainer_eval_weights: the same launch on the shadow
            g.d[0].B = t->sW[l];
            g.d[0].aux = t->sb[l];
        }
        if (t->bn && l < t->L - 1) {   // and on the folded layers: relu(W' x + b') is the frozen-statistics layer
            g.d[0].B = t->fW[l];
            g.d[0].aux = t->fb[l];
        }
        T_K((launch_tgemm<false, true, TEPI_BIAS_RELU, TEPI_BIAS>(g, 1, st)));
    }
    *logits = t->H[t->L];
    return MMC_OK;
}

int trainer_scratch(mmc_trainer* t, size_t bytes, void** out)
{
    if ((int64_t)bytes > t->scratch.cap) {   // only on growth: the buffer is kept for the trainer's lifetime
        HIP_TRY(hipSetDevice(t->device));
        if (int r = t->scratch.reserve((int64_t)bytes)) return r;
    }
    *out = t->scratch.p;
    return MMC_OK;
}

int trainer_classes(const mmc_trainer* t) { return t->K; }
int trainer_input_dim(const mmc_trainer* t) { return t->dims[0]; }
int trainer_device(const mmc_trainer* t) { return t->device; }

// logits of the current parameters (eval mode): X n x dims[0] host -> logits n x K host
extern "C" int mmc_trainer_logits(mmc_trainer* t, const float* X, int64_t n, float* logits, void* hip_stream)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (n < 0) return mmc_fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    if (n == 0) return MMC_OK;
    if (!X || !logits) return mmc_fail(MMC_ERR_ARG, "X/logits is NULL");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    for (int64_t off = 0; off < n; off += kTrainerForwardRows) {
        const int cur = (int)((n - off) < kTrainerForwardRows ? (n - off) : kTrainerForwardRows);
        const float* z = nullptr;
        int r = trainer_forward(t, X + (size_t)off * t->dims[0], cur, st, &z);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(logits + (size_t)off * t->K, z, (size_t)cur * t->K * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return MMC_OK;
}

// the loss stage of a step on caller logits: the step's kernel, class weights, loss options and 1 / sum of w[y_i] (include/mmc.h)
extern "C" int mmc_trainer_loss_gradient(mmc_trainer* t, const float* logits, const int32_t* y, int64_t n, float* dlogits, float* row_loss,
                                         void* hip_stream)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!logits || !y || !dlogits || !row_loss) return mmc_fail(MMC_ERR_ARG, "logits / y / dlogits / row_loss is NULL");
    if (n < 1 || n > kTrainerForwardRows) return mmc_fail(MMC_ERR_ARG, "n = %lld outside [1, %d]", (long long)n, kTrainerForwardRows);
    double wsum = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (y[i] < 0 || y[i] >= t->K) return mmc_fail(MMC_ERR_ARG, "label index y[%lld] = %d outside [0, %d)", (long long)i, y[i], t->K);
        wsum += t->cw ? (double)t->cw_host[y[i]] : 1.0;
    }
    if (!(wsum > 0.0)) return mmc_fail(MMC_ERR_ARG, "the rows have zero total class weight");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(t->device));
    const int mb = (int)n, L = t->L;
    int r = trainer_reserve(t, 0, mb, 1);   // the step's own logits / gradient / row-loss buffers
    if (r) return r;
    void* yd = nullptr;
    if ((r = trainer_scratch(t, (size_t)mb * 4, &yd))) return r;
    const size_t cells = (size_t)mb * t->K;
    HIP_TRY(hipMemcpyAsync(t->H[L], logits, cells * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(yd, y, (size_t)mb * 4, hipMemcpyHostToDevice, st));
    if (t->hier) {   // the kernel a step of this trainer runs
        CeHierGroup g;
        g.d[0] = CeHierDesc{ce_desc(t, t->H[L], static_cast<const int32_t*>(yd), mb, (float)(1.0 / wsum)), nullptr, trainer_hier_loss(t)};
        hipLaunchKernelGGL(ce_grad_hier_kernel, dim3((mb + 3) / 4), dim3(256), 0, st, g);
    } else {
        CeGroup g;
        g.d[0] = ce_desc(t, t->H[L], static_cast<const int32_t*>(yd), mb, (float)(1.0 / wsum));
        hipLaunchKernelGGL(ce_grad_kernel, dim3((mb + 3) / 4), dim3(256), 0, st, g);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dlogits, t->dZ[L], cells * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(row_loss, t->row_loss, (size_t)mb * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MMC_OK;
}

// mmc_trainer_loss_gradient for the mixed instantiation: two targets per row and one lam for all rows (include/mmc.h, "regularisers")
extern "C" int mmc_trainer_loss_gradient_mixed(mmc_trainer* t, const float* logits, const int32_t* y, const int32_t* y2, float lam, int64_t n,
                                               float* dlogits, float* row_loss, void* hip_stream)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!logits || !y || !y2 || !dlogits || !row_loss) return mmc_fail(MMC_ERR_ARG, "logits / y / y2 / dlogits / row_loss is NULL");
    if (n < 1 || n > kTrainerForwardRows) return mmc_fail(MMC_ERR_ARG, "n = %lld outside [1, %d]", (long long)n, kTrainerForwardRows);
    if (!(lam >= 0.f && lam <= 1.f)) return mmc_fail(MMC_ERR_ARG, "lam = %g outside [0, 1]", (double)lam);
    if (t->hier) return mmc_fail(MMC_ERR_ARG, "a mixed loss stage takes no hierarchy (mmc_trainer_set_hierarchy)");
    const float oml = 1.0f - lam;
    double wsum = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (y[i] < 0 || y[i] >= t->K) return mmc_fail(MMC_ERR_ARG, "label index y[%lld] = %d outside [0, %d)", (long long)i, y[i], t->K);
        if (y2[i] < 0 || y2[i] >= t->K) return mmc_fail(MMC_ERR_ARG, "label index y2[%lld] = %d outside [0, %d)", (long long)i, y2[i], t->K);
        wsum += (double)lam * (t->cw ? (double)t->cw_host[y[i]] : 1.0) + (double)oml * (t->cw ? (double)t->cw_host[y2[i]] : 1.0);
    }
    if (!(wsum > 0.0)) return mmc_fail(MMC_ERR_ARG, "the rows have zero total mixed class weight");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(t->device));
    const int mb = (int)n, L = t->L;
    int r = trainer_reserve(t, 0, mb, 1);
    if (r) return r;
    void* yd = nullptr;
    if ((r = trainer_scratch(t, (size_t)mb * 8, &yd))) return r;
    int32_t* y1d = static_cast<int32_t*>(yd);
    int32_t* y2d = y1d + mb;
    const size_t cells = (size_t)mb * t->K;
    HIP_TRY(hipMemcpyAsync(t->H[L], logits, cells * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(y1d, y, (size_t)mb * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(y2d, y2, (size_t)mb * 4, hipMemcpyHostToDevice, st));
    CeMixGroup g;
    g.d[0] = CeMixDesc{t->H[L], y1d, y2d, t->cw, t->dZ[L], t->row_loss, mb, t->K, (float)(1.0 / wsum), lam, oml, trainer_ce_loss(t)};
    hipLaunchKernelGGL(ce_grad_mixed_kernel, dim3((mb + 3) / 4), dim3(256), 0, st, g);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dlogits, t->dZ[L], cells * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(row_loss, t->row_loss, (size_t)mb * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MMC_OK;
}

// The weighted loss stage of a step on caller logits and an explicit log q (include/mmc.h, "group-robust training"): the step's own
// kernels -- ce_grad_weighted_kernel, then with groups dro_update_kernel and row_scale_kernel -- on buffers of the trainer's scratch.
// The trainer's own distribution is neither read nor written.
extern "C" int mmc_trainer_loss_gradient_weighted(mmc_trainer* t, const float* logits, const int32_t* y, const float* row_weight,
                                                  const int32_t* row_group, const double* log_q_in, double eta, int n_groups, int64_t n,
                                                  float* dlogits, float* row_loss, double* log_q_out, double* group_loss, void* hip_stream)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!logits || !y || !dlogits || !row_loss) return mmc_fail(MMC_ERR_ARG, "logits / y / dlogits / row_loss is NULL");
    if (n < 1 || n > kTrainerForwardRows) return mmc_fail(MMC_ERR_ARG, "n = %lld outside [1, %d]", (long long)n, kTrainerForwardRows);
    const int G = row_group ? n_groups : 0;
    if (row_group) {
        if (n_groups < 1 || n_groups > MMC_DRO_MAX_GROUPS) return mmc_fail(MMC_ERR_ARG, "n_groups = %d outside [1, %d]", n_groups, MMC_DRO_MAX_GROUPS);
        if (!(eta >= 0.0 && eta <= 10.0)) return mmc_fail(MMC_ERR_ARG, "eta = %g outside [0, 10]", eta);
        if (!log_q_in || !log_q_out) return mmc_fail(MMC_ERR_ARG, "row_group needs log_q_in and log_q_out");
        for (int a = 0; a < G; ++a)
            if (!std::isfinite(log_q_in[a])) return mmc_fail(MMC_ERR_ARG, "log_q_in[%d] = %g is not finite", a, log_q_in[a]);
    }
    for (int64_t i = 0; i < n; ++i)
        if (y[i] < 0 || y[i] >= t->K) return mmc_fail(MMC_ERR_ARG, "label index y[%lld] = %d outside [0, %d)", (long long)i, y[i], t->K);
    const int mb = (int)n, L = t->L;
    std::vector<double> wsums, vmass;
    int r = minibatch_masses("", t, y, nullptr, row_weight, row_group, G, n, mb, &wsums, &vmass);
    if (r) return r;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(t->device));
    if ((r = trainer_reserve(t, 0, mb, 1))) return r;
    // scratch: V [G] and log q [G] and group loss [G] in double first (8-byte aligned), then y, groups, weights and c by row
    void* sc = nullptr;
    if ((r = trainer_scratch(t, (size_t)G * 24 + (size_t)mb * 16, &sc))) return r;
    double* Vd = static_cast<double*>(sc);
    double* lqd = Vd + G;
    double* gld = lqd + G;
    int32_t* yd = reinterpret_cast<int32_t*>(gld + G);
    int32_t* gd = yd + mb;
    float* wd = reinterpret_cast<float*>(gd + mb);
    float* cd = wd + mb;
    const size_t cells = (size_t)mb * t->K;
    HIP_TRY(hipMemcpyAsync(t->H[L], logits, cells * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(yd, y, (size_t)mb * 4, hipMemcpyHostToDevice, st));
    if (row_weight) HIP_TRY(hipMemcpyAsync(wd, row_weight, (size_t)mb * 4, hipMemcpyHostToDevice, st));
    if (t->hier) {
        CeHierGroup g;
        g.d[0] = CeHierDesc{ce_desc(t, t->H[L], yd, mb, (float)(1.0 / wsums[0])), row_weight ? wd : nullptr, trainer_hier_loss(t)};
        hipLaunchKernelGGL(ce_grad_hier_kernel, dim3((mb + 3) / 4), dim3(256), 0, st, g);
    } else {
        CeRowGroup g;
        g.d[0] = CeRowDesc{ce_desc(t, t->H[L], yd, mb, (float)(1.0 / wsums[0])), row_weight ? wd : nullptr};
        hipLaunchKernelGGL(ce_grad_weighted_kernel, dim3((mb + 3) / 4), dim3(256), 0, st, g);
    }
    HIP_TRY(hipGetLastError());
    if (row_group) {
        HIP_TRY(hipMemcpyAsync(gd, row_group, (size_t)mb * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(Vd, vmass.data(), (size_t)G * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(lqd, log_q_in, (size_t)G * 8, hipMemcpyHostToDevice, st));
        DroGroup du;
        du.d[0] = DroDesc{t->row_loss, gd, Vd, lqd, cd, gld, mb, G, eta};
        hipLaunchKernelGGL(dro_update_kernel, dim3(1), dim3(1024), 0, st, du);
        RowScaleGroup rs;
        rs.d[0] = RowScaleDesc{t->dZ[L], t->row_loss, cd, mb, t->K};
        hipLaunchKernelGGL(row_scale_kernel, dim3((mb + 3) / 4), dim3(256), 0, st, rs);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(log_q_out, lqd, (size_t)G * 8, hipMemcpyDeviceToHost, st));
        if (group_loss) HIP_TRY(hipMemcpyAsync(group_loss, gld, (size_t)G * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(dlogits, t->dZ[L], cells * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(row_loss, t->row_loss, (size_t)mb * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MMC_OK;
}

// The step's two batch-normalisation kernels on caller arrays (include/mmc.h, "batch normalisation"): bn_forward_kernel on Z with the
// trainer's current gamma / beta of hidden layer `layer`, then, given dA, bn_backward_kernel.  Everything lives in the trainer's
// scratch: neither the running statistics nor any other state is read or written.
extern "C" int mmc_trainer_norm_stage(mmc_trainer* t, int layer, const float* Z, const float* dA, int64_t mb, float* H, float* dZ,
                                      float* g_gamma, float* g_beta, float* batch_mean, float* batch_var, void* hip_stream)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!t->bn) return mmc_fail(MMC_ERR_ARG, "the trainer has no batch normalisation (mmc_trainer_set_batch_norm)");
    if (layer < 0 || layer >= t->L - 1) return mmc_fail(MMC_ERR_ARG, "layer = %d is not a hidden layer [0, %d)", layer, t->L - 1);
    if (!Z || !H || !batch_mean || !batch_var) return mmc_fail(MMC_ERR_ARG, "Z / H / batch_mean / batch_var is NULL");
    if (dA && (!dZ || !g_gamma || !g_beta)) return mmc_fail(MMC_ERR_ARG, "dA needs dZ, g_gamma and g_beta");
    if (mb < 2 || mb > kTrainerForwardRows) return mmc_fail(MMC_ERR_ARG, "mb = %lld outside [2, %d]", (long long)mb, kTrainerForwardRows);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(t->device));
    const int M = (int)mb, N = t->dims[layer + 1];
    const size_t cells = (size_t)M * N;
    void* sc = nullptr;
    if (int r = trainer_scratch(t, (3 * cells + 5 * (size_t)N) * 4, &sc)) return r;
    float* Zd = static_cast<float*>(sc);
    float* Ad = Zd + cells;
    float* Hd = Ad + cells;
    float* mud = Hd + cells;
    float* rsd = mud + N;
    float* vd = rsd + N;
    float* ggd = vd + N;
    float* gbd = ggd + N;
    HIP_TRY(hipMemcpyAsync(Zd, Z, cells * 4, hipMemcpyHostToDevice, st));
    BnFwdGroup gf;
    gf.d[0] = BnFwdDesc{Zd, t->bn_ptr(t->bn_p, layer, 0), t->bn_ptr(t->bn_p, layer, 1), Hd, mud, rsd, nullptr, nullptr, vd, M, N,
                        (float)t->bn_eps, (float)t->bn_mom, (float)(1.0 - t->bn_mom), (float)((double)M / ((double)M - 1.0))};
    hipLaunchKernelGGL(bn_forward_kernel, dim3((N + 63) / 64), dim3(256), 0, st, gf);
    HIP_TRY(hipGetLastError());
    if (dA) {
        HIP_TRY(hipMemcpyAsync(Ad, dA, cells * 4, hipMemcpyHostToDevice, st));
        BnBwdGroup gb;
        gb.d[0] = BnBwdDesc{Ad, Zd, mud, rsd, t->bn_ptr(t->bn_p, layer, 0), ggd, gbd, M, N};
        hipLaunchKernelGGL(bn_backward_kernel, dim3((N + 63) / 64), dim3(256), 0, st, gb);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(dZ, Ad, cells * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(g_gamma, ggd, (size_t)N * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(g_beta, gbd, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(H, Hd, cells * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(batch_mean, mud, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(batch_var, vd, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MMC_OK;
}
