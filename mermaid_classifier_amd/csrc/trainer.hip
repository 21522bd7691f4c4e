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
// Per trainer and pass, off by default (include/mmc.h, "distillation"; a member without a target set runs the loss kernels above as ever):
//   soft      l_i = s_i [(1 - alpha) b_i + alpha tau^2 w_t k_i], k_i the cross-entropy of the row's own target, read in place
//             from a resident target set, against softmax(u / tau); row weights ride the same kernel   ce_grad_distill_kernel, ce_grad_rows_distill
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
//
// This file holds the kernels and everything that launches one (the step, its loss stage, the gathers, the eval-mode forward, the
// probes); the handle and its options are in trainer_options.cpp, the passes in trainer_pass.cpp, over trainer_state.h.
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
#include "trainer_state.h"

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
// What a kernel of a step takes: its members' descriptors by value, within the 4 KB of kernel arguments the runtime passes.
template <class D>
struct Group {
    static_assert(sizeof(D) * MMC_TRAINER_GROUP_MAX <= 4096, "kernel-argument limit");
    D d[MMC_TRAINER_GROUP_MAX];
};
using GemmGroup = Group<GemmDesc>;
// the forward launch of a layer in which at least one member drops: the members' mask parameters beside their descriptors
struct GemmDropGroup {
    GemmDesc d[MMC_TRAINER_GROUP_MAX];
    DropMask r[MMC_TRAINER_GROUP_MAX];
};
static_assert(sizeof(GemmDropGroup) <= 4096, "kernel-argument limit");

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
using DropRowsGroup = Group<DropRowsDesc>;

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
using CeGroup = Group<CeDesc>;

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
using CeMixGroup = Group<CeMixDesc>;

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
using CeRowGroup = Group<CeRowDesc>;

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
using CeHierGroup = Group<CeHierDesc>;

__global__ __launch_bounds__(256) void ce_grad_hier_kernel(const CeHierGroup g)
{
    const CeHierDesc& d = g.d[blockIdx.z];
    if ((int)blockIdx.x * 4 >= d.c.M) return;
    ce_grad_rows_hier(blockIdx.x, d.c.logits, d.c.y, d.c.M, d.c.K, d.c.cw, d.c.inv_wsum, d.c.dlogits, d.c.row_loss, d.c.loss, d.h, d.rw);
}

// ---- distillation (include/mmc.h): the loss stage of a member whose pass has a target set, with or without row weights.  A body of
// its own: the members without targets keep the kernels above and their code.
struct DistillLoss {
    const float* q;           // the target set's rows [.][K]
    const int64_t* visit;     // the pass's visiting order on the device, or null: position pos reads row visit ? visit[pos] : pos
    int64_t start;            // the mini-batch's first position in the pass
    float om_alpha;           // (float)(1 - alpha)
    float a_grad, a_loss;     // (float)(alpha tau), (float)(alpha tau^2)
    float inv_tau;            // (float)(1 / tau)
    int temp;                 // tau != 1: the second instantiation
};

// One wave per row, classes lane-strided, every row reduction a lane-strided sum (or max) and the xor butterfly.  The row's target
// q is read in place from the target set: 4 K consecutive bytes per wave, lane-strided, no gather copy.
//   hard   b, db: the general form, operation for operation as ce_grad_rows<true> forms it (at its defaults the plain weighted CE)
//   soft   TEMP = false: qt = q as stored, pt = p, the hard term's softmax; sq = sum_c q_c (its fp32 sum stands where 1 would)
//          TEMP = true:  v_c = u_c inv_tau with its own maximum mv and lv = logf(sum expf(v_c - mv)), pt_c = expf(v_c - mv - lv);
//                        g_c = logf(q_c) inv_tau over the classes with q_c > 0, its own maximum mg and lg = logf(sum expf(g_c - mg)),
//                        qt_c = expf(g_c - mg - lg), 0 where q_c == 0; sq = sum_c qt_c
//          k = -sum_c qt_c log pt_c, a class with qt_c == 0 adding 0
//   row    l_i = s_i (om_alpha b + (a_loss w_t) k),  dl_i/dz_c = s_i (om_alpha db_c + (a_grad w_t) (pt_c sq - qt_c)),
//          s_i = rw ? rw[row] * inv_wsum : inv_wsum
// Finite on any finite logits row and any valid target row: a valid row has a positive entry, so mg is finite and its sum is at
// least 1; log pt_c is finite; nothing divides.
template <bool TEMP>
__device__ __forceinline__ void ce_grad_rows_distill(int block, const float* __restrict__ logits, const int32_t* __restrict__ y, int M, int K,
                                                     const float* __restrict__ cw, float inv_wsum, float* __restrict__ dlogits,
                                                     float* __restrict__ row_loss, const CeLoss& ls, const DistillLoss& dl,
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
    const int64_t pos = dl.start + row;
    const float* qr = dl.q + (size_t)(dl.visit ? dl.visit[pos] : pos) * K;
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
    float sl = 0.f;            // sum_c w_c logp_c of the smoothing term
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
    const float a = ls.om_eps * w;
    const float af = a * f;
    float lb = a * m * nll;
    if (smooth) lb = lb - ls.eps_k * sl;
    // the soft term
    float mv = 0.f, lv = 0.f, mg = 0.f, lg = 0.f;
    if (TEMP) {
        mv = -INFINITY;
        mg = -INFINITY;
        for (int c = lane; c < K; c += 64) {
            const float u = pr ? z[c] + pr[c] : z[c];
            mv = fmaxf(mv, u * dl.inv_tau);
            const float q = qr[c];
            if (q > 0.f) mg = fmaxf(mg, logf(q) * dl.inv_tau);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            mv = fmaxf(mv, __shfl_xor(mv, o));
            mg = fmaxf(mg, __shfl_xor(mg, o));
        }
        float sv = 0.f, sg = 0.f;
        for (int c = lane; c < K; c += 64) {
            const float u = pr ? z[c] + pr[c] : z[c];
            sv += expf(u * dl.inv_tau - mv);
            const float q = qr[c];
            sg += q > 0.f ? expf(logf(q) * dl.inv_tau - mg) : 0.f;
        }
        sv = wave_sum(sv);
        sg = wave_sum(sg);
        lv = logf(sv);
        lg = logf(sg);
    }
    float sq = 0.f, sk = 0.f;   // sum_c qt_c; sum_c qt_c log pt_c
    for (int c = lane; c < K; c += 64) {
        const float u = pr ? z[c] + pr[c] : z[c];
        const float q = qr[c];
        float qt, lpt;
        if (TEMP) {
            qt = q > 0.f ? expf(logf(q) * dl.inv_tau - mg - lg) : 0.f;
            lpt = u * dl.inv_tau - mv - lv;
        } else {
            qt = q;
            lpt = u - mx - lse;
        }
        sq += qt;
        sk += qt != 0.f ? qt * lpt : 0.f;
    }
    sq = wave_sum(sq);
    sk = wave_sum(sk);
    const float wg = dl.a_grad * w, wl = dl.a_loss * w;
    for (int c = lane; c < K; c += 64) {
        const float u = pr ? z[c] + pr[c] : z[c];
        const float p = expf(u - mx - lse);
        float d = af * (p - (c == yi ? 1.0f : 0.0f));
        if (smooth) d = d + ls.eps_k * (p * ls.w_total - (cw ? cw[c] : 1.0f));
        const float q = qr[c];
        float qt, pt;
        if (TEMP) {
            qt = q > 0.f ? expf(logf(q) * dl.inv_tau - mg - lg) : 0.f;
            pt = expf(u * dl.inv_tau - mv - lv);
        } else {
            qt = q;
            pt = p;
        }
        d = dl.om_alpha * d + wg * (pt * sq - qt);
        dlogits[(size_t)row * K + c] = inv_wsum * d;
    }
    if (lane == 0) row_loss[row] = (dl.om_alpha * lb + wl * (-sk)) * inv_wsum;
}

struct CeDistillDesc {
    CeDesc c;          // inv_wsum as in CeDesc, or as in CeRowDesc for a member with row weights or groups
    const float* rw;   // the weights of the mini-batch's positions, or null
    DistillLoss d;
};
using CeDistillGroup = Group<CeDistillDesc>;

__global__ __launch_bounds__(256) void ce_grad_distill_kernel(const CeDistillGroup g)
{
    const CeDistillDesc& d = g.d[blockIdx.z];
    if ((int)blockIdx.x * 4 >= d.c.M) return;
    if (d.d.temp)
        ce_grad_rows_distill<true>(blockIdx.x, d.c.logits, d.c.y, d.c.M, d.c.K, d.c.cw, d.c.inv_wsum, d.c.dlogits, d.c.row_loss, d.c.loss, d.d, d.rw);
    else
        ce_grad_rows_distill<false>(blockIdx.x, d.c.logits, d.c.y, d.c.M, d.c.K, d.c.cw, d.c.inv_wsum, d.c.dlogits, d.c.row_loss, d.c.loss, d.d, d.rw);
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
using DroGroup = Group<DroDesc>;

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
using RowScaleGroup = Group<RowScaleDesc>;

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
using ColsumGroup = Group<ColsumDesc>;

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
using SumsqGroup = Group<SumsqDesc>;

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
using LossGroup = Group<LossDesc>;

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
using AdamGroup = Group<AdamDesc>;

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
using GnormGroup = Group<GnormDesc>;

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
using AdamOptGroup = Group<AdamOptDesc>;

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
using BnFwdGroup = Group<BnFwdDesc>;
struct BnBwdDesc {
    float* dA;                   // [M][N] in: gradient w.r.t. gamma xhat + beta; out: gradient w.r.t. Z
    const float *Z, *mu, *rstd, *gamma;
    float *ggamma, *gbeta;       // [N]
    int M, N;
};
using BnBwdGroup = Group<BnBwdDesc>;
// the fold of one trainer: one descriptor per hidden layer (n_layers <= 16, so at most 15)
struct BnFoldDesc {
    const float *W, *b, *gamma, *beta, *rmean, *rvar;
    float *Wf, *bf;
    int N, K;
    float eps;
};
using BnFoldGroup = Group<BnFoldDesc>;
static_assert(sizeof(BnFwdGroup) <= 4096, "kernel-argument limit");   // (Group's own check, spelled out: tests/test_batch_norm_host.py reads it)

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

// ---- host: every launch of the kernels above ---------------------------------------------------------------------------------------
// The members of one launch: their descriptors in blockIdx.z order, how many, and the largest of up to two extents among them.
// The grid's x and y are made from the largest extents (blocks), z is the member count; an empty launch does nothing.
template <class D>
struct GroupLaunch {
    Group<D> g;
    int n = 0;
    size_t ext[2] = {0, 0};
    void add(const D& desc, size_t e0 = 0, size_t e1 = 0)
    {
        g.d[n++] = desc;
        ext[0] = std::max(ext[0], e0);
        ext[1] = std::max(ext[1], e1);
    }
    unsigned blocks(int i, size_t per) const { return (unsigned)((ext[i] + per - 1) / per); }
    void launch(void (*kernel)(const Group<D>), dim3 grid, unsigned block, hipStream_t st) const
    {
        if (!n) return;
        grid.z = n;
        hipLaunchKernelGGL(kernel, grid, dim3(block), 0, st, g);
    }
};

// a GEMM launch: 64 x 64 tiles over the largest M and N of its members (GemmDesc goes in with add(d, d.M, d.N))
dim3 gemm_tiles(const GroupLaunch<GemmDesc>& m) { return dim3(m.blocks(0, 64), m.blocks(1, 64)); }
int launch_gemm(const GroupLaunch<GemmDesc>& m, void (*kernel)(const GemmGroup), hipStream_t st)
{
    m.launch(kernel, gemm_tiles(m), 256, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the kernel's fp32 scalars of the trainer's loss options, each the float of a double expression (include/mmc.h)
CeLoss trainer_ce_loss(const mmc_trainer* t)
{
    return CeLoss{t->prior, (float)(1.0 - t->label_smoothing), (float)(t->label_smoothing / (double)t->K), (float)t->focal_gamma, t->w_total};
}

HierLoss trainer_hier_loss(const mmc_trainer* t)
{
    HierLoss h{t->hier_ids, t->hier_T, t->hier_levels, {0.f, 0.f, 0.f, 0.f}};
    std::copy(t->hier_lam, t->hier_lam + MMC_HIER_MAX_LEVELS, h.lam);
    return h;
}

double trainer_lr_at(const mmc_trainer* t, long long step)
{
    double lr = t->lr;
    mmc_lr_schedule_at(t->lr, t->lr_kind, t->warmup_steps, t->total_steps, t->final_ratio, step, &lr);   // the options were checked when set
    return lr;
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

// ---- batch normalisation: hidden layer h of t on mb rows, the trainer's gamma / beta; the arrays are the step's or a probe's -------
BnFwdDesc bn_forward_desc(const mmc_trainer* t, int h, int mb, const float* Z, float* H, float* mu, float* rstd, float* rmean, float* rvar,
                          float* var)
{
    return BnFwdDesc{Z, t->bn_ptr(t->bn_p, h, 0), t->bn_ptr(t->bn_p, h, 1), H, mu, rstd, rmean, rvar, var, mb, t->dims[h + 1],
                     (float)t->bn_eps, (float)t->bn_mom, (float)(1.0 - t->bn_mom), (float)((double)mb / ((double)mb - 1.0))};
}

BnBwdDesc bn_backward_desc(const mmc_trainer* t, int h, int mb, float* dA, const float* Z, const float* mu, const float* rstd, float* ggamma,
                           float* gbeta)
{
    return BnBwdDesc{dA, Z, mu, rstd, t->bn_ptr(t->bn_p, h, 0), ggamma, gbeta, mb, t->dims[h + 1]};
}

void launch_bn_forward(const GroupLaunch<BnFwdDesc>& m, hipStream_t st) { m.launch(bn_forward_kernel, dim3(m.blocks(0, 64)), 256, st); }
void launch_bn_backward(const GroupLaunch<BnBwdDesc>& m, hipStream_t st) { m.launch(bn_backward_kernel, dim3(m.blocks(0, 64)), 256, st); }

// ---- the loss stage ------------------------------------------------------------------------------------------------------------
// One member of a loss stage: cur rows of logits, their targets and what a mixed or a weighted member adds.  Class weights, loss
// options and hierarchy are the trainer's, and the gradient and the row losses go to its dZ[L] and row_loss.
struct LossMember {
    const mmc_trainer* t;
    const float* logits;
    const int32_t* y;
    int cur;
    float inv_wsum;
    const int32_t* y2 = nullptr;    // a mixed member: the second targets and lam
    float lam = 0.f;
    bool weighted = false;          // a weighted member, whether or not it has either array
    const float* rw = nullptr;      // the rows' weights, or null (all 1)
    const int32_t* rg = nullptr;    // the rows' groups, or null; with them the five below
    const double* V = nullptr;      // [n_groups] the groups' masses in these rows
    double* logq = nullptr;         // [n_groups] in / out
    float* row_scale = nullptr;     // [cur] c_i
    double* group_loss = nullptr;   // [n_groups] L_a, or null
    int n_groups = 0;
    double eta = 0.0;
    const float* q = nullptr;           // a member with targets: the target rows, the pass's visiting order on the device (or null)
    const int64_t* q_visit = nullptr;   // and the mini-batch's first position in the pass
    int64_t q_start = 0;
};

// the kernel's fp32 scalars of the trainer's distillation options, each the float of a double expression (include/mmc.h)
DistillLoss trainer_distill_loss(const mmc_trainer* t, const float* q, const int64_t* visit, int64_t start)
{
    const double a = t->distill_alpha, tau = t->distill_tau;
    return DistillLoss{q, visit, start, (float)(1.0 - a), (float)(a * tau), (float)(a * tau * tau), (float)(1.0 / tau), tau != 1.0 ? 1 : 0};
}

// The loss launches of `cnt` members.  Which kernel a member runs: with targets ce_grad_distill_kernel; with a hierarchy
// ce_grad_hier_kernel (row weights ride either, and the two never meet: the setters and the passes refuse); else weighted
// ce_grad_weighted_kernel; else mixed ce_grad_mixed_kernel; else ce_grad_kernel.  A weighted member with groups then moves its q
// on the device and every row takes its group's share.
void loss_stage(const LossMember* mem, int cnt, hipStream_t st)
{
    GroupLaunch<CeDesc> plain;
    GroupLaunch<CeMixDesc> mixed;
    GroupLaunch<CeRowDesc> rows;
    GroupLaunch<CeHierDesc> hier;
    GroupLaunch<CeDistillDesc> soft;
    GroupLaunch<DroDesc> dro;
    GroupLaunch<RowScaleDesc> scale;
    for (int i = 0; i < cnt; ++i) {
        const LossMember& m = mem[i];
        const mmc_trainer* t = m.t;
        const CeDesc c{m.logits, m.y, t->cw, t->dZ[t->L], t->row_loss, m.cur, t->K, m.inv_wsum, t->general ? 1 : 0, trainer_ce_loss(t)};
        if (m.q)
            soft.add(CeDistillDesc{c, m.weighted ? m.rw : nullptr, trainer_distill_loss(t, m.q, m.q_visit, m.q_start)}, m.cur);
        else if (t->hier)
            hier.add(CeHierDesc{c, m.weighted ? m.rw : nullptr, trainer_hier_loss(t)}, m.cur);
        else if (m.weighted)
            rows.add(CeRowDesc{c, m.rw}, m.cur);
        else if (m.y2)
            mixed.add(CeMixDesc{m.logits, m.y, m.y2, t->cw, t->dZ[t->L], t->row_loss, m.cur, t->K, m.inv_wsum, m.lam, 1.0f - m.lam, c.loss}, m.cur);
        else
            plain.add(c, m.cur);
        if (m.weighted && m.rg) {
            dro.add(DroDesc{t->row_loss, m.rg, m.V, m.logq, m.row_scale, m.group_loss, m.cur, m.n_groups, m.eta});
            scale.add(RowScaleDesc{t->dZ[t->L], t->row_loss, m.row_scale, m.cur, t->K}, m.cur);
        }
    }
    plain.launch(ce_grad_kernel, dim3(plain.blocks(0, 4)), 256, st);   // one wave per row, four rows per workgroup
    mixed.launch(ce_grad_mixed_kernel, dim3(mixed.blocks(0, 4)), 256, st);
    rows.launch(ce_grad_weighted_kernel, dim3(rows.blocks(0, 4)), 256, st);
    hier.launch(ce_grad_hier_kernel, dim3(hier.blocks(0, 4)), 256, st);
    soft.launch(ce_grad_distill_kernel, dim3(soft.blocks(0, 4)), 256, st);
    dro.launch(dro_update_kernel, dim3(1), 1024, st);
    scale.launch(row_scale_kernel, dim3(scale.blocks(0, 4)), 256, st);
}

// Adam: one tensor of member t (W[l], b[l], or all of gamma / beta) into the launch it takes: the members that neither clip nor average
// go through adam_kernel, the others through adam_opt_kernel.  `shadow` is the tensor's averaged copy, or null.
void add_adam(GroupLaunch<AdamDesc>& plain, GroupLaunch<AdamOptDesc>& opt, const mmc_trainer* t, float step_size, float bc2_sqrt, float* p,
              const float* g, float* m, float* v, size_t n, float* shadow)
{
    const float om1 = (float)(1.0 - t->beta1), om2 = (float)(1.0 - t->beta2), b2f = (float)t->beta2, epsf = (float)t->eps;
    if (t->max_norm > 0.0 || !t->sW.empty())
        opt.add(AdamOptDesc{p, g, m, v, n, om1, b2f, om2, epsf, step_size, bc2_sqrt, t->max_norm > 0.0 ? t->coef.p : nullptr, shadow,
                            (float)(1.0 - t->ema_decay)}, n);
    else
        plain.add(AdamDesc{p, g, m, v, n, om1, b2f, om2, epsf, step_size, bc2_sqrt}, n);
}

void launch_adam(const GroupLaunch<AdamDesc>& m, hipStream_t st) { m.launch(adam_kernel, dim3(m.blocks(0, 256)), 256, st); }
void launch_adam(const GroupLaunch<AdamOptDesc>& m, hipStream_t st) { m.launch(adam_opt_kernel, dim3(m.blocks(0, 256)), 256, st); }

void launch_sumsq(const GroupLaunch<SumsqDesc>& m, hipStream_t st) { m.launch(sumsq_kernel, dim3(256), 256, st); }   // 256 blocks always

}  // namespace

// W' / b' of the hidden layers from the current gamma, beta and running statistics, on `st`; nothing when the fold is current
int trainer_refresh_fold(mmc_trainer* t, hipStream_t st)
{
    if (!t->bn || !t->fold_stale) return 0;
    const int H = t->L - 1;
    if (H > 0) {   // one descriptor per hidden layer: n_layers <= 16, so at most 15
        GroupLaunch<BnFoldDesc> fold;
        for (int h = 0; h < H; ++h)
            fold.add(BnFoldDesc{t->W[h], t->b[h], t->bn_ptr(t->bn_p, h, 0), t->bn_ptr(t->bn_p, h, 1), t->bn_ptr(t->bn_run, h, 0),
                                t->bn_ptr(t->bn_run, h, 1), t->fW[h], t->fb[h], t->dims[h + 1], t->dims[h], (float)t->bn_eps},
                     t->dims[h + 1]);
        fold.launch(bn_fold_kernel, dim3(fold.blocks(0, 1)), 256, st);
        HIP_TRY(hipGetLastError());
    }
    t->fold_stale = false;
    return 0;
}

// the staging, activation and loss buffers of a pass of `steps` mini-batches of mb rows over n staged rows
int trainer_reserve(mmc_trainer* t, int64_t n, int mb, int steps)
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
        GroupLaunch<DropRowsDesc> drop;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            if (t->thresh_input) drop.add(DropRowsDesc{t->H[0], act[i].cur, t->dims[0], drop_mask(t, 0)}, (size_t)act[i].cur * t->dims[0]);
        }
        drop.launch(dropout_rows_kernel, dim3(std::min(drop.blocks(0, 256), 4096u)), 256, st);   // grid-stride
    }
    for (int l = 0; l < Lmax; ++l) {
        GroupLaunch<GemmDesc> fw;
        GroupLaunch<BnFwdDesc> norm;
        DropMask masks[MMC_TRAINER_GROUP_MAX];
        bool drops = false;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            if (l >= t->L) continue;
            GemmDesc d = forward_desc(t, l, act[i].cur);
            masks[fw.n] = DropMask{};
            if (t->thresh_hidden && l < t->L - 1) {   // the last layer never drops
                d.epi = TEPI_BIAS_RELU_DROP;
                masks[fw.n] = drop_mask(t, l + 1);
                drops = true;
            }
            if (t->bn && l < t->L - 1) {   // a normalised layer: Z = H W^T + b to a buffer of its own, bn_forward_kernel makes H(l+1)
                d.C = t->Zbuf[l + 1];
                d.epi = TEPI_BIAS;
                norm.add(bn_forward_desc(t, l, act[i].cur, t->Zbuf[l + 1], t->H[l + 1], t->bn_ptr(t->bn_stat, l, 0), t->bn_ptr(t->bn_stat, l, 1),
                                         t->bn_ptr(t->bn_run, l, 0), t->bn_ptr(t->bn_run, l, 1), nullptr),
                         t->dims[l + 1]);
            }
            fw.add(d, d.M, d.N);
        }
        if (drops) {   // the members' masks beside their descriptors
            GemmDropGroup g;
            std::copy(fw.g.d, fw.g.d + fw.n, g.d);
            std::copy(masks, masks + fw.n, g.r);
            dim3 grid = gemm_tiles(fw);
            grid.z = fw.n;
            hipLaunchKernelGGL(tgemm_f32_drop_kernel, grid, dim3(256), 0, st, g);
            HIP_TRY(hipGetLastError());
        } else if (int r = launch_gemm(fw, tgemm_f32_kernel<false, true, TEPI_BIAS_RELU, TEPI_BIAS>, st)) {
            return r;
        }
        launch_bn_forward(norm, st);
    }
    {
        LossMember mem[MMC_TRAINER_GROUP_MAX];
        for (int i = 0; i < cnt; ++i) {   // the distribution over the groups is the trainer's own and lives across steps
            const StepMember& a = act[i];
            const mmc_trainer* t = a.t;
            mem[i] = LossMember{t, t->H[t->L], t->y + a.off, a.cur, a.inv_wsum, a.mixed ? t->y2 + a.off : nullptr, a.lam, a.weighted, a.rw, a.rg,
                                a.V, t->logq, t->row_scale, nullptr, t->n_groups, t->dro_eta, a.q, a.q_visit, a.q_start};
        }
        loss_stage(mem, cnt, st);
    }
    // regularised loss of this mini-batch (before the update): data + (0.5 alpha / mb) sum W^2
    for (int l = 0; l < Lmax; ++l) {
        GroupLaunch<SumsqDesc> sq;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            if (l < t->L) sq.add(SumsqDesc{t->W[l], t->partials + 256 * l, (size_t)t->dims[l + 1] * t->dims[l]});
        }
        launch_sumsq(sq, st);
    }
    {
        GroupLaunch<LossDesc> fin;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            fin.add(LossDesc{t->row_loss, t->partials, t->losses + act[i].slot, act[i].cur, 256 * t->L, (float)(0.5 * t->alpha / (double)act[i].cur)});
        }
        fin.launch(loss_finalize_kernel, dim3(1), 256, st);
    }
    for (int l = Lmax - 1; l >= 0; --l) {
        GroupLaunch<GemmDesc> gw, gz;
        GroupLaunch<ColsumDesc> gc;
        GroupLaunch<BnBwdDesc> norm;
        bool drops = false;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            if (l >= t->L) continue;
            const int no = t->dims[l + 1], ni = t->dims[l], mb = act[i].cur;
            gw.add(GemmDesc{t->dZ[l + 1], t->H[l], t->gW[l], t->W[l], no, ni, mb, TEPI_L2, (float)(t->alpha / (double)mb)}, no, ni);
            // the bias of a normalised layer is frozen: gb[l] stays the zeros it was filled with
            if (!(t->bn && l < t->L - 1)) gc.add(ColsumDesc{t->dZ[l + 1], t->gb[l], mb, no}, no);
            if (t->bn && l > 0)   // dZ[l] is dA of hidden layer l - 1 once this iteration's mask launch has run: make it dZ in place
                norm.add(bn_backward_desc(t, l - 1, mb, t->dZ[l], t->Zbuf[l], t->bn_ptr(t->bn_stat, l - 1, 0), t->bn_ptr(t->bn_stat, l - 1, 1),
                                          t->bn_ptr(t->bn_g, l - 1, 0), t->bn_ptr(t->bn_g, l - 1, 1)),
                         ni);
            if (l > 0) {
                GemmDesc d{t->dZ[l + 1], t->W[l], t->dZ[l], t->H[l], mb, ni, no, TEPI_MASK, 0.f};
                if (t->thresh_hidden) {   // H(l) was dropped in the forward: the kept elements carry the scale back
                    d.epi = TEPI_MASK_SCALE;
                    d.scale = t->scale_hidden;
                    drops = true;
                }
                gz.add(d, d.M, d.N);
            }
        }
        if (int r = launch_gemm(gw, tgemm_f32_kernel<true, false, TEPI_L2, TEPI_L2>, st)) return r;
        gc.launch(colsum_kernel, dim3(gc.blocks(0, 256)), 256, st);
        if (int r = launch_gemm(gz, drops ? tgemm_f32_mask_scale_kernel : tgemm_f32_kernel<false, false, TEPI_MASK, TEPI_MASK>, st)) return r;
        launch_bn_backward(norm, st);
    }
    {   // gradient clipping: the clipping members' norm over every gW[l] / gb[l] (the L2 term is in gW), their coefficient to device
        // memory; the Adam stage reads it there, so nothing waits on the host
        for (int l = 0; l < Lmax; ++l) {
            GroupLaunch<SumsqDesc> sw, sb;
            for (int i = 0; i < cnt; ++i) {
                const mmc_trainer* t = act[i].t;
                if (!(t->max_norm > 0.0) || l >= t->L) continue;
                sw.add(SumsqDesc{t->gW[l], t->gpartials + 256 * (2 * l), (size_t)t->dims[l + 1] * t->dims[l]});
                sb.add(SumsqDesc{t->gb[l], t->gpartials + 256 * (2 * l + 1), (size_t)t->dims[l + 1]});
            }
            launch_sumsq(sw, st);
            launch_sumsq(sb, st);
        }
        // the normalised members' g_gamma / g_beta of every hidden layer: one more tensor, its partials after the layers'
        GroupLaunch<SumsqDesc> sn;
        GroupLaunch<GnormDesc> fin;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            if (!(t->max_norm > 0.0)) continue;
            const bool extra = t->bn && t->bn_total;
            if (extra) sn.add(SumsqDesc{t->bn_g, t->gpartials + 256 * (2 * t->L), (size_t)t->bn_total});
            fin.add(GnormDesc{t->gpartials, t->coef, t->gnorm + act[i].slot, 256 * (2 * t->L + (extra ? 1 : 0)), (float)t->max_norm});
        }
        launch_sumsq(sn, st);
        fin.launch(gnorm_finalize_kernel, dim3(1), 256, st);
    }
    float step_size[MMC_TRAINER_GROUP_MAX], bc2_sqrt[MMC_TRAINER_GROUP_MAX];
    for (int i = 0; i < cnt; ++i) {
        mmc_trainer* t = act[i].t;
        ++t->t;
        const double bc1 = 1.0 - std::pow(t->beta1, (double)t->t), bc2 = 1.0 - std::pow(t->beta2, (double)t->t);
        step_size[i] = (float)(trainer_lr_at(t, t->t) / bc1);
        bc2_sqrt[i] = (float)std::sqrt(bc2);
    }
    for (int l = 0; l < Lmax; ++l) {
        GroupLaunch<AdamDesc> gw, gb;
        GroupLaunch<AdamOptDesc> ow, ob;
        for (int i = 0; i < cnt; ++i) {
            const mmc_trainer* t = act[i].t;
            if (l >= t->L) continue;
            const bool ema = !t->sW.empty();
            add_adam(gw, ow, t, step_size[i], bc2_sqrt[i], t->W[l], t->gW[l], t->mW[l], t->vW[l], (size_t)t->dims[l + 1] * t->dims[l],
                     ema ? t->sW[l].p : nullptr);
            add_adam(gb, ob, t, step_size[i], bc2_sqrt[i], t->b[l], t->gb[l], t->mb[l], t->vb[l], (size_t)t->dims[l + 1], ema ? t->sb[l].p : nullptr);
        }
        launch_adam(gw, st);
        launch_adam(gb, st);
        launch_adam(ow, st);
        launch_adam(ob, st);
    }
    {   // gamma and beta of the normalised members, every hidden layer at once: further descriptors of the same two kernels
        GroupLaunch<AdamDesc> gn;
        GroupLaunch<AdamOptDesc> on;
        for (int i = 0; i < cnt; ++i) {
            mmc_trainer* t = act[i].t;
            if (!t->bn) continue;
            t->fold_stale = true;
            if (t->bn_total) add_adam(gn, on, t, step_size[i], bc2_sqrt[i], t->bn_p, t->bn_g, t->bn_m, t->bn_v, (size_t)t->bn_total, nullptr);
        }
        launch_adam(gn, st);
        launch_adam(on, st);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mmc_fail(MMC_ERR_HIP, "trainer step launch failed: %s", hipGetErrorString(e));
    return 0;
}

// ---- staging the rows of a pass -----------------------------------------------------------------------------------------------
// t->X / t->y = rows t->order[0 .. n) of the uploaded t->Xn / t->yn: the host-fed pass (dims[0] a multiple of 4)
void gather_ordered(mmc_trainer* t, int64_t n, hipStream_t st)
{
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)n), dim3(256), 0, st, t->Xn, t->yn, t->order, n, t->dims[0] / 4, t->X, t->y);
}

// rows [c0, c0 + rows) of the pass into the staging t->X / t->y
int gather_chunk(mmc_trainer* t, const mmc_featureset* fs, bool visited, bool mixed, int mb, int64_t c0, int rows, hipStream_t st)
{
    const int64_t* vis = visited ? t->visit + c0 : nullptr;
    const dim3 grid((rows + 3) / 4), block(256);
    const int64_t* par = mixed ? t->partner + c0 : nullptr;   // c0 is a multiple of mb: the chunk's first mini-batch is c0 / mb of the pass
    const float* lam = mixed ? t->lam + c0 / mb : nullptr;
    // (each kernel named in a launch of its own: taking their addresses through a conditional changes their device code)
    if (mixed && (fs->dim & 3))
        hipLaunchKernelGGL(gather_set_rows_mixed_kernel<false>, grid, block, 0, st, fs->X, fs->y, vis, c0, par, lam, mb, rows, fs->dim, t->X, t->y, t->y2);
    else if (mixed)
        hipLaunchKernelGGL(gather_set_rows_mixed_kernel<true>, grid, block, 0, st, fs->X, fs->y, vis, c0, par, lam, mb, rows, fs->dim, t->X, t->y, t->y2);
    else if (fs->dim & 3)
        hipLaunchKernelGGL(gather_set_rows_kernel<false>, grid, block, 0, st, fs->X, fs->y, vis, c0, rows, fs->dim, t->X, t->y);
    else
        hipLaunchKernelGGL(gather_set_rows_kernel<true>, grid, block, 0, st, fs->X, fs->y, vis, c0, rows, fs->dim, t->X, t->y);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the eval-mode forward ------------------------------------------------------------------------------------------------------
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
        GemmDesc d = forward_desc(t, l, n);
        if (t->eval_which == MMC_WEIGHTS_AVERAGED) {   // mmc_trainer_eval_weights: the same launch on the shadow
            d.B = t->sW[l];
            d.aux = t->sb[l];
        }
        if (t->bn && l < t->L - 1) {   // and on the folded layers: relu(W' x + b') is the frozen-statistics layer
            d.B = t->fW[l];
            d.aux = t->fb[l];
        }
        GroupLaunch<GemmDesc> fw;
        fw.add(d, d.M, d.N);
        if ((r = launch_gemm(fw, tgemm_f32_kernel<false, true, TEPI_BIAS_RELU, TEPI_BIAS>, st))) return r;
    }
    *logits = t->H[t->L];
    return MMC_OK;
}

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

// ---- probes: one stage of a step on caller arrays (include/mmc.h) -----------------------------------------------------------------
namespace {

// What the three loss probes share.  First the step's own logits / gradient / row-loss buffers for n rows, the caller's logits in
// t->H[L], and *scratch = `bytes` of the trainer's scratch for what else the probe uploads.
int loss_probe_begin(mmc_trainer* t, const float* logits, int n, size_t bytes, void** scratch, hipStream_t st)
{
    HIP_TRY(hipSetDevice(t->device));
    int r = trainer_reserve(t, 0, n, 1);
    if (r) return r;
    if ((r = trainer_scratch(t, bytes, scratch))) return r;
    HIP_TRY(hipMemcpyAsync(t->H[t->L], logits, (size_t)n * t->K * 4, hipMemcpyHostToDevice, st));
    return 0;
}

// Then loss_stage on one member, which is the stage of a step of this trainer, and the gradient and the row losses on their way
// back; the caller synchronises the stream.
int loss_probe_run(mmc_trainer* t, const LossMember& m, float* dlogits, float* row_loss, hipStream_t st)
{
    loss_stage(&m, 1, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dlogits, t->dZ[t->L], (size_t)m.cur * t->K * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(row_loss, t->row_loss, (size_t)m.cur * 4, hipMemcpyDeviceToHost, st));
    return 0;
}

}  // namespace

// the loss stage of a step on caller logits: the step's kernel, class weights, loss options and 1 / sum of w[y_i]
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
    const int mb = (int)n;
    void* sc = nullptr;
    int r = loss_probe_begin(t, logits, mb, (size_t)mb * 4, &sc, st);
    if (r) return r;
    int32_t* yd = static_cast<int32_t*>(sc);
    HIP_TRY(hipMemcpyAsync(yd, y, (size_t)mb * 4, hipMemcpyHostToDevice, st));
    if ((r = loss_probe_run(t, LossMember{t, t->H[t->L], yd, mb, (float)(1.0 / wsum)}, dlogits, row_loss, st))) return r;
    HIP_TRY(hipStreamSynchronize(st));
    return MMC_OK;
}

// mmc_trainer_loss_gradient for the mixed instantiation: two targets per row and one lam for all rows ("regularisers")
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
    const int mb = (int)n;
    void* sc = nullptr;
    int r = loss_probe_begin(t, logits, mb, (size_t)mb * 8, &sc, st);
    if (r) return r;
    int32_t* y1d = static_cast<int32_t*>(sc);
    int32_t* y2d = y1d + mb;
    HIP_TRY(hipMemcpyAsync(y1d, y, (size_t)mb * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(y2d, y2, (size_t)mb * 4, hipMemcpyHostToDevice, st));
    LossMember m{t, t->H[t->L], y1d, mb, (float)(1.0 / wsum)};
    m.y2 = y2d;
    m.lam = lam;
    if ((r = loss_probe_run(t, m, dlogits, row_loss, st))) return r;
    HIP_TRY(hipStreamSynchronize(st));
    return MMC_OK;
}

namespace {

// The weighted loss stage of a step on caller logits and an explicit log q (include/mmc.h, "group-robust training"): a weighted
// member whether or not either array is given, its groups' state in the trainer's scratch.  The trainer's own distribution is
// neither read nor written.  `q` (n x K host target rows, or null) makes it the distilled stage: the rows go to the scratch behind
// everything else, pass the target set's validity rule and are read in place, position i reading row i.
int weighted_loss_probe(mmc_trainer* t, const float* logits, const int32_t* y, const float* q, const float* row_weight,
                        const int32_t* row_group, const double* log_q_in, double eta, int n_groups, int64_t n, float* dlogits,
                        float* row_loss, double* log_q_out, double* group_loss, void* hip_stream)
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
    const int mb = (int)n;
    std::vector<double> wsums, vmass;
    int r = 0;
    if ((r = minibatch_masses("", t, y, nullptr, row_weight, row_group, G, n, mb, &wsums, &vmass))) return r;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // scratch: V [G] and log q [G] and group loss [G] in double first (8-byte aligned), then y, groups, weights and c by row
    void* sc = nullptr;
    const size_t cells = q ? (size_t)mb * t->K : 0;
    if ((r = loss_probe_begin(t, logits, mb, (size_t)G * 24 + (size_t)mb * 16 + cells * 4 + 16, &sc, st))) return r;
    double* Vd = static_cast<double*>(sc);
    double* lqd = Vd + G;
    double* gld = lqd + G;
    int32_t* yd = reinterpret_cast<int32_t*>(gld + G);
    int32_t* gd = yd + mb;
    float* wd = reinterpret_cast<float*>(gd + mb);
    float* cd = wd + mb;
    float* qd = cd + mb;
    if (q) {
        HIP_TRY(hipMemcpyAsync(qd, q, cells * 4, hipMemcpyHostToDevice, st));
        if ((r = target_rows_check(qd, mb, t->K, reinterpret_cast<int32_t*>(qd + cells), 0, st))) return r;
    }
    HIP_TRY(hipMemcpyAsync(yd, y, (size_t)mb * 4, hipMemcpyHostToDevice, st));
    if (row_weight) HIP_TRY(hipMemcpyAsync(wd, row_weight, (size_t)mb * 4, hipMemcpyHostToDevice, st));
    LossMember m{t, t->H[t->L], yd, mb, (float)(1.0 / wsums[0])};
    m.weighted = true;
    m.rw = row_weight ? wd : nullptr;
    m.q = q ? qd : nullptr;
    if (row_group) {   // the caller's log q and eta, never the trainer's
        HIP_TRY(hipMemcpyAsync(gd, row_group, (size_t)mb * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(Vd, vmass.data(), (size_t)G * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(lqd, log_q_in, (size_t)G * 8, hipMemcpyHostToDevice, st));
        m.rg = gd; m.V = Vd; m.logq = lqd; m.row_scale = cd; m.group_loss = gld; m.n_groups = G; m.eta = eta;
    }
    if ((r = loss_probe_run(t, m, dlogits, row_loss, st))) return r;
    if (row_group) {
        HIP_TRY(hipMemcpyAsync(log_q_out, lqd, (size_t)G * 8, hipMemcpyDeviceToHost, st));
        if (group_loss) HIP_TRY(hipMemcpyAsync(group_loss, gld, (size_t)G * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return MMC_OK;
}

}  // namespace

extern "C" int mmc_trainer_loss_gradient_weighted(mmc_trainer* t, const float* logits, const int32_t* y, const float* row_weight,
                                                  const int32_t* row_group, const double* log_q_in, double eta, int n_groups, int64_t n,
                                                  float* dlogits, float* row_loss, double* log_q_out, double* group_loss, void* hip_stream)
{
    return weighted_loss_probe(t, logits, y, nullptr, row_weight, row_group, log_q_in, eta, n_groups, n, dlogits, row_loss, log_q_out,
                               group_loss, hip_stream);
}

// The distilled loss stage of a step on caller logits and caller target rows (include/mmc.h, "distillation"): the weighted probe
// with a target row per position, so row weights and groups compose with it exactly as they do in a pass.
static int check_distill_probe(const mmc_trainer* t, const float* q)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!q) return mmc_fail(MMC_ERR_ARG, "q is NULL");
    if (t->distill_alpha == 0.0) return mmc_fail(MMC_ERR_ARG, "targets: the trainer needs mmc_trainer_set_distillation(alpha > 0)");
    if (t->hier) return mmc_fail(MMC_ERR_ARG, "a distilled loss stage takes no hierarchy (mmc_trainer_set_hierarchy)");
    return 0;
}

extern "C" int mmc_trainer_loss_gradient_distill_weighted(mmc_trainer* t, const float* logits, const int32_t* y, const float* q,
                                                          const float* row_weight, const int32_t* row_group, const double* log_q_in,
                                                          double eta, int n_groups, int64_t n, float* dlogits, float* row_loss,
                                                          double* log_q_out, double* group_loss, void* hip_stream)
{
    if (int r = check_distill_probe(t, q)) return r;
    return weighted_loss_probe(t, logits, y, q, row_weight, row_group, log_q_in, eta, n_groups, n, dlogits, row_loss, log_q_out, group_loss,
                               hip_stream);
}

extern "C" int mmc_trainer_loss_gradient_distill(mmc_trainer* t, const float* logits, const int32_t* y, const float* q, const float* row_weight,
                                                 int64_t n, float* dlogits, float* row_loss, void* hip_stream)
{
    if (int r = check_distill_probe(t, q)) return r;
    return weighted_loss_probe(t, logits, y, q, row_weight, nullptr, nullptr, 0.0, 0, n, dlogits, row_loss, nullptr, nullptr, hip_stream);
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
    GroupLaunch<BnFwdDesc> fw;
    fw.add(bn_forward_desc(t, layer, M, Zd, Hd, mud, rsd, nullptr, nullptr, vd), N);
    launch_bn_forward(fw, st);
    HIP_TRY(hipGetLastError());
    if (dA) {
        HIP_TRY(hipMemcpyAsync(Ad, dA, cells * 4, hipMemcpyHostToDevice, st));
        GroupLaunch<BnBwdDesc> bw;
        bw.add(bn_backward_desc(t, layer, M, Ad, Zd, mud, rsd, ggd, gbd), N);
        launch_bn_backward(bw, st);
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

