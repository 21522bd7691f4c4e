// k_generic.hip -- hand-written CDNA4 (gfx950) kernels for the EfficientNet-B0 patch
// feature-extraction path.  gfx950 only: 64-wide wavefronts, v_mfma_f32_16x16x32_f16,
// v_mfma_f32_16x16x4_f32, LDS.  No CUDA compatibility paths.
//
// k_generic.hip: the per-layer kernels of the generic schedule (EfficientNet-B4, MMC_FUSE=0) and the head: stem_conv, pw_gemm,
// pw_gemm_fp8, dwconv, squeeze-excite, the calibrated MLP head, crop (mbconv_a / mbconv_d: k_mbconv.hip).
//
// Data layout in HBM: activations are NHWC fp16 ([patch][y][x][channel]); channel counts are
// multiples of 8 so every lane moves 16-byte vectors.  Accumulation is always fp32.
//
// What each kernel replaces in the reference's call graph (pyspacer EfficientNet.extract_features,
// invoked at scripts/build_feature_bucket.py:434):
//   stem_conv_kernel   transformation() + _conv_stem + _bn0 + swish
//   pw_gemm_kernel     _expand_conv+_bn0+swish | SE-scale + _project_conv+_bn2(+skip) | _conv_head+_bn1+swish+avgpool
//   dwconv_kernel      _depthwise_conv + _bn1 + swish, plus the squeeze-excite partial sums
//   se_gate_kernel     adaptive_avg_pool2d + _se_reduce + swish + _se_expand + sigmoid
//   mlp_gemm_f32_kernel / calibrate_kernel   CalibratedHead.forward (inference/head.py:66-89)
//   calibrate_topk_kernel   the same + the per-point sorted(...)[:k] of AnnotationRun (pyspacer/annotation.py:251-261)
//   calibrate_eval_kernel   the same + per-row est / score / rank / p_true and the integer totals of a validation pass
//                           (pyspacer/trainer.py:271-291, metrics/ranking.py:54-65, metrics/probability.py:47-49)
//   crop_kernel        pyspacer crop_patches (reflect pad + slice)
#include "device_common.h"
#include "topk_key.h"

// ---------------------------------------------------------------------------------------------
// Stem: u8 HWC patch -> conv3x3 stride 2 (TF-same: pad right/bottom by 1) -> +bias -> SiLU -> fp16
// One workgroup = 16x16 output pixels of one patch; wave w owns output rows 4w..4w+3, one MFMA
// fragment (16 pixels x 32 channels) per row.  The 33x33x3 input tile is staged in LDS as exact
// fp16 integers (u8 - 128); normalisation (x/255-mean)/std is folded into weights and bias on the
// host, and padded pixels hold 255*mean-128 so they contribute exactly the folded zero.
// K packing (32 slots = 4 lane-quarters x 8): quarter q<3 = kernel row q, bytes 0..7 of the 9-byte
// (kx,c) run; quarter 3 = byte 8 of rows 0,1,2 then zeros.  Weights are packed to match on the host.
// ---------------------------------------------------------------------------------------------
#define STEM_TILE 16
#define STEM_IN (2 * STEM_TILE + 1)   // 33
#define STEM_ROWH 104                 // halves per LDS row (99 used), keeps rows 16-B aligned

template <int NT>   // NT fragments of 16 output channels: 2 for B0 (32), 3 for B4 (48)
__global__ __launch_bounds__(256) void stem_conv_kernel(const uint8_t* __restrict__ patches,  // [B][224][224][3]
                                                        const _Float16* __restrict__ w,        // [16 NT][32] (n, kslot)
                                                        const float* __restrict__ bias,        // [16 NT]
                                                        const float* __restrict__ padval,      // [3]  255*mean-128
                                                        _Float16* __restrict__ out)            // [B][112][112][16 NT]
{
    __shared__ __attribute__((aligned(16))) _Float16 tile[STEM_IN * STEM_ROWH];
    const int tx = blockIdx.x, ty = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x;
    const uint8_t* img = patches + (size_t)b * (224 * 224 * 3);
    const int iy0 = ty * 32, ix0 = tx * 32;
    const float pv0 = padval[0], pv1 = padval[1], pv2 = padval[2];
    // stage: 33 rows x 25 dwords
    for (int i = tid; i < STEM_IN * 25; i += 256) {
        const int r = i / 25, d = i - r * 25;
        const int iy = iy0 + r;
        const int boff = ix0 * 3 + d * 4;  // byte offset inside the image row
        uint32_t word = 0;
        const bool row_ok = iy < 224;
        if (row_ok && boff < 672) word = *reinterpret_cast<const uint32_t*>(img + (size_t)iy * 672 + boff);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int bb = d * 4 + e;  // byte inside the tile row
            if (bb < 99) {
                const int col = ix0 + bb / 3;
                const int c = bb % 3;
                float v;
                if (row_ok && col < 224) v = (float)((word >> (8 * e)) & 0xffu) - 128.0f;
                else v = (c == 0) ? pv0 : (c == 1 ? pv1 : pv2);
                tile[r * STEM_ROWH + bb] = (_Float16)v;
            }
        }
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, q = lane >> 4;
    // weight fragments (A operand): rows = output channels
    h8 wf[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) wf[t] = *reinterpret_cast<const h8*>(w + (t * 16 + m) * 32 + q * 8);
    float bs[4 * NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) bs[t * 4 + j] = bias[q * 4 * NT + t * 4 + j];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const int oyl = wave * 4 + f;  // local output row
        h8 a;
        if (q < 3) {
            const _Float16* src = tile + (2 * oyl + q) * STEM_ROWH + 6 * m;
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = src[j];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = (_Float16)0.0f;
#pragma unroll
            for (int j = 0; j < 3; ++j) a[j] = tile[(2 * oyl + j) * STEM_ROWH + 6 * m + 8];
        }
        f4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            acc[t] = (f4){bs[t * 4], bs[t * 4 + 1], bs[t * 4 + 2], bs[t * 4 + 3]};  // bias = accumulator init
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[t], a, acc[t], 0, 0, 0);
        }
        const int oy = ty * 16 + oyl, ox = tx * 16 + m;
        _Float16* op = out + (((size_t)b * 112 + oy) * 112 + ox) * (16 * NT) + q * 4 * NT;
        if (NT == 2) {
            h8 o;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) o[t * 4 + j] = (_Float16)silu_scaled(acc[t][j]);
            *reinterpret_cast<h8*>(op) = o;
        } else {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                h4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = (_Float16)silu_scaled(acc[t][j]);
                *reinterpret_cast<h4*>(op + 4 * t) = o;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Pointwise (1x1) convolution as an MFMA GEMM:  Y[m][n] = epi( sum_k X[m][k] * W[n][k] + bias[n] ).
// Operands are swapped (weights = MFMA A operand, activations = B operand) so that the fp32 result
// fragment holds, per lane, 4*NT CONSECUTIVE output channels of one pixel -> 8-byte stores that
// coalesce to full lines.  Within a chunk of 16*NT channels the host permutes weight rows:
//   fragment row (t*16 + 4q + j)  <->  channel (chunk*16NT + q*4NT + 4t + j).
// Weights are packed on the host in FRAGMENT ORDER: the 1 KB a wave feeds to one MFMA (16 rows x
// 32 k, lane-linear) is contiguous, at ((chunk*KS32 + kstep)*NT + t) KB.  A workgroup (4 waves,
// 64*MT rows, one chunk) stages UK k-steps of weight fragments per batch through LDS with perfectly
// coalesced 16-byte copies, so each fragment leaves L2 once per workgroup instead of once per wave,
// and reads them back with conflict-free lane-linear ds_read_b128.  Activation fragments go straight
// from HBM/L2 to registers (each wave owns its rows), one batch ahead of the MFMAs.
// EPI_SILU   : y = silu(acc+bias)                              (expand conv)
// EPI_LINEAR : y = acc+bias (+ residual)                       (project conv), optional SE gate on X
// EPI_GAP    : out[patch][n] = mean over the patch's HW rows of silu(acc+bias)   (head conv + avgpool)
// ---------------------------------------------------------------------------------------------
template <int MT, int NT, int EPI, bool GATE, bool RES, int UK, bool DG>
__global__ __launch_bounds__(256) void pw_gemm_kernel(const _Float16* __restrict__ X, int M, int K,
                                                      const _Float16* __restrict__ Wp, int KS32,
                                                      const float* __restrict__ bias,  // natural channel order, zero padded
                                                      _Float16* __restrict__ Y, int N,
                                                      const float* __restrict__ gate,  // [patch][K] fp32
                                                      int HW,
                                                      const _Float16* __restrict__ res,
                                                      float* __restrict__ gap_out, float inv_hw)
{
    constexpr int NFRAG = UK * NT;             // weight fragments per batch
    constexpr int NPASS = (NFRAG + 3) / 4;     // 4 waves copy one fragment each per pass
    __shared__ __attribute__((aligned(16))) _Float16 wlds[NFRAG * 512];
    __shared__ float red[EPI == EPI_GAP ? 4 * 16 * NT : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, q = lane >> 4;
    const int chunk = blockIdx.y;
    const _Float16* wsrc = Wp + (size_t)chunk * KS32 * NT * 512 + lane * 8;
    int row[MT];
    bool rok[MT];
    int gpatch[MT];
    if (EPI == EPI_GAP) {
        // one workgroup = one patch; rows beyond HW are masked
        const int ml = wave * 16 + m;
        row[0] = blockIdx.x * HW + ml;
        rok[0] = ml < HW;
        gpatch[0] = blockIdx.x;
    } else {
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            row[i] = (blockIdx.x * 4 + wave) * (16 * MT) + i * 16 + m;
            rok[i] = row[i] < M;
            gpatch[i] = GATE ? (rok[i] ? row[i] / HW : 0) : 0;
        }
    }
    // bias is the accumulator's initial value: lane (m,q) owns channels cbase + 4t + j
    const int cbase = chunk * 16 * NT + q * 4 * NT;
    f4 acc[MT][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const f4 bv = *reinterpret_cast<const f4*>(bias + cbase + 4 * t);
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i][t] = bv;
    }

    const int nbatch = (KS32 + UK - 1) / UK;
    uint4 wst[NPASS];   // weight staging registers (global -> regs -> LDS)
    h8 xf[UK][MT];      // activation fragments of the current batch
    auto load_w = [&](int bt) {
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int f = ps * 4 + wave;                 // fragment index inside the batch: u*NT + t
            const int ks = bt * UK + f / NT;
            uint4 v = {0u, 0u, 0u, 0u};
            if (f < NFRAG && ks < KS32)
                v = *reinterpret_cast<const uint4*>(wsrc + ((size_t)(bt * UK) * NT + f) * 512);
            wst[ps] = v;
        }
    };
    // DG (defer gate; used by the small-M 7x7 layers, which are latency- not occupancy-bound): activation
    // fragments and their fp32 squeeze-excite gates are only LOADED in load_x; the multiply happens in
    // apply_gate() right before the MFMAs that consume them, so the loads of batch bt+1 really overlap the
    // MFMAs of batch bt.  !DG multiplies at load time (waits for the data, but keeps 8 fewer VGPRs per
    // fragment alive, which is what the large-M layers want).
    constexpr int GN = (GATE && DG) ? 2 : 1;
    auto load_x = [&](int bt, h8 (&dst)[UK][MT], f4 (&g)[UK][MT][GN]) {
#pragma unroll
        for (int u = 0; u < UK; ++u) {
            const int k = (bt * UK + u) * 32 + q * 8;
            const bool kok = k < K;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (kok && rok[i]) v = *reinterpret_cast<const h8*>(X + (size_t)row[i] * K + k);
                if (GATE) {
                    f4 g0 = {0.f, 0.f, 0.f, 0.f}, g1 = g0;
                    if (kok && rok[i]) {
                        g0 = *reinterpret_cast<const f4*>(gate + (size_t)gpatch[i] * K + k);
                        g1 = *reinterpret_cast<const f4*>(gate + (size_t)gpatch[i] * K + k + 4);
                    }
                    if (DG) {
                        g[u][i][0] = g0;
                        g[u][i][GN - 1] = g1;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            v[j] = (_Float16)((float)v[j] * g0[j]);
                            v[4 + j] = (_Float16)((float)v[4 + j] * g1[j]);
                        }
                    }
                }
                dst[u][i] = v;
            }
        }
    };
    auto apply_gate = [&](h8 (&x)[UK][MT], f4 (&g)[UK][MT][GN]) {
        if (!(GATE && DG)) return;
#pragma unroll
        for (int u = 0; u < UK; ++u)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    x[u][i][j] = (_Float16)((float)x[u][i][j] * g[u][i][0][j]);
                    x[u][i][4 + j] = (_Float16)((float)x[u][i][4 + j] * g[u][i][GN - 1][j]);
                }
    };
    f4 gf[UK][MT][GN];
    load_w(0);
    load_x(0, xf, gf);
    for (int bt = 0; bt < nbatch; ++bt) {
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int f = ps * 4 + wave;
            if (f < NFRAG) *reinterpret_cast<uint4*>(wlds + f * 512 + lane * 8) = wst[ps];
        }
        apply_gate(xf, gf);
        __syncthreads();
        h8 xn[UK][MT];
        f4 gn[UK][MT][GN];
        const bool more = bt + 1 < nbatch;
        if (more) {  // next batch's global loads fly during this batch's MFMAs
            load_w(bt + 1);
            load_x(bt + 1, xn, gn);
        }
#pragma unroll
        for (int u = 0; u < UK; ++u) {
            if (bt * UK + u < KS32) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const h8 wf = *reinterpret_cast<const h8*>(wlds + (u * NT + t) * 512 + lane * 8);
#pragma unroll
                    for (int i = 0; i < MT; ++i)
                        acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[u][i], acc[i][t], 0, 0, 0);
                }
            }
        }
        __syncthreads();
        if (more) {
#pragma unroll
            for (int u = 0; u < UK; ++u)
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    xf[u][i] = xn[u][i];
#pragma unroll
                    for (int e = 0; e < GN; ++e) gf[u][i][e] = gn[u][i][e];
                }
        }
    }
    // epilogue: lane (m,q) holds channels cbase + 4t + j of pixel row[i]; acc already includes the bias
    if (EPI == EPI_GAP) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = row16_sum(rok[0] ? silu_scaled(acc[0][t][j]) : 0.0f);
                if (m == 0) red[wave * 16 * NT + q * 4 * NT + 4 * t + j] = v;
            }
        __syncthreads();
        if (tid < 16 * NT) {
            const float s = ((red[tid] + red[16 * NT + tid]) + (red[32 * NT + tid] + red[48 * NT + tid])) * inv_hw;
            const int c = chunk * 16 * NT + tid;
            if (c < N) gap_out[(size_t)blockIdx.x * N + c] = s;
        }
        return;
    }
    // skip-connection operands: ALL of them requested before the first is used (unconditional, clamped addresses) -- inside the
    // row / channel conditions below every load was followed by its own s_waitcnt vmcnt(0): MT x NT exposed round trips per workgroup
    h4 rres[MT][NT];
    if (RES) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int c = cbase + 4 * t;
                rres[i][t] = *reinterpret_cast<const h4*>(res + (size_t)(rok[i] ? row[i] : 0) * N + (c < N ? c : 0));
            }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        if (!rok[i]) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = cbase + 4 * t;
            if (c < N) {  // N is a multiple of 4
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = acc[i][t][j];
                if (EPI == EPI_SILU) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = silu_scaled(v[j]);
                }
                if (RES) {
                    const h4 r = rres[i][t];
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] += (float)r[j];
                }
                h4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = (_Float16)v[j];
                *reinterpret_cast<h4*>(Y + (size_t)row[i] * N + c) = o;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// pw_gemm_fp8_kernel: SE-scale + project conv (+ skip) on fp8 MFMA operands -- BASELINE.json configs[4] ("EfficientNet-B4, fp8
// weights/activations on CDNA4 fp8 MFMA"; not in the reference).  v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 operands and unit
// block scales: K = 128 per instruction at twice the fp16 rate (tools/ubench/mfma_f8.hip: layout and cycles).
//   weights      e4m3, one fp32 scale per output channel (amax / 448), quantised and packed in fragment order on the host
//   activations  the fp16 depthwise output times its fp32 squeeze-excite gate, one fp32 scale per pixel row (amax / 447 of the
//                gated row), quantised here: pass 1 reads the row for its maximum, pass 2 reads it again (L2 / Infinity Cache),
//                scales, converts (v_cvt_pk_fp8_f32) and feeds the MFMAs
//   epilogue     y = acc * row scale * channel scale + bias (+ skip) -> fp16
// Operands are swapped as in pw_gemm_kernel (A = weights, B = pixels): a lane ends up with 4 consecutive channels of one pixel.
// One workgroup = 4 waves x 16 pixel rows x NT output fragments.
// ---------------------------------------------------------------------------------------------
typedef int v8i __attribute__((ext_vector_type(8)));
template <int NT, bool RES>
__global__ __launch_bounds__(256) void pw_gemm_fp8_kernel(Fp8GemmArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, q = lane >> 4;
    const int row = (blockIdx.x * 4 + wave) * 16 + m;
    const bool rok = row < a.M;
    const int rowc = rok ? row : a.M - 1;
    const _Float16* xr = a.X + (size_t)rowc * a.K;
    const float* gr = a.gate + (size_t)(rowc / a.HW) * a.K;
    const int f0 = blockIdx.y * NT;
    // one k-step of this lane: 32 channels from 128 ks + 32 q, as x * gate in fp32 (zeros past K)
    auto gated = [&](int ks, float (&v)[32]) {
        const int k0 = 128 * ks + 32 * q;
#pragma unroll
        for (int c8 = 0; c8 < 4; ++c8) {
            const int k = k0 + 8 * c8;
            h8 x = {0, 0, 0, 0, 0, 0, 0, 0};
            f4 g0 = {0.f, 0.f, 0.f, 0.f}, g1 = g0;
            if (k < a.K) {
                x = *reinterpret_cast<const h8*>(xr + k);
                g0 = *reinterpret_cast<const f4*>(gr + k);
                g1 = *reinterpret_cast<const f4*>(gr + k + 4);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[8 * c8 + j] = (float)x[j] * g0[j]; v[8 * c8 + 4 + j] = (float)x[4 + j] * g1[j]; }
        }
    };
    // ---- pass 1: the row's largest magnitude ----
    float mx = 0.f;
    for (int ks = 0; ks < a.KS128; ++ks) {
        float v[32];
        gated(ks, v);
#pragma unroll
        for (int e = 0; e < 32; e += 2) mx = __builtin_fmaxf(mx, __builtin_fmaxf(__builtin_fabsf(v[e]), __builtin_fabsf(v[e + 1])));
    }
    mx = __builtin_fmaxf(mx, __shfl_xor(mx, 16));
    mx = __builtin_fmaxf(mx, __shfl_xor(mx, 32));
    // 447 (not 448): the scaled maximum stays below e4m3's largest finite value after fp32 rounding
    const float inv = mx > 0.f ? 447.0f / mx : 0.f;
    const float sx = mx > 0.f ? mx * (1.0f / 447.0f) : 0.f;
    // ---- pass 2: quantise and multiply ----
    f4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};
    const uint8_t* wl = a.W8 + (size_t)lane * 32;
    for (int ks = 0; ks < a.KS128; ++ks) {
        float v[32];
        gated(ks, v);
        v8i bq;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            int w = 0;
            w = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * d] * inv, v[4 * d + 1] * inv, w, false);
            w = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * d + 2] * inv, v[4 * d + 3] * inv, w, true);
            bq[d] = w;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const uint8_t* wp = wl + ((size_t)(f0 + t) * a.KS128 + ks) * 2048;
            union { uint4 u[2]; v8i v; } aw;
            aw.u[0] = *reinterpret_cast<const uint4*>(wp);
            aw.u[1] = *reinterpret_cast<const uint4*>(wp + 16);
            acc[t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(aw.v, bq, acc[t], 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
        }
    }
    // ---- epilogue: lane (m, q) holds channels 16 (f0 + t) + 4 q + j of pixel row m ----
    if (!rok) return;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = 16 * (f0 + t) + 4 * q;
        if (c >= a.N) continue;   // N is a multiple of 4
        const f4 sw = *reinterpret_cast<const f4*>(a.sw + c), bv = *reinterpret_cast<const f4*>(a.bias + c);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = acc[t][j] * sx * sw[j] + bv[j];
        if (RES) {
            const h4 r = *reinterpret_cast<const h4*>(a.res + (size_t)row * a.N + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += (float)r[j];
        }
        h4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (_Float16)v[j];
        *reinterpret_cast<h4*>(a.Y + (size_t)row * a.N + c) = o;
    }
}

// ---------------------------------------------------------------------------------------------
// Depthwise KSxKS convolution, stride ST, TF-same padding, + bias (BN folded) + SiLU, fp16 out,
// plus per-(patch, channel) partial sums of the fp32 SiLU outputs for squeeze-excite.
// Thread = 8 channels x TW consecutive output pixels of one row; channel-group index is the fastest
// thread index so neighbouring lanes read neighbouring 16-byte vectors (coalesced NHWC).
// blockDim.x = CG*S (CG = channel groups of 8 per workgroup = C/8/gridDim.z, S strips per pass).  Partial sums are reduced through
// LDS in a fixed order and written to pool_part[patch][blockIdx.x][C] (deterministic, no atomics).
// ---------------------------------------------------------------------------------------------
template <int KS, int ST, int TW>
__global__ __launch_bounds__(256) void dwconv_kernel(const _Float16* __restrict__ in,  // [B][H][W][C]
                                                     const float* __restrict__ wt,     // [KS*KS][C]
                                                     const float* __restrict__ bias,   // [C]
                                                     _Float16* __restrict__ out,       // [B][Ho][Wo][C]
                                                     float* __restrict__ pool_part,    // [B][gridDim.x][C]
                                                     int H, int W, int C, int Ho, int Wo, int pad_t, int pad_l,
                                                     int CG, int S, int iters)
{
    extern __shared__ __attribute__((aligned(16))) float red[];  // [S][8 CG]
    const int tid = threadIdx.x;
    const int cg = tid % CG, s = tid / CG;
    const int b = blockIdx.y;
    const int strips_per_row = Wo / TW;
    const int nstrips = Ho * strips_per_row;
    const int coff = blockIdx.z * CG * 8;   // layers wider than 2048 channels split their channel groups over z
    const int CL = CG * 8;
    const int c0 = coff + cg * 8;
    const _Float16* inb = in + (size_t)b * H * W * C + c0;
    _Float16* outb = out + (size_t)b * Ho * Wo * C + c0;
    float bs[8];
    {
        const f4 b0 = *reinterpret_cast<const f4*>(bias + c0);
        const f4 b1 = *reinterpret_cast<const f4*>(bias + c0 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { bs[j] = b0[j]; bs[4 + j] = b1[j]; }
    }
    float pooled[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) pooled[j] = 0.f;
    constexpr int NX = (TW - 1) * ST + KS;  // input columns a strip touches
    for (int it = 0; it < iters; ++it) {
        const int strip = (blockIdx.x * iters + it) * S + s;
        if (strip < nstrips) {
            const int oy = strip / strips_per_row;
            const int ox0 = (strip - oy * strips_per_row) * TW;
            float acc[TW][8];
#pragma unroll
            for (int t = 0; t < TW; ++t)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[t][j] = bs[j];
#pragma unroll 1
            for (int ky = 0; ky < KS; ++ky) {
                const int iy = oy * ST - pad_t + ky;
                if (iy < 0 || iy >= H) continue;
                const _Float16* rowp = inb + (size_t)iy * W * C;
                float wk[KS][8];
#pragma unroll
                for (int kx = 0; kx < KS; ++kx) {
                    const f4 w0 = *reinterpret_cast<const f4*>(wt + (size_t)(ky * KS + kx) * C + c0);
                    const f4 w1 = *reinterpret_cast<const f4*>(wt + (size_t)(ky * KS + kx) * C + c0 + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { wk[kx][j] = w0[j]; wk[kx][4 + j] = w1[j]; }
                }
#pragma unroll
                for (int xr = 0; xr < NX; ++xr) {
                    const int ix = ox0 * ST - pad_l + xr;
                    h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (ix >= 0 && ix < W) v = *reinterpret_cast<const h8*>(rowp + (size_t)ix * C);
                    float vf[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) vf[j] = (float)v[j];
#pragma unroll
                    for (int t = 0; t < TW; ++t) {
                        const int kx = xr - t * ST;
                        if (kx >= 0 && kx < KS) {
#pragma unroll
                            for (int j = 0; j < 8; ++j) acc[t][j] = __builtin_fmaf(vf[j], wk[kx][j], acc[t][j]);
                        }
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < TW; ++t) {
                h8 o;
                silu_scaled_staged(acc[t]);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float y = acc[t][j];
                    pooled[j] += y;
                    o[j] = (_Float16)y;
                }
                *reinterpret_cast<h8*>(outb + ((size_t)oy * Wo + ox0 + t) * C) = o;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[s * CL + cg * 8 + j] = pooled[j];
    __syncthreads();
    for (int c = tid; c < CL; c += blockDim.x) {
        float sum = 0.f;
        for (int ss = 0; ss < S; ++ss) sum += red[ss * CL + c];
        pool_part[((size_t)b * gridDim.x + blockIdx.x) * C + coff + c] = sum;
    }
}

// ---------------------------------------------------------------------------------------------
// Squeeze-excite in ONE launch: both FCs for 16 patches per workgroup of 16 waves.  The two tiny
// GEMMs are pure latency chains, so the workgroup is wide instead of deep:
//   FC1  r[16][Cs4] = silu(br + P[16][C] . Wr^T): the 16 waves split K (each sums its pool-partial slabs on
//        the fly and issues all its loads before its exact-f32 MFMAs), partials meet in LDS;
//   FC2  gate[16][C] = sigmoid(be + r . We^T): the 16 waves split the C/16 output fragments, r comes from LDS.
// ---------------------------------------------------------------------------------------------
#define SE_MAXG 5   // k-groups (16 k each) a wave may own in FC1: C <= 16 waves * 5 * 16 = 1280
#define SE_MAXT 1   // output fragments a wave may own in FC2 (after the gridDim.y split)
// Weights are fp32 (fp16 storage was tried: the gate error it causes is coherent per channel and
// roughly doubled the end-to-end feature error), packed in MFMA fragment order (16 bytes per lane,
// 1 KB per fragment, contiguous -> perfectly coalesced loads):
//   WrP[(g*3 + t)*64 + lane][4] = Wr[16t + i][16g + 4q .. +4]      (zero for j >= Cs, carries 1/(HW log2e))
//   WeP[(T*3 + g)*64 + lane][4] = We[16T + i][16g + 4q .. +4]      (zero for k >= Cs)
// gridDim = (ceil(M/16), NSPLIT): every y-slice recomputes FC1 (cheap) and owns 1/NSPLIT of FC2's outputs,
// so the weight stream of one patch group is spread over NSPLIT compute units.
template <int MAXG>
__global__ __launch_bounds__(1024) void se_fused_kernel(const float* __restrict__ pool_part, int nslab, int M, int C,
                                                        int Cs4, const float* __restrict__ WrP,
                                                        const float* __restrict__ br,  // [48] zero padded
                                                        const float* __restrict__ WeP,
                                                        const float* __restrict__ be, float* __restrict__ gate)
{
    __shared__ __attribute__((aligned(16))) float part[16][16][48];  // [wave][row][j]
    __shared__ __attribute__((aligned(16))) float rs[16][48];        // [row][j]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int row = blockIdx.x * 16 + i;
    const bool rok = row < M;
    const int NG = C >> 4;            // k-groups of FC1 == output fragments of FC2
    const int per_y = (NG + gridDim.y - 1) / gridDim.y;
    const int t_lo = blockIdx.y * per_y;
    const int t_hi = (t_lo + per_y) < NG ? (t_lo + per_y) : NG;
    // FC2's weight fragments and bias do not depend on FC1: issue their loads first so the whole kernel
    // is one memory round trip (pool partials, Wr, We, be all in flight together)
    f4 we[SE_MAXT][3];
    f4 bev[SE_MAXT];
#pragma unroll
    for (int u = 0; u < SE_MAXT; ++u) {
        const int T = t_lo + wave + 16 * u;
        bev[u] = (f4){0.f, 0.f, 0.f, 0.f};
        if (T < t_hi) bev[u] = *reinterpret_cast<const f4*>(be + T * 16 + 4 * q);
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            f4 w = {0.f, 0.f, 0.f, 0.f};
            if (T < t_hi) w = *reinterpret_cast<const f4*>(WeP + ((size_t)(T * 3 + g) * 64 + lane) * 4);
            we[u][g] = w;
        }
    }
    // ---- FC1: this wave owns k-groups g = wave, wave+16, ... ----
    {
        f4 xv[MAXG];
        f4 wv[MAXG][3];
#pragma unroll
        for (int u = 0; u < MAXG; ++u) {
            const int g = wave + 16 * u;
            const bool gok = g < NG;
            const int k = g * 16 + 4 * q;
            f4 x = {0.f, 0.f, 0.f, 0.f};
            if (rok && gok) {
                const float* xp = pool_part + (size_t)row * nslab * C + k;
                f4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
                int p = 0;
                if (MAXG <= 2) {   // early blocks: many slabs, few channels -> 16 independent loads per round trip
                    for (; p + 15 < nslab; p += 16) {
                        f4 v[16];
#pragma unroll
                        for (int e = 0; e < 16; ++e) v[e] = *reinterpret_cast<const f4*>(xp + (size_t)(p + e) * C);
#pragma unroll
                        for (int e = 0; e < 16; e += 4) {
                            s0 += v[e];
                            s1 += v[e + 1];
                            s2 += v[e + 2];
                            s3 += v[e + 3];
                        }
                    }
                }
                for (; p + 3 < nslab; p += 4) {
                    s0 += *reinterpret_cast<const f4*>(xp + (size_t)p * C);
                    s1 += *reinterpret_cast<const f4*>(xp + (size_t)(p + 1) * C);
                    s2 += *reinterpret_cast<const f4*>(xp + (size_t)(p + 2) * C);
                    s3 += *reinterpret_cast<const f4*>(xp + (size_t)(p + 3) * C);
                }
                for (; p < nslab; ++p) s0 += *reinterpret_cast<const f4*>(xp + (size_t)p * C);
                x = (s0 + s1) + (s2 + s3);
            }
            xv[u] = x;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                f4 w = {0.f, 0.f, 0.f, 0.f};
                if (gok) w = *reinterpret_cast<const f4*>(WrP + ((size_t)(g * 3 + t) * 64 + lane) * 4);
                wv[u][t] = w;
            }
        }
        f4 acc[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[t] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < MAXG; ++u)
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u][t][s], xv[u][s], acc[t], 0, 0, 0);
        // lane (i,q) holds outputs j = 16t + 4q + jj of row i
#pragma unroll
        for (int t = 0; t < 3; ++t) *reinterpret_cast<f4*>(&part[wave][i][16 * t + 4 * q]) = acc[t];
    }
    __syncthreads();
    if (tid < 16 * 48) {
        const int r = tid / 48, j = tid - r * 48;
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) s += part[w][r][j];
        rs[r][j] = (j < Cs4) ? silu_f(s + br[j]) : 0.f;
    }
    __syncthreads();
    // ---- FC2: output fragments T = y*per_y + wave + 16u ----
    {
        f4 xr[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) xr[g] = *reinterpret_cast<const f4*>(&rs[i][g * 16 + 4 * q]);
#pragma unroll
        for (int u = 0; u < SE_MAXT; ++u) {
            const int T = t_lo + wave + 16 * u;
            if (T >= t_hi) break;
            f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(we[u][g][s], xr[g][s], acc, 0, 0, 0);
            if (rok) {
                const int n = T * 16 + 4 * q;
                const f4 bv = bev[u];
                f4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = sigmoid_f(acc[j] + bv[j]);
                *reinterpret_cast<f4*>(gate + (size_t)row * C + n) = o;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// se_small_kernel: squeeze-excite for the early blocks (C <= 256 channels, Cs <= 16 squeeze units), one patch per
// 256-thread workgroup.  The work is tiny (b0: 32x8, b1: 96x4, b2: 144x6 MACs per FC), what matters is that the
// launch gets onto the chip at once while the other lane's big kernels fill it: a 16-wave / 52 KB workgroup of
// se_fused_kernel has to wait for a whole compute unit to drain, a 4-wave / 1 KB one fits anywhere.
// fp32 throughout, natural weight layouts, fixed summation order (slab sums in 4 chains, wave butterfly for FC1).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void se_small_kernel(const float* __restrict__ pool_part, int nparts, int C, int Cs,
                                                       const float* __restrict__ wr,   // [Cs][C], carries 1/(HW log2e)
                                                       const float* __restrict__ br,   // [Cs]
                                                       const float* __restrict__ we,   // [C][Cs]
                                                       const float* __restrict__ be,   // [C]
                                                       float* __restrict__ gate)       // [B][C]
{
    // (Round 3 re-tried both FCs' operands requested at the top, this time unconditionally from clamped addresses: 9.7 / 7.5 / 6.8 us against
    // 6.9 / 6.7 / 7.3 -- the 36 extra requests per thread in front of block 0's 49 pool partials cost more than the two round trips they hide.)
    __shared__ float pooled[256];
    __shared__ float rs[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    if (tid < C) {
        const float* pp = pool_part + (size_t)b * nparts * C + tid;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int p = 0;
#pragma unroll 4   // 16 partials in flight per round trip (block 0 has 49 tiles: twelve dependent round trips otherwise); same sums
        for (; p + 3 < nparts; p += 4) {
            s0 += pp[(size_t)p * C];
            s1 += pp[(size_t)(p + 1) * C];
            s2 += pp[(size_t)(p + 2) * C];
            s3 += pp[(size_t)(p + 3) * C];
        }
        for (; p < nparts; ++p) s0 += pp[(size_t)p * C];
        pooled[tid] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    for (int j = wave; j < Cs; j += 4) {
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s = __builtin_fmaf(pooled[c], wr[(size_t)j * C + c], s);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) rs[j] = silu_f(s + br[j]);
    }
    __syncthreads();
    if (tid < C) {
        float acc = be[tid];
        for (int j = 0; j < Cs; ++j) acc = __builtin_fmaf(rs[j], we[(size_t)tid * Cs + j], acc);
        gate[(size_t)b * C + tid] = sigmoid_f(acc);
    }
}

// se_wide_kernel: the same computation without the size limits (any C, any Cs; pooled vector and squeeze units in
// dynamic LDS) -- the squeeze-excite of the generic per-layer schedule (EfficientNet-B4: C <= 2688, Cs <= 112).  One workgroup
// per patch.
__global__ __launch_bounds__(1024) void se_wide_kernel(const float* __restrict__ pool_part, int nparts, int C, int Cs,
                                                      const float* __restrict__ wr,   // [Cs][C], carries 1/(HW log2e)
                                                      const float* __restrict__ br,   // [Cs]
                                                      const float* __restrict__ we,   // [Cs][C] (transposed: lanes read neighbours)
                                                      const float* __restrict__ be,   // [C]
                                                      float* __restrict__ gate)       // [B][C]
{
    extern __shared__ float se_sm[];
    float* pooled = se_sm;            // [C]
    float* rs = se_sm + C;            // [Cs]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    for (int c = tid; c < C; c += 1024) {
        const float* pp = pool_part + (size_t)b * nparts * C + c;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int p = 0;
        for (; p + 3 < nparts; p += 4) {
            s0 += pp[(size_t)p * C];
            s1 += pp[(size_t)(p + 1) * C];
            s2 += pp[(size_t)(p + 2) * C];
            s3 += pp[(size_t)(p + 3) * C];
        }
        for (; p < nparts; ++p) s0 += pp[(size_t)p * C];
        pooled[c] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    for (int j = wave; j < Cs; j += 16) {   // 16 waves: the FC1 rows are a latency chain per wave
        float s = 0.f;
        // sixteen weights requested per round trip (unconditional, clamped; round 3: the loop was load -> wait -> fma, one exposed L2
        // round trip per 64 channels -- up to 42 per row); the products are summed in the same order as before
        for (int c0 = lane; c0 < C; c0 += 1024) {
            float w[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) w[u] = wr[(size_t)j * C + (c0 + 64 * u < C ? c0 + 64 * u : C - 1)];
            // (the pool sums of eight channels per LDS round trip: read inside the FMA loop they were one exposed round trip per FMA)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int c = c0 + 64 * (8 * h + u);
                    x[u] = pooled[c < C ? c : C - 1];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int c = c0 + 64 * (8 * h + u);
                    s = c < C ? __builtin_fmaf(x[u], w[8 * h + u], s) : s;
                }
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) rs[j] = silu_f(s + br[j]);
    }
    __syncthreads();
    // excite FC: a thread's (up to three) channels advance together, sixteen squeeze units per round trip: 48 requests in flight
    // (round 3: one request, one wait, one fma -- up to 3 x 112 exposed L2 round trips per thread); same summation order per channel
    {
        constexpr int NC = 3;   // C <= 3072
        float acc[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) acc[k] = be[tid + 1024 * k < C ? tid + 1024 * k : C - 1];
        for (int j0 = 0; j0 < Cs; j0 += 16) {
            float w[NC][16];
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const int c = tid + 1024 * k < C ? tid + 1024 * k : C - 1;
#pragma unroll
                for (int u = 0; u < 16; ++u) w[k][u] = we[(size_t)(j0 + u < Cs ? j0 + u : Cs - 1) * C + c];
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float r[8];   // (eight squeeze units per LDS round trip)
#pragma unroll
                for (int u = 0; u < 8; ++u) r[u] = rs[j0 + 8 * h + u < Cs ? j0 + 8 * h + u : Cs - 1];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int k = 0; k < NC; ++k)
                        acc[k] = j0 + 8 * h + u < Cs ? __builtin_fmaf(r[u], w[k][8 * h + u], acc[k]) : acc[k];
            }
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const int c = tid + 1024 * k;
            if (c < C) gate[(size_t)b * C + c] = sigmoid_f(acc[k]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Calibrated MLP head, fp32 end to end (the reference gate is max|dp| <= 1e-6, inference/export.py:31).
// Y[m][n] = act( sum_k X[m][k] W[n][k] + b[n] ) on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32).
// Lane (i=l&15, q=l>>4) loads 4 consecutive k of its row (16 B) and feeds element s at step s, so
// the 16 k of a group are covered by 4 MFMAs with both operands using the same k permutation.
// Workgroup = 4 waves; wave w owns rows [16*(4*bx+w), +16) and NT fragments of 16 output columns.
// ---------------------------------------------------------------------------------------------
template <int NT, bool RELU>
__global__ __launch_bounds__(256) void mlp_gemm_f32_kernel(const float* __restrict__ X, int M, int K,
                                                           const float* __restrict__ W, const float* __restrict__ bias,
                                                           float* __restrict__ Y, int N)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int row = (blockIdx.x * 4 + wave) * 16 + i;
    const bool rok = row < M;
    const int n0 = blockIdx.y * 16 * NT;
    // four independent accumulation chains per fragment (k-step s feeds chain s): shorter chains
    // than one 1280-long fma sequence -> less fp32 drift against the reference's blocked sgemm,
    // and no MFMA dependent-issue stalls.
    f4 acc[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[t][s] = (f4){0.f, 0.f, 0.f, 0.f};
    const int K16 = K & ~15;
    for (int k0 = 0; k0 < K16; k0 += 16) {
        f4 xv = {0.f, 0.f, 0.f, 0.f};
        if (rok) xv = *reinterpret_cast<const f4*>(X + (size_t)row * K + k0 + 4 * q);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n = n0 + t * 16 + i;
            f4 wv = {0.f, 0.f, 0.f, 0.f};
            if (n < N) wv = *reinterpret_cast<const f4*>(W + (size_t)n * K + k0 + 4 * q);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc[t][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[s], xv[s], acc[t][s], 0, 0, 0);
        }
    }
    if (K16 < K) {  // K tail: K is padded to a multiple of 4 by mmc_head_create
        f4 xv = {0.f, 0.f, 0.f, 0.f};
        const int k = K16 + 4 * q;
        if (rok && k < K) xv = *reinterpret_cast<const f4*>(X + (size_t)row * K + k);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n = n0 + t * 16 + i;
            f4 wv = {0.f, 0.f, 0.f, 0.f};
            if (n < N && k < K) wv = *reinterpret_cast<const f4*>(W + (size_t)n * K + k);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc[t][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[s], xv[s], acc[t][s], 0, 0, 0);
        }
    }
    // swapped operands: lane (i,q) holds outputs n = n0 + 16t + 4q + j of row `row`
    if (!rok) return;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + t * 16 + 4 * q + j;
            if (n < N) {
                float v = ((acc[t][0][j] + acc[t][1][j]) + (acc[t][2][j] + acc[t][3][j])) + bias[n];
                if (RELU) v = fmaxf(v, 0.f);
                Y[(size_t)row * N + n] = v;
            }
        }
}

// mlp_gemm_f32_group_kernel: one Linear layer of every member of a head ensemble in one launch (include/mmc.h, "head ensembles").
// Member blockIdx.z has its own operands and shape (MlpGroupArgs); the grid's y extent is the widest member's, and a workgroup past
// its member's N leaves.  An output element gets the arithmetic of mlp_gemm_f32_kernel<4, .> above, step for step: the same k order,
// the same four chains on v_mfma_f32_16x16x4_f32, the same ((a0 + a1) + (a2 + a3)) + bias -- so a member's logits have the bits
// of its own head's launches.  relu is per member: one member's last layer can sit beside another's hidden layer.
__global__ __launch_bounds__(256) void mlp_gemm_f32_group_kernel(MlpGroupArgs g)
{
    constexpr int NT = 4;
    const MlpGroupMember& mb = g.m[blockIdx.z];
    const int K = mb.K, N = mb.N, M = g.M;
    const int n0 = blockIdx.y * 16 * NT;
    if (n0 >= N) return;   // (workgroup-uniform)
    const float* __restrict__ X = mb.X;
    const float* __restrict__ W = mb.W;
    const float* __restrict__ bias = mb.bias;
    float* __restrict__ Y = mb.Y;
    const bool relu = mb.relu != 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int row = (blockIdx.x * 4 + wave) * 16 + i;
    const bool rok = row < M;
    f4 acc[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[t][s] = (f4){0.f, 0.f, 0.f, 0.f};
    const int K16 = K & ~15;
    for (int k0 = 0; k0 < K16; k0 += 16) {
        f4 xv = {0.f, 0.f, 0.f, 0.f};
        if (rok) xv = *reinterpret_cast<const f4*>(X + (size_t)row * K + k0 + 4 * q);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n = n0 + t * 16 + i;
            f4 wv = {0.f, 0.f, 0.f, 0.f};
            if (n < N) wv = *reinterpret_cast<const f4*>(W + (size_t)n * K + k0 + 4 * q);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc[t][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[s], xv[s], acc[t][s], 0, 0, 0);
        }
    }
    if (K16 < K) {  // K tail: K is padded to a multiple of 4 by mmc_head_create
        f4 xv = {0.f, 0.f, 0.f, 0.f};
        const int k = K16 + 4 * q;
        if (rok && k < K) xv = *reinterpret_cast<const f4*>(X + (size_t)row * K + k);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n = n0 + t * 16 + i;
            f4 wv = {0.f, 0.f, 0.f, 0.f};
            if (n < N && k < K) wv = *reinterpret_cast<const f4*>(W + (size_t)n * K + k);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc[t][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[s], xv[s], acc[t][s], 0, 0, 0);
        }
    }
    if (!rok) return;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + t * 16 + 4 * q + j;
            if (n < N) {
                float v = ((acc[t][0][j] + acc[t][1][j]) + (acc[t][2][j] + acc[t][3][j])) + bias[n];
                if (relu) v = fmaxf(v, 0.f);
                Y[(size_t)row * N + n] = v;
            }
        }
}

// The calibration arithmetic of CalibratedHead.forward (head.py:75-89), one wave per row, lane l owning classes l, l + 64, ...:
// softmax -> Platt sigmoid -> row normalise (uniform row when the sum is 0) -> sklearn overshoot clip.  calibrate_kernel and
// calibrate_topk_kernel are both built from these pieces, so a probability has the same bits whichever of them wrote it.
__device__ __forceinline__ float wave_max_f(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum_f(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the row's maximum logit and the sum of exp(x - max)
__device__ __forceinline__ void calib_softmax_stats(const float* __restrict__ x, int K, int lane, float& mx, float& se)
{
    mx = -INFINITY;
    for (int k = lane; k < K; k += 64) mx = fmaxf(mx, x[k]);
    mx = wave_max_f(mx);
    se = 0.f;
    for (int k = lane; k < K; k += 64) se += expf(x[k] - mx);
    se = wave_sum_f(se);
}
// one class before normalisation: sigmoid(-(a p + b)) of its softmax probability p
__device__ __forceinline__ float calib_sigmoid(float xk, float mx, float se, float ak, float bk)
{
    const float p = expf(xk - mx) / se;
    return 1.0f / (1.0f + expf(ak * p + bk));
}
// c / (row sum cs), the uniform row when cs is 0, values in (1, 1 + 1e-5] clipped to 1
__device__ __forceinline__ float calib_normalise(float c, float cs, int K)
{
    float v = (cs != 0.f) ? c / cs : 1.0f / (float)K;
    if (v > 1.0f && v <= 1.00001f) v = 1.0f;
    return v;
}

// One wave per row: the calibration above -> argmax (first maximum, like numpy/torch argmax).   head.py:75-89
__global__ __launch_bounds__(256) void calibrate_kernel(const float* __restrict__ logits, int M, int K,
                                                        const float* __restrict__ a, const float* __restrict__ bcal,
                                                        float* __restrict__ proba, int32_t* __restrict__ argmax_out)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* x = logits + (size_t)row * K;
    float mx, se;
    calib_softmax_stats(x, K, lane, mx, se);
    float cs = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float c = calib_sigmoid(x[k], mx, se, a[k], bcal[k]);
        proba[(size_t)row * K + k] = c;
        cs += c;
    }
    cs = wave_sum_f(cs);
    float best = -INFINITY;
    int besti = 0x7fffffff;
    for (int k = lane; k < K; k += 64) {
        const float v = calib_normalise(proba[(size_t)row * K + k], cs, K);
        proba[(size_t)row * K + k] = v;
        if (v > best) { best = v; besti = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(besti, o);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
    }
    if (argmax_out && lane == 0) argmax_out[row] = besti;
}

// ---------------------------------------------------------------------------------------------
// calibrate_topk_kernel: the same calibration, then the k best classes of the row in the order of the reference's
// sorted(zip(labels, proba), key=itemgetter(1), reverse=True)[:k] (mermaid_classifier/pyspacer/annotation.py:253-255): score
// descending, and -- the sort is stable -- equal scores in class order.
// One wave per row, four rows per workgroup.  A probability is >= 0, so its fp32 bit pattern orders like its value; the
// 64-bit key (bits << 32) | (0xFFFFFFFF - class) therefore orders a row exactly as the reference does, keys are distinct, and
// one wave-wide maximum per round picks the next class.  Nothing is marked as taken: keys leave in strictly decreasing order,
// so after a round the lane that owned the winner looks among its own classes for its largest key BELOW the winner -- which
// holds for every bit pattern, NaN included: k rounds, k distinct classes in [0, K), whatever the logits are.
// A lane only ever reads the row entries it wrote itself (classes lane, lane + 64, ...), so the row needs no barrier; it sits
// in a wave-private LDS row (ROW_IN_LDS: K <= TOPK_LDS_MAX_K, bank-conflict free) and is not re-read from HBM between rounds.
// Wider heads keep the same algorithm with the row in `rowbuf` (M x K floats in global memory: the caller's proba or scratch).
// ---------------------------------------------------------------------------------------------
#define TOPK_LDS_MAX_K 2048   // 4 rows x 2048 classes x 4 B = 32 KB of LDS per workgroup
// (topk_key: topk_key.h, shared with cover.hip)
template <bool ROW_IN_LDS>
__global__ __launch_bounds__(256) void calibrate_topk_kernel(const float* __restrict__ logits, int M, int K,
                                                             const float* __restrict__ a, const float* __restrict__ bcal, int k,
                                                             int32_t* __restrict__ idx_out,   // [M][k]
                                                             float* __restrict__ score_out,   // [M][k]
                                                             float* proba,                    // [M][K] or NULL
                                                             float* rowbuf)                   // [M][K] when !ROW_IN_LDS
{
    extern __shared__ float topk_rows[];   // [4][K] when ROW_IN_LDS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= M) return;
    const float* x = logits + (size_t)row * K;
    float* r = ROW_IN_LDS ? topk_rows + (size_t)wave * K : rowbuf + (size_t)row * K;
    float mx, se;
    calib_softmax_stats(x, K, lane, mx, se);
    float cs = 0.f;
    for (int c = lane; c < K; c += 64) {
        const float v = calib_sigmoid(x[c], mx, se, a[c], bcal[c]);
        r[c] = v;
        cs += v;
    }
    cs = wave_sum_f(cs);
    unsigned long long cur = 0;   // this lane's largest key not yet selected; 0 = none (a real key's low word is >= 0xFFFFFFFF - K > 0)
    for (int c = lane; c < K; c += 64) {
        const float v = calib_normalise(r[c], cs, K);
        r[c] = v;
        if (proba) proba[(size_t)row * K + c] = v;
        const unsigned long long key = topk_key(v, c);
        cur = key > cur ? key : cur;
    }
    for (int j = 0; j < k; ++j) {   // k <= K (checked by the launcher): a real key is left in every round
        unsigned long long win = cur;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long t = __shfl_xor(win, o);
            win = t > win ? t : win;
        }
        if (lane == 0) {
            idx_out[(size_t)row * k + j] = (int32_t)(0xFFFFFFFFu - (unsigned)win);
            score_out[(size_t)row * k + j] = __uint_as_float((unsigned)(win >> 32));
        }
        if (cur == win) {   // the owner (keys are distinct): its next candidate is its largest key below the winner
            unsigned long long nb = 0;
            for (int c = lane; c < K; c += 64) {
                const unsigned long long key = topk_key(r[c], c);
                nb = (key < win && key > nb) ? key : nb;
            }
            cur = nb;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// mean_topk_kernel: a point is G consecutive rows (its views).  Per class m = (v_0 + v_1 + ... + v_{G-1}) / (float)G, summed left
// to right, v_g = the probability calibrate_kernel writes for row g (same helpers, same lane order of the row sums); then the k
// best classes of m by the rounds of calibrate_topk_kernel.  One wave per point, four points per workgroup; the mean row lives
// where calibrate_topk_kernel keeps its row (wave-private LDS row, or rowbuf [P][K]).  A view takes two passes over its logits
// after the softmax statistics: the row sum of its sigmoids, then sigmoid again -> normalise -> add into the mean row; recomputing
// the sigmoid (same helper, same operands: same bits) is what saves a second scratch row per wave.  G = 1: m = v_0 / 1.0f = v_0,
// the bits of calibrate_topk_kernel.
// ---------------------------------------------------------------------------------------------
template <bool ROW_IN_LDS>
__global__ __launch_bounds__(256) void mean_topk_kernel(const float* __restrict__ logits, int P, int G, int K,
                                                        const float* __restrict__ a, const float* __restrict__ bcal, int k,
                                                        int32_t* __restrict__ idx_out,   // [P][k]
                                                        float* __restrict__ score_out,   // [P][k]
                                                        float* proba,                    // [P][K] or NULL
                                                        float* rowbuf)                   // [P][K] when !ROW_IN_LDS
{
    extern __shared__ float topk_rows[];   // [4][K] when ROW_IN_LDS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pt = blockIdx.x * 4 + wave;
    if (pt >= P) return;
    float* r = ROW_IN_LDS ? topk_rows + (size_t)wave * K : rowbuf + (size_t)pt * K;
    for (int g = 0; g < G; ++g) {
        const float* x = logits + ((size_t)pt * G + g) * K;
        float mx, se;
        calib_softmax_stats(x, K, lane, mx, se);
        float cs = 0.f;
        for (int c = lane; c < K; c += 64) cs += calib_sigmoid(x[c], mx, se, a[c], bcal[c]);
        cs = wave_sum_f(cs);
        for (int c = lane; c < K; c += 64) {
            const float v = calib_normalise(calib_sigmoid(x[c], mx, se, a[c], bcal[c]), cs, K);
            r[c] = g == 0 ? v : r[c] + v;
        }
    }
    const float den = (float)G;
    unsigned long long cur = 0;   // this lane's largest key not yet selected (calibrate_topk_kernel)
    for (int c = lane; c < K; c += 64) {
        const float m = r[c] / den;
        r[c] = m;
        if (proba) proba[(size_t)pt * K + c] = m;
        const unsigned long long key = topk_key(m, c);
        cur = key > cur ? key : cur;
    }
    for (int j = 0; j < k; ++j) {
        unsigned long long win = cur;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long t = __shfl_xor(win, o);
            win = t > win ? t : win;
        }
        if (lane == 0) {
            idx_out[(size_t)pt * k + j] = (int32_t)(0xFFFFFFFFu - (unsigned)win);
            score_out[(size_t)pt * k + j] = __uint_as_float((unsigned)(win >> 32));
        }
        if (cur == win) {
            unsigned long long nb = 0;
            for (int c = lane; c < K; c += 64) {
                const unsigned long long key = topk_key(r[c], c);
                nb = (key < win && key > nb) ? key : nb;
            }
            cur = nb;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// calibrate_eval_kernel: the same calibration, then what a validation pass keeps of a row whose true class g is known
// (mermaid_classifier/pyspacer/trainer.py:271-291, metrics/ranking.py:54-65, metrics/probability.py:47-49):
//   est    = class of the largest topk_key (the first maximum, as numpy.argmax and the stable sort give it), score = v[est]
//   p_true = v[g];   rank = 1 + #{c : topk_key(v[c], c) > topk_key(v[g], g)}: the 1-based place of g in argsort(-v, stable)
// and the totals over the rows: rows seen, correct, unknown (mapped label -1), non-finite, sum of round(-log(clip(p_true, 1e-15,
// 1)) * 2^32), confusion[g][est], rank_hist[rank - 1].  Every total is an integer added with integer atomics, so it depends on
// neither the row order nor the grid nor how the rows are split over launches; the caller zeroes them.
// Rows as in calibrate_topk_kernel (one wave per row, wave-private LDS row or `rowbuf`), but a workgroup walks the rows with the
// grid's stride and keeps its partial totals on chip: the five counters in lane 0's registers, the rank histogram in LDS
// (ROW_IN_LDS), flushed with one atomic per touched destination at the end.  confusion goes straight to memory (one atomic per
// row, spread over the K x K table).  A lane reads only the row entries it wrote; v[g] comes from its owner lane by shuffle.
// y[row] is the caller's label; with label_map it is label_map[y[row]].  A label outside the table or the head is treated as -1.
// scored_out (the grouped pass of metrics.hip reads it) gets g for a row that entered confusion / rank_hist / the loss sum, else -1.
// ---------------------------------------------------------------------------------------------
template <bool ROW_IN_LDS>
__global__ __launch_bounds__(256) void calibrate_eval_kernel(const float* __restrict__ logits, int M, int K,
                                                             const float* __restrict__ a, const float* __restrict__ bcal,
                                                             const int32_t* __restrict__ y, const int32_t* __restrict__ label_map, int n_labels,
                                                             int32_t* __restrict__ est_out, float* __restrict__ score_out,   // [M] or NULL
                                                             int32_t* __restrict__ rank_out, float* __restrict__ ptrue_out,  // [M] or NULL
                                                             unsigned long long* __restrict__ totals,      // [EVAL_TOTALS]
                                                             unsigned long long* __restrict__ confusion,   // [K][K] or NULL
                                                             unsigned long long* __restrict__ rank_hist,   // [K] or NULL
                                                             int32_t* __restrict__ scored_out,             // [M] or NULL
                                                             float* rowbuf)                                // [M][K] when !ROW_IN_LDS
{
    extern __shared__ float eval_lds[];   // ROW_IN_LDS: [4][K] rows, then [K] unsigned rank counts
    __shared__ unsigned long long red[4][EVAL_TOTALS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned* hist = reinterpret_cast<unsigned*>(eval_lds + (size_t)4 * K);
    if (ROW_IN_LDS) {
        for (int c = threadIdx.x; c < K; c += 256) hist[c] = 0;
        __syncthreads();
    }
    unsigned long long tot[EVAL_TOTALS] = {0, 0, 0, 0, 0};   // lane 0's are the wave's
    for (int row = blockIdx.x * 4 + wave; row < M; row += gridDim.x * 4) {
        const float* x = logits + (size_t)row * K;
        float* r = ROW_IN_LDS ? eval_lds + (size_t)wave * K : rowbuf + (size_t)row * K;
        float mx, se;
        calib_softmax_stats(x, K, lane, mx, se);
        float cs = 0.f;
        for (int c = lane; c < K; c += 64) {
            const float v = calib_sigmoid(x[c], mx, se, a[c], bcal[c]);
            r[c] = v;
            cs += v;
        }
        cs = wave_sum_f(cs);
        unsigned long long best = 0;
        bool bad = false;
        for (int c = lane; c < K; c += 64) {
            const float v = calib_normalise(r[c], cs, K);
            r[c] = v;
            bad |= !(fabsf(v) <= 3.402823466e+38f);   // NaN or infinite
            const unsigned long long key = topk_key(v, c);
            best = key > best ? key : best;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long t = __shfl_xor(best, o);
            best = t > best ? t : best;
        }
        bad = __ballot(bad) != 0;
        const int est = (int)(0xFFFFFFFFu - (unsigned)best);
        int g = y[row];
        if (label_map) g = (g >= 0 && g < n_labels) ? label_map[g] : -1;
        if (g < 0 || g >= K) g = -1;
        int rank = 0;
        float pt = 0.f;
        if (g >= 0) {   // (wave-uniform)
            const int owner = g & 63;
            pt = __shfl(lane == owner ? r[g] : 0.f, owner);
            const unsigned long long keyg = topk_key(pt, g);
            int above = 0;
            for (int c = lane; c < K; c += 64) above += topk_key(r[c], c) > keyg;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o);
            rank = 1 + above;
        }
        if (lane == 0) {
            if (est_out) est_out[row] = est;
            if (score_out) score_out[row] = __uint_as_float((unsigned)(best >> 32));
            if (rank_out) rank_out[row] = rank;
            if (ptrue_out) ptrue_out[row] = pt;
            if (scored_out) scored_out[row] = (g >= 0 && !bad) ? g : -1;
            tot[0] += 1;
            if (g < 0) tot[2] += 1;
            else if (bad) tot[3] += 1;
            else {
                tot[1] += est == g;
                tot[4] += (unsigned long long)llrint(-log(fmin(fmax((double)pt, 1e-15), 1.0)) * 4294967296.0);
                if (confusion) atomicAdd(&confusion[(size_t)g * K + est], 1ull);
                if (rank_hist) {
                    if (ROW_IN_LDS) atomicAdd(&hist[rank - 1], 1u);
                    else atomicAdd(&rank_hist[rank - 1], 1ull);
                }
            }
        }
    }
    if (lane == 0)
        for (int i = 0; i < EVAL_TOTALS; ++i) red[wave][i] = tot[i];
    __syncthreads();
    if (threadIdx.x < EVAL_TOTALS) {
        const unsigned long long s = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        if (s) atomicAdd(&totals[threadIdx.x], s);
    }
    if (ROW_IN_LDS && rank_hist)
        for (int c = threadIdx.x; c < K; c += 256)
            if (hist[c]) atomicAdd(&rank_hist[c], (unsigned long long)hist[c]);
}

// ---------------------------------------------------------------------------------------------
// Head ensembles (include/mmc.h, "head ensembles"): M members' logits for the same rows lie in one [M][rows][K] buffer.  A point is G
// consecutive rows.  Per class: v_{j,g} = the probability calibrate_kernel writes for member j's row g (same helpers, same lane
// order of the row sums), m_j = (v_{j,0} + ... + v_{j,G-1}) / (float)G as mean_topk_kernel forms it, and
// e = (m_0 + ... + m_{M-1}) / (float)M, both summed left to right in fp32.  M = 1: e = m_0 / 1.0f, the bits of mean_topk_kernel.
// ensemble_row makes e for one point in a wave: two wave-private LDS rows, mrow for the member's mean and erow for the ensemble's;
// a lane reads only entries it wrote (classes lane, lane + 64, ...), so there is no barrier.  It also returns the two entropies
// H(e) and (1/M) sum_j H(m_j), H(p) = -sum_c p_c log p_c with a zero class adding 0: each lane adds its classes' terms in
// double, a fixed xor butterfly folds the lanes, the members' sums are added in member order -- no atomics, so the bits depend on
// the logits, M, G and K alone -- and lane j keeps member j's best class (largest topk_key of m_j: the first maximum) for the votes.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_d(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double entropy_term(float p) { return p == 0.f ? 0.0 : -(double)p * log((double)p); }

__device__ __forceinline__ void ensemble_row(const float* __restrict__ logits, size_t mstride, size_t row0, int Mn, int G, int K,
                                             const EnsembleCal& cal, int lane, float* mrow, float* erow, bool want_stats, double& h_e,
                                             double& h_m, int& member_best)
{
    const float den = (float)G;
    h_m = 0.0;
    member_best = -1;
    for (int j = 0; j < Mn; ++j) {
        const float* __restrict__ a = cal.a[j];
        const float* __restrict__ bcal = cal.b[j];
        for (int g = 0; g < G; ++g) {
            const float* x = logits + (size_t)j * mstride + (row0 + g) * K;
            float mx, se;
            calib_softmax_stats(x, K, lane, mx, se);
            float cs = 0.f;
            for (int c = lane; c < K; c += 64) cs += calib_sigmoid(x[c], mx, se, a[c], bcal[c]);
            cs = wave_sum_f(cs);
            for (int c = lane; c < K; c += 64) {
                const float v = calib_normalise(calib_sigmoid(x[c], mx, se, a[c], bcal[c]), cs, K);
                mrow[c] = g == 0 ? v : mrow[c] + v;
            }
        }
        unsigned long long best = 0;
        double h = 0.0;
        for (int c = lane; c < K; c += 64) {
            const float m = mrow[c] / den;
            erow[c] = j == 0 ? m : erow[c] + m;
            const unsigned long long key = topk_key(m, c);
            best = key > best ? key : best;
            if (want_stats) h += entropy_term(m);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long t = __shfl_xor(best, o);
            best = t > best ? t : best;
        }
        if (lane == j) member_best = (int)(0xFFFFFFFFu - (unsigned)best);
        if (want_stats) h_m += wave_sum_d(h);
    }
    const float dm = (float)Mn;
    double h = 0.0;
    for (int c = lane; c < K; c += 64) {
        const float e = erow[c] / dm;
        erow[c] = e;
        if (want_stats) h += entropy_term(e);
    }
    h_e = want_stats ? wave_sum_d(h) : 0.0;
    h_m /= (double)Mn;
}
// what a point keeps of them (lane 0 writes): H(e), the members' mean entropy, their difference -- the mutual information between
// prediction and member, stored as computed (rounding can leave it a hair below 0) -- each rounded to fp32 once; and the votes:
// the members whose own best class is the ensemble's
__device__ __forceinline__ void ensemble_write_stats(float* __restrict__ stats, int32_t* __restrict__ votes, size_t pt, int lane, int Mn,
                                                     double h_e, double h_m, int member_best, int best_class)
{
    const unsigned long long agree = __ballot(lane < Mn && member_best == best_class);
    if (lane != 0) return;
    if (stats) {
        stats[pt * ENSEMBLE_STATS + 0] = (float)h_e;
        stats[pt * ENSEMBLE_STATS + 1] = (float)h_m;
        stats[pt * ENSEMBLE_STATS + 2] = (float)(h_e - h_m);
    }
    if (votes) votes[pt] = __popcll(agree);
}

// ensemble_topk_kernel: e of a point, then its k best classes by the rounds of calibrate_topk_kernel.  One wave per point, four
// points per workgroup, LDS [4][2][K] floats (K <= TOPK_LDS_MAX_K: 64 KB at the limit).  Nothing rows x K is written unless the
// caller wants the means (proba).
__global__ __launch_bounds__(256) void ensemble_topk_kernel(const float* __restrict__ logits, int P, int G, int K, int Mn, size_t mstride,
                                                            EnsembleCal cal, int k,
                                                            int32_t* __restrict__ idx_out,   // [P][k]
                                                            float* __restrict__ score_out,   // [P][k]
                                                            float* __restrict__ proba,       // [P][K] or NULL
                                                            float* __restrict__ stats,       // [P][ENSEMBLE_STATS] or NULL
                                                            int32_t* __restrict__ votes)     // [P] or NULL
{
    extern __shared__ float ens_rows[];   // [4][2][K]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pt = blockIdx.x * 4 + wave;
    if (pt >= P) return;
    float* mrow = ens_rows + (size_t)wave * 2 * K;
    float* r = mrow + K;
    double h_e, h_m;
    int member_best;
    ensemble_row(logits, mstride, (size_t)pt * G, Mn, G, K, cal, lane, mrow, r, stats != nullptr, h_e, h_m, member_best);
    unsigned long long cur = 0;   // this lane's largest key not yet selected (calibrate_topk_kernel)
    for (int c = lane; c < K; c += 64) {
        const float e = r[c];
        if (proba) proba[(size_t)pt * K + c] = e;
        const unsigned long long key = topk_key(e, c);
        cur = key > cur ? key : cur;
    }
    int best_class = 0;
    for (int j = 0; j < k; ++j) {
        unsigned long long win = cur;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long t = __shfl_xor(win, o);
            win = t > win ? t : win;
        }
        if (j == 0) best_class = (int)(0xFFFFFFFFu - (unsigned)win);
        if (lane == 0) {
            idx_out[(size_t)pt * k + j] = (int32_t)(0xFFFFFFFFu - (unsigned)win);
            score_out[(size_t)pt * k + j] = __uint_as_float((unsigned)(win >> 32));
        }
        if (cur == win) {
            unsigned long long nb = 0;
            for (int c = lane; c < K; c += 64) {
                const unsigned long long key = topk_key(r[c], c);
                nb = (key < win && key > nb) ? key : nb;
            }
            cur = nb;
        }
    }
    ensemble_write_stats(stats, votes, (size_t)pt, lane, Mn, h_e, h_m, member_best, best_class);
}

// ensemble_eval_kernel: e of a row (G = 1), then what calibrate_eval_kernel keeps of it -- est, score, rank, p_true, the five
// totals, confusion, rank_hist, by the same rules for the label map, unknown and non-finite rows and with the same integer atomics,
// so the tables depend on neither the grid nor the chunking -- plus the row's entropies and votes.  LDS: [4][2][K] rows, then [K]
// unsigned rank counts when hist_lds (the launcher sets it while both fit in 64 KB; otherwise rank_hist takes one atomic per row).
__global__ __launch_bounds__(256) void ensemble_eval_kernel(const float* __restrict__ logits, int M, int K, int Mn, size_t mstride,
                                                            EnsembleCal cal, const int32_t* __restrict__ y,
                                                            const int32_t* __restrict__ label_map, int n_labels,
                                                            int32_t* __restrict__ est_out, float* __restrict__ score_out,   // [M] or NULL
                                                            int32_t* __restrict__ rank_out, float* __restrict__ ptrue_out,  // [M] or NULL
                                                            float* __restrict__ stats,                    // [M][ENSEMBLE_STATS] or NULL
                                                            int32_t* __restrict__ votes,                  // [M] or NULL
                                                            unsigned long long* __restrict__ totals,      // [EVAL_TOTALS]
                                                            unsigned long long* __restrict__ confusion,   // [K][K] or NULL
                                                            unsigned long long* __restrict__ rank_hist,   // [K] or NULL
                                                            int hist_lds)
{
    extern __shared__ float ens_eval_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned* hist = reinterpret_cast<unsigned*>(ens_eval_lds + (size_t)8 * K);
    if (hist_lds) {
        for (int c = threadIdx.x; c < K; c += 256) hist[c] = 0;
        __syncthreads();
    }
    float* mrow = ens_eval_lds + (size_t)wave * 2 * K;
    float* r = mrow + K;
    unsigned long long tot[EVAL_TOTALS] = {0, 0, 0, 0, 0};   // lane 0's are the wave's
    for (int row = blockIdx.x * 4 + wave; row < M; row += gridDim.x * 4) {
        double h_e, h_m;
        int member_best;
        ensemble_row(logits, mstride, (size_t)row, Mn, 1, K, cal, lane, mrow, r, stats != nullptr, h_e, h_m, member_best);
        unsigned long long best = 0;
        bool bad = false;
        for (int c = lane; c < K; c += 64) {
            const float v = r[c];
            bad |= !(fabsf(v) <= 3.402823466e+38f);   // NaN or infinite
            const unsigned long long key = topk_key(v, c);
            best = key > best ? key : best;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long t = __shfl_xor(best, o);
            best = t > best ? t : best;
        }
        bad = __ballot(bad) != 0;
        const int est = (int)(0xFFFFFFFFu - (unsigned)best);
        ensemble_write_stats(stats, votes, (size_t)row, lane, Mn, h_e, h_m, member_best, est);
        int g = y[row];
        if (label_map) g = (g >= 0 && g < n_labels) ? label_map[g] : -1;
        if (g < 0 || g >= K) g = -1;
        int rank = 0;
        float pt = 0.f;
        if (g >= 0) {   // (wave-uniform)
            const int owner = g & 63;
            pt = __shfl(lane == owner ? r[g] : 0.f, owner);
            const unsigned long long keyg = topk_key(pt, g);
            int above = 0;
            for (int c = lane; c < K; c += 64) above += topk_key(r[c], c) > keyg;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o);
            rank = 1 + above;
        }
        if (lane == 0) {
            if (est_out) est_out[row] = est;
            if (score_out) score_out[row] = __uint_as_float((unsigned)(best >> 32));
            if (rank_out) rank_out[row] = rank;
            if (ptrue_out) ptrue_out[row] = pt;
            tot[0] += 1;
            if (g < 0) tot[2] += 1;
            else if (bad) tot[3] += 1;
            else {
                tot[1] += est == g;
                tot[4] += (unsigned long long)llrint(-log(fmin(fmax((double)pt, 1e-15), 1.0)) * 4294967296.0);
                if (confusion) atomicAdd(&confusion[(size_t)g * K + est], 1ull);
                if (rank_hist) {
                    if (hist_lds) atomicAdd(&hist[rank - 1], 1u);
                    else atomicAdd(&rank_hist[rank - 1], 1ull);
                }
            }
        }
    }
    if (lane == 0)   // one atomic per wave and touched total (no static LDS: at K = 2048 the rows alone are the 64 KB)
        for (int i = 0; i < EVAL_TOTALS; ++i)
            if (tot[i]) atomicAdd(&totals[i], tot[i]);
    __syncthreads();
    if (hist_lds && rank_hist)
        for (int c = threadIdx.x; c < K; c += 256)
            if (hist[c]) atomicAdd(&rank_hist[c], (unsigned long long)hist[c]);
}

// ---------------------------------------------------------------------------------------------
// rank_rows_kernel: the ranking tables of a validation pass (mermaid_classifier/pyspacer/metrics/ranking.py:88-128, :163-209).  It
// runs behind calibrate_eval_kernel on the same chunk of logits and reads that kernel's per-row `scored` (the true class g of a row
// that entered confusion / rank_hist, else -1) and `rank`.  An unscored row does nothing.  For a scored row:
//   class_rank_hist[g][rank - 1] += 1                      the rank histogram of calibrate_eval_kernel, broken down by true class
//   hier_hist[j][m_j] += 1 for j = 0 .. kmax - 1           c_0, c_1, ... are the row's classes in the order of calibrate_topk_kernel
//                                                          (score descending, equal scores in class order) and m_j is the largest
//                                                          sim_level[g][c_i] over i <= j: the running maximum of ranking.py:184
// The calibration and the selection rounds are those of calibrate_topk_kernel, helper for helper, so c_j is the class mmc_head_topk
// names.  Without sim_level only the first table is made and no row is calibrated.
// Rows as in calibrate_eval_kernel (one wave per row, wave-private LDS row or `rowbuf`, the grid's stride).  hier_hist is kept as
// 32-bit counters in LDS behind the rows (a chunk holds fewer than 2^32 rows) and flushed with one 64-bit atomic per non-zero cell;
// class_rank_hist goes straight to memory, one atomic per row spread over the K x K table.  Integer atomics only: the tables depend
// on neither the row order nor the grid nor the chunking; the caller zeroes them.
// ---------------------------------------------------------------------------------------------
template <bool ROW_IN_LDS>
__global__ __launch_bounds__(256) void rank_rows_kernel(const float* __restrict__ logits, int M, int K,
                                                        const float* __restrict__ a, const float* __restrict__ bcal,
                                                        const int32_t* __restrict__ scored, const int32_t* __restrict__ rank,   // [M]
                                                        const uint8_t* __restrict__ sim_level,             // [K][K] or NULL
                                                        int n_levels, int kmax,
                                                        unsigned long long* __restrict__ class_rank_hist,  // [K][K] or NULL
                                                        unsigned long long* __restrict__ hier_hist,        // [kmax][n_levels] or NULL
                                                        float* rowbuf)                                     // [M][K] when !ROW_IN_LDS
{
    extern __shared__ float rank_lds[];   // [4][K] rows when ROW_IN_LDS, then [kmax][n_levels] unsigned counts
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned* hh = reinterpret_cast<unsigned*>(rank_lds + (ROW_IN_LDS ? (size_t)4 * K : 0));
    const int cells = sim_level ? kmax * n_levels : 0;
    for (int i = threadIdx.x; i < cells; i += 256) hh[i] = 0;
    __syncthreads();
    for (int row = blockIdx.x * 4 + wave; row < M; row += gridDim.x * 4) {
        const int g = scored[row];
        if (g < 0) continue;   // (wave-uniform)
        if (class_rank_hist && lane == 0) atomicAdd(&class_rank_hist[(size_t)g * K + (rank[row] - 1)], 1ull);
        if (!sim_level) continue;
        const float* x = logits + (size_t)row * K;
        float* r = ROW_IN_LDS ? rank_lds + (size_t)wave * K : rowbuf + (size_t)row * K;
        float mx, se;
        calib_softmax_stats(x, K, lane, mx, se);
        float cs = 0.f;
        for (int c = lane; c < K; c += 64) {
            const float v = calib_sigmoid(x[c], mx, se, a[c], bcal[c]);
            r[c] = v;
            cs += v;
        }
        cs = wave_sum_f(cs);
        unsigned long long cur = 0;   // this lane's largest key not yet selected (calibrate_topk_kernel)
        for (int c = lane; c < K; c += 64) {
            const float v = calib_normalise(r[c], cs, K);
            r[c] = v;
            const unsigned long long key = topk_key(v, c);
            cur = key > cur ? key : cur;
        }
        const uint8_t* lv = sim_level + (size_t)g * K;
        unsigned m = 0;   // lane 0's: the running maximum level
        for (int j = 0; j < kmax; ++j) {   // kmax <= K (checked by the launcher): a real key is left in every round
            unsigned long long win = cur;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long t = __shfl_xor(win, o);
                win = t > win ? t : win;
            }
            if (lane == 0) {
                const unsigned l = lv[0xFFFFFFFFu - (unsigned)win];
                m = l > m ? l : m;
                atomicAdd(&hh[j * n_levels + m], 1u);
            }
            if (cur == win) {   // the owner: its largest key below the winner
                unsigned long long nb = 0;
                for (int c = lane; c < K; c += 64) {
                    const unsigned long long key = topk_key(r[c], c);
                    nb = (key < win && key > nb) ? key : nb;
                }
                cur = nb;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += 256)
        if (hh[i]) atomicAdd(&hier_hist[i], (unsigned long long)hh[i]);
}

// ---------------------------------------------------------------------------------------------
// crop_patches: reflect-pad + slice as pure index arithmetic on the resident image.
// numpy 'reflect': index i<0 -> -i ; i>=n -> 2(n-1)-i.  One thread = 4 output pixels (12 bytes).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void crop_kernel(const uint8_t* __restrict__ image, int H, int W,
                                                   const int32_t* __restrict__ rowcols, uint8_t* __restrict__ out)
{
    const int p = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;  // over 224*56 groups of 4 pixels
    if (idx >= 224 * 56) return;
    const int y = idx / 56, xg = idx - y * 56;
    // device-resident points have not been seen by the host: clamp them into the image so that a bad point can never
    // turn into an out-of-bounds read (the host-points path rejects such points with MMC_ERR_ARG before launching)
    int row = rowcols[2 * p], col = rowcols[2 * p + 1];
    row = row < 0 ? 0 : (row >= H ? H - 1 : row);
    col = col < 0 ? 0 : (col >= W ? W - 1 : col);
    int sy = row - 112 + y;
    sy = sy < 0 ? -sy : sy;
    sy = sy >= H ? 2 * (H - 1) - sy : sy;
    uint32_t w[3] = {0, 0, 0};
    uint8_t* wb = reinterpret_cast<uint8_t*>(w);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int sx = col - 112 + xg * 4 + e;
        sx = sx < 0 ? -sx : sx;
        sx = sx >= W ? 2 * (W - 1) - sx : sx;
        const uint8_t* src = image + ((size_t)sy * W + sx) * 3;
        wb[3 * e + 0] = src[0];
        wb[3 * e + 1] = src[1];
        wb[3 * e + 2] = src[2];
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(out + ((size_t)p * 224 * 224 + (size_t)y * 224 + xg * 4) * 3);
    dst[0] = w[0];
    dst[1] = w[1];
    dst[2] = w[2];
}

// ---------------------------------------------------------------------------------------------
// crop_views_kernel: patch p = view views[p] of point p (include/mmc.h, "patch views"), on crop_kernel's scheme: one thread =
// 4 consecutive output pixels, one 12-byte store.  view_source() says where an output pixel lies in the base patch; the base patch
// is crop_kernel's window (z = 0) or the rounded mean of the 2x2 footprint in the 448-pixel window (z = 1), both reflected once
// (H, W > 224 bound every index: a window reaches at most 224 pixels past an edge).  For odd r the four pixels of a thread come
// from four source rows; the image lines a workgroup touches are shared with its neighbours through the caches.
// The view is uniform per workgroup (blockIdx.y = patch), so the branches below do not diverge.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect1(int i, int n)
{
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}
__global__ __launch_bounds__(256) void crop_views_kernel(const uint8_t* __restrict__ image, int H, int W,
                                                         const int32_t* __restrict__ rowcols, const uint8_t* __restrict__ views,
                                                         uint8_t* __restrict__ out)
{
    const int p = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;  // over 224*56 groups of 4 pixels
    if (idx >= 224 * 56) return;
    const int i = idx / 56, jg = idx - i * 56;
    const int v = views ? (views[p] & 15) : 0;       // device codes are masked, as device points are clamped
    int row = rowcols[2 * p], col = rowcols[2 * p + 1];
    row = row < 0 ? 0 : (row >= H ? H - 1 : row);
    col = col < 0 ? 0 : (col >= W ? W - 1 : col);
    uint32_t w[3] = {0, 0, 0};
    uint8_t* wb = reinterpret_cast<uint8_t*>(w);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int by, bx;
        view_source(v, i, jg * 4 + e, by, bx);
        if (!(v & 8)) {
            const uint8_t* src = image + ((size_t)reflect1(row - 112 + by, H) * W + reflect1(col - 112 + bx, W)) * 3;
            wb[3 * e + 0] = src[0];
            wb[3 * e + 1] = src[1];
            wb[3 * e + 2] = src[2];
        } else {
            const size_t y0 = (size_t)reflect1(row - 224 + 2 * by, H) * W, y1 = (size_t)reflect1(row - 223 + 2 * by, H) * W;
            const int x0 = reflect1(col - 224 + 2 * bx, W), x1 = reflect1(col - 223 + 2 * bx, W);
            const uint8_t *s00 = image + (y0 + x0) * 3, *s01 = image + (y0 + x1) * 3;
            const uint8_t *s10 = image + (y1 + x0) * 3, *s11 = image + (y1 + x1) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) wb[3 * e + c] = (uint8_t)(((int)s00[c] + s01[c] + s10[c] + s11[c] + 2) >> 2);
        }
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(out + ((size_t)p * 224 * 224 + (size_t)i * 224 + jg * 4) * 3);
    dst[0] = w[0];
    dst[1] = w[1];
    dst[2] = w[2];
}

// =============================================================================================
// Host-side launchers (plain C++ signatures declared in kernels.h)
// =============================================================================================
int launch_stem(const uint8_t* patches, const _Float16* w, const float* bias, const float* padval, _Float16* out, int B,
                int channels, hipStream_t st)
{
    dim3 grid(7, 7, B);
    if (channels == 32) hipLaunchKernelGGL(stem_conv_kernel<2>, grid, dim3(256), 0, st, patches, w, bias, padval, out);
    else if (channels == 48) hipLaunchKernelGGL(stem_conv_kernel<3>, grid, dim3(256), 0, st, patches, w, bias, padval, out);
    else return -13;
    LAUNCH_CHECK();
    return 0;
}

template <int MT, int NT, int EPI, bool GATE, bool RES, bool DG>
static int launch_gemm_t(const GemmArgs& a, hipStream_t st)
{
    constexpr int UK = MT * NT <= 4 ? 4 : 2;   // k-steps per LDS batch, bounded by registers
    static_assert(!DG || (GATE && MT == 1 && UK == 4), "the deferred gate exists for gated one-fragment forms only");
    // EPI_GAP: one workgroup per patch (its HW <= 64 rows) and chunk
    const dim3 grid(EPI == EPI_GAP ? a.M / a.HW : (a.M + 64 * MT - 1) / (64 * MT), a.n_chunks, 1);
    hipLaunchKernelGGL((pw_gemm_kernel<MT, NT, EPI, GATE, RES, UK, DG>), grid, dim3(256), 0, st, a.X, a.M, a.K, a.Wp, a.Kp / 32,
                       a.bias, a.Y, a.N, a.gate, a.HW, a.res, a.gap_out, a.inv_hw);
    LAUNCH_CHECK();
    return 0;
}

// pw_gemm_kernel's instantiations.  Key: MT, NT, EPI, GATE, RES, DG (deferred gate: 7x7 project layers).  The chunk widths
// are what pick_nt (mmc_api.cpp) gives the layers of B0 and B4: an expand conv (SiLU, never gated) has 3, 5, 6, 7 or 8
// fragments per chunk, a project conv (linear, always gated, with or without skip) 1 to 4, the head (GAP) is packed with 4.
static_assert(EPI_SILU == 0 && EPI_LINEAR == 1 && EPI_GAP == 2, "the labels below spell the epilogues as numbers");
#define G(MT, NT, EPI, GATE, RES, DG) \
    {{MT, NT, EPI, GATE, RES, DG}, "pw_gemm<" #MT "," #NT "," #EPI "," #GATE "," #RES ">", launch_gemm_t<MT, NT, EPI, GATE != 0, RES != 0, DG != 0>},
#define EXPAND(NT) G(1, NT, 0, 0, 0, 0) G(2, NT, 0, 0, 0, 0)
#define PROJECT(NT, RES) G(1, NT, 1, 1, RES, 0) G(1, NT, 1, 1, RES, 1) G(2, NT, 1, 1, RES, 0)
static const Inst<6, GemmArgs> PW_GEMM_TABLE[] = {
    EXPAND(3) EXPAND(5) EXPAND(6) EXPAND(7) EXPAND(8)
    PROJECT(1, 0) PROJECT(2, 0) PROJECT(3, 0) PROJECT(4, 0)
    PROJECT(1, 1) PROJECT(2, 1) PROJECT(3, 1) PROJECT(4, 1)
    G(1, 4, 2, 0, 0, 0)
};
#undef PROJECT
#undef EXPAND
#undef G

// the gate is deferred where the form allows it: one row fragment per wave, four k-steps per LDS batch
static int gemm_dg(int mt, int nt, bool gate, int defer_gate) { return (defer_gate && gate && mt == 1 && nt <= 4) ? 1 : 0; }

const char* pw_gemm_label(int mt, int nt, int epi, int gate, int res, int defer_gate)
{
    if (epi == EPI_GAP) mt = 1;   // one form, whatever the batch
    return inst_label(PW_GEMM_TABLE, {mt, nt, epi, gate, res, gemm_dg(mt, nt, gate != 0, defer_gate)});
}

int launch_pw_gemm(const GemmArgs& a, hipStream_t st)
{
    if (a.epi == EPI_GAP && a.HW > 64) return -2;
    const int mt = (a.mt == 2 && a.epi != EPI_GAP) ? 2 : 1;
    return inst_launch(PW_GEMM_TABLE, {mt, a.nt, a.epi, a.gate ? 1 : 0, a.res ? 1 : 0, gemm_dg(mt, a.nt, a.gate, a.defer_gate)}, a, st, -3);
}

int launch_pw_gemm_fp8(const Fp8GemmArgs& a, hipStream_t st)
{
    if (a.M < 1 || (a.K & 7) || (a.N & 3) || a.KS128 * 128 < a.K || a.NFp % 7 || 16 * a.NFp < a.N || !a.gate || a.HW < 1) return -17;
    dim3 grid((a.M + 63) / 64, a.NFp / 7);
    if (a.res) hipLaunchKernelGGL((pw_gemm_fp8_kernel<7, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((pw_gemm_fp8_kernel<7, false>), grid, dim3(256), 0, st, a);
    LAUNCH_CHECK();
    return 0;
}

template <int KS, int ST, int TW>
static int launch_dw_t(const DwArgs& a, hipStream_t st)
{
    const int nz = a.nz > 0 ? a.nz : 1;
    if (a.CG * nz * 8 != a.C || a.CG * a.S > 256 || a.CG * a.S < 1) return -14;
    dim3 grid(a.parts, a.B, nz);
    dim3 block(a.CG * a.S);
    const size_t shm = (size_t)a.S * a.CG * 8 * sizeof(float);
    hipLaunchKernelGGL((dwconv_kernel<KS, ST, TW>), grid, block, shm, st, a.in, a.wt, a.bias, a.out, a.pool_part, a.H,
                       a.W, a.C, a.Ho, a.Wo, a.pad_t, a.pad_l, a.CG, a.S, a.iters);
    LAUNCH_CHECK();
    return 0;
}

// dwconv_kernel's instantiations.  Key: kernel size, stride, outputs per thread along x (4 where Ho divides by 4, 7 at 7x7,
// else 2: no stride-2 3x3 layer lands on 7x7 and no stride-2 5x5 layer on 14x14)
#define DW(KS, ST, TW) {{KS, ST, TW}, "dwconv<" #KS "," #ST "," #TW ">", launch_dw_t<KS, ST, TW>},
static const Inst<3, DwArgs> DWCONV_TABLE[] = {
    DW(3, 1, 4) DW(3, 1, 2) DW(3, 1, 7) DW(3, 2, 4) DW(3, 2, 2)
    DW(5, 1, 4) DW(5, 1, 2) DW(5, 1, 7) DW(5, 2, 4) DW(5, 2, 7)
};
#undef DW

const char* dwconv_label(int ks, int stride, int tw) { return inst_label(DWCONV_TABLE, {ks, stride, tw}); }
int launch_dwconv(const DwArgs& a, hipStream_t st) { return inst_launch(DWCONV_TABLE, {a.ks, a.stride, a.tw}, a, st, -4); }

int launch_se_small(const float* pool_part, int nparts, int B, int C, int Cs, const float* wr, const float* br,
                    const float* we, const float* be, float* gate, hipStream_t st)
{
    if (C > 256 || Cs > 16 || B < 1) return -12;
    hipLaunchKernelGGL(se_small_kernel, dim3(B), dim3(256), 0, st, pool_part, nparts, C, Cs, wr, br, we, be, gate);
    LAUNCH_CHECK();
    return 0;
}

int launch_se_wide(const float* pool_part, int nparts, int B, int C, int Cs, const float* wr, const float* br,
                   const float* we_t, const float* be, float* gate, hipStream_t st)
{
    if (B < 1 || C < 1 || C > 3072 || Cs < 1 || (size_t)(C + Cs) * 4 > 64000) return -12;   // (3072: three channels per thread in the excite FC)
    hipLaunchKernelGGL(se_wide_kernel, dim3(B), dim3(1024), (size_t)(C + Cs) * sizeof(float), st, pool_part, nparts, C, Cs, wr, br, we_t, be, gate);
    LAUNCH_CHECK();
    return 0;
}

int launch_se_gate(const float* pool_part, int nparts, int B, int C, int Cs4, const float* WrP, const float* br,
                   const float* WeP, const float* be, float* gate, hipStream_t st)
{
    if (C > 16 * SE_MAXG * 16 || Cs4 > 48 || (C & 15)) return -6;
    const int ng = C / 16;
    int nsplit = (ng + 16 * SE_MAXT - 1) / (16 * SE_MAXT);   // each y-slice covers <= 16 waves * SE_MAXT fragments
    if (ng >= 30 && nsplit < 4) nsplit = 4;                  // big layers: spread the weight stream over 4 CUs
    const dim3 grid((B + 15) / 16, nsplit);
    const int maxg = (ng + 15) / 16;                         // FC1 k-groups per wave
#define SE_LAUNCH(G) hipLaunchKernelGGL((se_fused_kernel<G>), grid, dim3(1024), 0, st, pool_part, nparts, B, C, Cs4, WrP, br, WeP, be, gate)
    if (maxg <= 1) SE_LAUNCH(1);
    else if (maxg <= 2) SE_LAUNCH(2);
    else if (maxg <= 3) SE_LAUNCH(3);
    else SE_LAUNCH(SE_MAXG);
#undef SE_LAUNCH
    LAUNCH_CHECK();
    return 0;
}

int launch_mlp_layer(const float* X, int M, int K, const float* W, const float* bias, float* Y, int N, bool relu,
                     hipStream_t st)
{
    constexpr int NT = 4;
    dim3 grid((M + 63) / 64, (N + 16 * NT - 1) / (16 * NT), 1);
    if (relu)
        hipLaunchKernelGGL((mlp_gemm_f32_kernel<NT, true>), grid, dim3(256), 0, st, X, M, K, W, bias, Y, N);
    else
        hipLaunchKernelGGL((mlp_gemm_f32_kernel<NT, false>), grid, dim3(256), 0, st, X, M, K, W, bias, Y, N);
    LAUNCH_CHECK();
    return 0;
}

int launch_calibrate(const float* logits, int M, int K, const float* a, const float* b, float* proba, int32_t* argmax,
                     hipStream_t st)
{
    hipLaunchKernelGGL(calibrate_kernel, dim3((M + 3) / 4), dim3(256), 0, st, logits, M, K, a, b, proba, argmax);
    LAUNCH_CHECK();
    return 0;
}

int launch_calibrate_topk(const float* logits, int M, int K, const float* a, const float* b, int k, int32_t* idx, float* scores,
                          float* proba, float* rowbuf, hipStream_t st)
{
    if (M < 1 || K < 1 || k < 1 || k > K || !idx || !scores) return -18;
    const dim3 grid((M + 3) / 4);
    if (K <= TOPK_LDS_MAX_K) {
        hipLaunchKernelGGL((calibrate_topk_kernel<true>), grid, dim3(256), (size_t)4 * K * sizeof(float), st, logits, M, K, a, b, k,
                           idx, scores, proba, (float*)nullptr);
    } else {
        // the row lives in global memory: in the probability output when the caller wants one, else in the scratch rows
        float* rows = proba ? proba : rowbuf;
        if (!rows) return -18;
        hipLaunchKernelGGL((calibrate_topk_kernel<false>), grid, dim3(256), 0, st, logits, M, K, a, b, k, idx, scores,
                           (float*)nullptr, rows);
    }
    LAUNCH_CHECK();
    return 0;
}

int launch_mean_topk(const float* logits, int P, int G, int K, const float* a, const float* b, int k, int32_t* idx, float* scores,
                     float* proba, float* rowbuf, hipStream_t st)
{
    if (P < 1 || G < 1 || G > VIEWS_MAX || K < 1 || k < 1 || k > K || !idx || !scores) return -18;
    const dim3 grid((P + 3) / 4);
    if (K <= TOPK_LDS_MAX_K) {
        hipLaunchKernelGGL((mean_topk_kernel<true>), grid, dim3(256), (size_t)4 * K * sizeof(float), st, logits, P, G, K, a, b, k, idx,
                           scores, proba, (float*)nullptr);
    } else {
        float* rows = proba ? proba : rowbuf;   // as launch_calibrate_topk: the mean row lives in the output when there is one
        if (!rows) return -18;
        hipLaunchKernelGGL((mean_topk_kernel<false>), grid, dim3(256), 0, st, logits, P, G, K, a, b, k, idx, scores, (float*)nullptr,
                           rows);
    }
    LAUNCH_CHECK();
    return 0;
}

int launch_calibrate_eval(const float* logits, int M, int K, const float* a, const float* b, const int32_t* y, const int32_t* label_map,
                          int n_labels, int32_t* est, float* score, int32_t* rank, float* p_true, long long* totals, long long* confusion,
                          long long* rank_hist, int32_t* scored, float* rowbuf, hipStream_t st)
{
    if (M < 1 || K < 1 || !y || !totals || (label_map && n_labels < 1)) return -18;
    // a workgroup keeps its partial totals on chip while it walks rows: enough workgroups to fill the chip, no more
    const int nb = (M + 3) / 4;
    const dim3 grid(nb < 2048 ? nb : 2048);
    unsigned long long* t = reinterpret_cast<unsigned long long*>(totals);
    unsigned long long* cf = reinterpret_cast<unsigned long long*>(confusion);
    unsigned long long* rh = reinterpret_cast<unsigned long long*>(rank_hist);
    if (K <= TOPK_LDS_MAX_K) {
        hipLaunchKernelGGL((calibrate_eval_kernel<true>), grid, dim3(256), (size_t)5 * K * sizeof(float), st, logits, M, K, a, b, y, label_map,
                           n_labels, est, score, rank, p_true, t, cf, rh, scored, (float*)nullptr);
    } else {
        if (!rowbuf) return -18;
        hipLaunchKernelGGL((calibrate_eval_kernel<false>), grid, dim3(256), 0, st, logits, M, K, a, b, y, label_map, n_labels, est, score,
                           rank, p_true, t, cf, rh, scored, rowbuf);
    }
    LAUNCH_CHECK();
    return 0;
}

int launch_mlp_group(const MlpGroupArgs& g, int members, hipStream_t st)
{
    if (members < 1 || members > ENSEMBLE_MAX || g.M < 1) return -18;
    int nmax = 0;
    for (int j = 0; j < members; ++j) {
        const MlpGroupMember& m = g.m[j];
        if (!m.X || !m.W || !m.bias || !m.Y || m.K < 4 || (m.K & 3) || m.N < 1) return -18;
        nmax = m.N > nmax ? m.N : nmax;
    }
    const dim3 grid((g.M + 63) / 64, (nmax + 63) / 64, members);
    hipLaunchKernelGGL(mlp_gemm_f32_group_kernel, grid, dim3(256), 0, st, g);
    LAUNCH_CHECK();
    return 0;
}

static int ensemble_check(int P, int K, int Mn, const EnsembleCal& cal)
{
    if (P < 1 || K < 1 || K > TOPK_LDS_MAX_K || Mn < 1 || Mn > ENSEMBLE_MAX) return -18;
    for (int j = 0; j < Mn; ++j)
        if (!cal.a[j] || !cal.b[j]) return -18;
    return 0;
}

int launch_ensemble_topk(const float* logits, int P, int G, int K, int Mn, size_t member_stride, const EnsembleCal& cal, int k,
                         int32_t* idx, float* scores, float* proba, float* stats, int32_t* votes, hipStream_t st)
{
    if (ensemble_check(P, K, Mn, cal) || G < 1 || G > VIEWS_MAX || k < 1 || k > K || !logits || !idx || !scores) return -18;
    hipLaunchKernelGGL(ensemble_topk_kernel, dim3((P + 3) / 4), dim3(256), (size_t)8 * K * sizeof(float), st, logits, P, G, K, Mn,
                       member_stride, cal, k, idx, scores, proba, stats, votes);
    LAUNCH_CHECK();
    return 0;
}

int launch_ensemble_eval(const float* logits, int M, int K, int Mn, size_t member_stride, const EnsembleCal& cal, const int32_t* y,
                         const int32_t* label_map, int n_labels, int32_t* est, float* score, int32_t* rank, float* p_true, float* stats,
                         int32_t* votes, long long* totals, long long* confusion, long long* rank_hist, hipStream_t st)
{
    if (ensemble_check(M, K, Mn, cal) || !logits || !y || !totals || (label_map && n_labels < 1)) return -18;
    const int nb = (M + 3) / 4;
    const dim3 grid(nb < 2048 ? nb : 2048);   // as calibrate_eval_kernel: the partial totals stay on chip while a workgroup walks rows
    const int hist_lds = (size_t)9 * K * sizeof(float) <= 65536;   // the rows and the counts inside 64 KB
    const size_t lds = (size_t)(hist_lds ? 9 : 8) * K * sizeof(float);
    hipLaunchKernelGGL(ensemble_eval_kernel, grid, dim3(256), lds, st, logits, M, K, Mn, member_stride, cal, y, label_map, n_labels, est,
                       score, rank, p_true, stats, votes, reinterpret_cast<unsigned long long*>(totals),
                       reinterpret_cast<unsigned long long*>(confusion), reinterpret_cast<unsigned long long*>(rank_hist), hist_lds);
    LAUNCH_CHECK();
    return 0;
}

int launch_rank_rows(const float* logits, int M, int K, const float* a, const float* b, const int32_t* scored, const int32_t* rank,
                     const uint8_t* sim_level, int n_levels, int kmax, long long* class_rank_hist, long long* hier_hist, float* rowbuf,
                     hipStream_t st)
{
    if (M < 1 || K < 1 || !scored || !rank || (sim_level == nullptr) != (hier_hist == nullptr)) return -18;
    if (sim_level && (n_levels < 1 || n_levels > 256 || kmax < 1 || kmax > K || kmax > RANK_MAX_K)) return -18;
    if (!sim_level && !class_rank_hist) return 0;   // nothing to add
    const int nb = (M + 3) / 4;
    const dim3 grid(nb < 2048 ? nb : 2048);   // as calibrate_eval_kernel: the partial tables stay on chip while a workgroup walks rows
    unsigned long long* ch = reinterpret_cast<unsigned long long*>(class_rank_hist);
    unsigned long long* hh = reinterpret_cast<unsigned long long*>(hier_hist);
    const size_t cells = sim_level ? (size_t)kmax * n_levels * sizeof(unsigned) : 0;   // at most 16 KB
    if (K <= TOPK_LDS_MAX_K) {
        hipLaunchKernelGGL((rank_rows_kernel<true>), grid, dim3(256), (size_t)4 * K * sizeof(float) + cells, st, logits, M, K, a, b, scored,
                           rank, sim_level, n_levels, kmax, ch, hh, (float*)nullptr);
    } else {
        if (sim_level && !rowbuf) return -18;
        hipLaunchKernelGGL((rank_rows_kernel<false>), grid, dim3(256), cells, st, logits, M, K, a, b, scored, rank, sim_level, n_levels,
                           kmax, ch, hh, rowbuf);
    }
    LAUNCH_CHECK();
    return 0;
}

int launch_crop(const uint8_t* image, int H, int W, const int32_t* rowcols, int n, uint8_t* out, hipStream_t st)
{
    dim3 grid((224 * 56 + 255) / 256, n, 1);
    hipLaunchKernelGGL(crop_kernel, grid, dim3(256), 0, st, image, H, W, rowcols, out);
    LAUNCH_CHECK();
    return 0;
}

int launch_crop_views(const uint8_t* image, int H, int W, const int32_t* rowcols, const uint8_t* views, int n, uint8_t* out,
                      hipStream_t st)
{
    dim3 grid((224 * 56 + 255) / 256, n, 1);
    hipLaunchKernelGGL(crop_views_kernel, grid, dim3(256), 0, st, image, H, W, rowcols, views, out);
    LAUNCH_CHECK();
    return 0;
}
