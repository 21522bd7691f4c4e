"""Stage references for local parity: one backbone launch at a time, value AND per-element error bound.

TEST INFRASTRUCTURE ONLY (like the rest of ``oracle/``): only ``tests/`` imports this module.

A *stage* is one launch, or one fused group of launches, from HBM tensor(s) to an HBM tensor.  Each stage function takes
its inputs as numpy arrays exactly as ``Backbone.read_activation`` returns them (no re-rounding) plus the folded fp32
tensors of ``mermaid_classifier_amd.weights.fold`` (never the state dict, never a kernel's packing), evaluates the
operation in torch float64 with the same-pad rule of ``oracle.efficientnet_b0_ref.same_pad``, and returns ``(ref, bound)`` in
the layout ``read_activation`` returns: NHWC for tensors, (N, Ce) for gates, (N, F) for the features.

``bound`` is a first-order forward error bound, carried next to the value through the same convolutions run on ``|w|``
and ``|x|``.  With ``u = 2**-11`` (fp16 unit roundoff) and ``v = 2**-24`` (fp32) the model is:

1. **Inputs.**  Tensors read from the device are exact.
2. **Weights.**  Every conv, depthwise and squeeze-excite weight carries a relative error <= u: the host rounds them to
   fp16 after folding the log2(e) of the scaled SiLU domain (``csrc/backbone_pack.h``: ``pack_pw``, ``pack_frag``, ``pack_stem``, ``pack_expand_rows``,
   ``pack_dw_pairs``, ``pack_dw_toeplitz``, ``pack_se_fc1_t16`` / ``pack_se_fc2_t16``); the fp32 taps of ``dwconv_kernel`` / ``mbconv_a_kernel`` and the fp32 squeeze-excite weights of ``se_small`` /
   ``se_wide`` / ``se_fused`` are charged the same (an overestimate there).  Biases are exact.
3. **Accumulation.**  A K-term dot product accumulated in fp32 (MFMA, ``v_dot2_f32_f16``, ``v_fma_mix_f32``) carries
   <= (K + 4) v (sum|w x| + |bias| + |skip|).  The ``+ 4`` is for what surrounds the dot product in fp32: the bias times log2(e)
   (``pack_bias`` of the stem's and the depthwise bias), the skip addition (``k_early.hip:84``, ``k_tail.hip:207``) and the fp32 factor 1/log2(e) that
   ``mmc_backbone_read_activation`` applies to SiLU-domain tensors on the way out (``mmc_api.cpp``, ``mmc_backbone_read_activation``).
4. **Values held in fp16.**  Each value the kernel holds in fp16 between phases carries a relative u plus an absolute 2**-25
   (half the smallest subnormal):
   - the expanded tensor in LDS (``k_mbconv.hip:434-437``, ``k_early.hip:562``, ``k_mid.hip:360``; block 11 inside
     ``tail7_kernel``: the chunk ``E[196][96]``, ``k_tail.hip:318-323``);
   - the gated operand fp16(g d) (``device_common.h:104-123`` ``gate_h8``; ``k_mid.hip:804``, ``k_tail.hip:490``, ``k_mbconv.hip:105``).
     ``thin_proj_kernel`` rounds fp16(g w) instead (``k_early.hip:24-27``, ``:66``): the same relative u on every product, and an
     absolute 2**-25 that multiplies |d| instead of |w| -- the project stage charges both;
   - the intermediate tensors of the fused B0 stem / block 0 / block 1 path (``k_early.hip:155``: gated block-0 operand;
     the projected block-0 output as the expand's MFMA operand; the stem tensor in LDS);
   - every stored fp16 output (``k_generic.hip:110``, ``k_early.hip:264``, ``k_mid.hip:203``, ``k_tail.hip:386``); block 11's
     depthwise output inside ``tail7_kernel`` is the compact ``D11[49][672]`` in LDS (``k_tail.hip:386-390``), which per-tensor mode
     copies out unchanged (``k_tail.hip:398-404``).
   Gates and features are fp32 and carry a relative v instead.
   The stem's padding value 255 mean - 128 is held in fp16 like the pixels beside it (``k_generic.hip:64-67``): the padded
   pixels carry a relative u, the real ones (u8 - 128) are exact.
5. **Activations.**  Errors pass through SiLU with a factor 1.1 (max |silu'| = 1.0998) and through sigmoid with a factor
   0.25.  Each evaluation adds a relative 8 v: ``v_exp_f32`` and ``v_rcp_f32`` at one ulp each plus the add and the multiply
   (``device_common.h:18-27``).
6. **Pool in the gate stage.**  The kernel pools the fp32 values before rounding them (``k_generic.hip:534``,
   ``k_early.hip:263``, ``k_mid.hip:202``, ``k_tail.hip:754``); the reference pools the fp16 tensor it is given.  The pool
   therefore carries u mean|d| per channel (plus its own fp32 summation, rule 3), which then passes through FC1, SiLU,
   FC2 and sigmoid under rules 2, 3 and 5.

7. **fp8 project convs** (``out_fp8``; ``pw_gemm_fp8_kernel``, ``k_generic.hip``).  The operands are not rounded values with an
   error: they are e4m3 CODES, and the reference replicates them bit for bit with its own codec (``e4m3_encode`` /
   ``e4m3_decode``, independent of ``backbone_pack.h``).  Weights: in float32, ``amax`` per output channel, ``sc = amax / 448`` (1
   where ``amax == 0``), codes of ``w / sc``, ``sw = float32(float64(sc) / log2 e)`` -- what ``pack_fp8`` does.  Activations: the
   device's fp16 depthwise tensor is recovered from ``read_activation``'s value (times fp32 log2 e, rounded to fp16: the round trip
   errs by 2**-23 relative, and re-applying the library's factor must reproduce the input bits -- asserted); then in float32,
   in the kernel's order, ``v = float32(d16) g``, ``mx = max |v|`` over the row, ``inv = 447 / mx``, ``sx = mx float32(1 / 447)``,
   codes of ``v inv`` (``mx == 0``: codes 0, ``sx = 0``).  The value is ``(sum_k qw qx) sx sw + bias (+ skip)`` in float64 (the
   code products are exact there).  What is left is rule 3, ``(K + 4) v (sum|qw qx| sx sw + |bias| + |skip|)``, and rule 4 on the
   stored output.  No weight term ``u``: the weights are replicated, not rounded.
   *Ambiguous operands.*  Every step above is one correctly rounded IEEE fp32 operation, so the codes should match exactly; the
   one allowance is for a division or multiply that differs in its last bit on the device.  An activation operand whose ``v inv``
   lies within 4 fp32 ulps of an e4m3 rounding boundary may land on the neighbouring code: for those operands only,
   ``|qw| (the e4m3 step at that boundary) sx sw`` is added to the bound of the outputs they feed, and their count is returned.
   Uniform fp32 products put 8 / 2**20 ~ 1e-5 of the operands there; the checks refuse a stage with more than ``AMBIGUOUS_MAX``
   (1e-4), so the term cannot hide a kernel that quantises differently.
   *The instruction's own sum.*  Rule 3 is applied as it stands, although ``v_mfma_scale_f32_16x16x128_f8f6f4`` does not sum its
   128 products the way the rule assumes.
   What the device tensors show (MI355X, the three parity patches, both schedules): every element is within 2 x bound, worst
   1.12 at K = 336 (2 of 65856 elements over 1 x) and falling with K (0.85 at 672, 0.77 at 960, 0.71 at 1632, 0.42 at 2688); the
   CPU emulation's plain fp32 sums give 0.86 at K = 336 and 0.42 at 2688 on the oracle's taps.  The part of |got - ref| that the
   fp16 store cannot explain reaches 30-56 units of the accumulator (of sx sw) whatever K is, i.e. 435 x 2**-24 sum|qw qx| at
   K = 336 (rule 3 alone: 340) down to 175 x 2**-24 at K = 2688 (2692), and only 90-93 % of the outputs equal the fp16 rounding of
   an exact sum through the fp32 epilogue.  No structure by row, column, fragment or channel.  So the instruction's internal sum is
   coarser than a sequential fp32 one by an amount that does not grow with K and that the factor 2 absorbs at these shapes.
   A micro-run against exact sums (``tools/ubench/mfma_f8_sum.hip`` -> ``profiles/mfma_f8_sum.txt``) says why: the instruction sums
   its products in groups of 8 consecutive k and drops, inside a group, whatever lies below 2**-15 of the group's largest product
   (2**2 next to 448 x 448; 7 of 64 equal small products lost; cancellation of the large ones does not bring it back), keeps 2**-23
   of the largest product across groups, and adds the finished sum to C with round to nearest even.  On random codes one
   instruction errs by up to 2**-11 of its largest product, 1045-1243 x 2**-24 sum|p| where rule 3 allows 132.  Real rows, one
   operand at 447 and most far below, stay much closer (the 435 above).  Rule 3 is therefore NOT a proven bound for this
   instruction: it is the stated rule, it holds with the factor 2 on these tensors, and a sound replacement would add a term of the
   form 2**-15 sum over groups of 8 of max|qw qx| -- left for a change that also re-proves the sharpness list against it.

The comparison that uses these bounds (``tests/test_gpu_local.py``, ``tests/test_gpu_local_fp8.py``) allows 2 x bound per element:
the factor covers the second-order terms this first-order model drops.
"""

from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from oracle.efficientnet_b0_ref import same_pad

U = 2.0 ** -11     # fp16 unit roundoff
V = 2.0 ** -24     # fp32 unit roundoff
TINY16 = 2.0 ** -25   # half the smallest fp16 subnormal
SILU_LIP = 1.1
SIGMOID_LIP = 0.25
ACT_REL = 8 * V

F64 = torch.float64


def _t(a) -> torch.Tensor:
    return torch.as_tensor(np.asarray(a), dtype=F64) if not isinstance(a, torch.Tensor) else a.to(F64)


class Weights:
    """The folded fp32 tensors of ``weights.fold`` by name, as float64, plus the block table."""

    def __init__(self, folded, arch):
        from mermaid_classifier_amd.weights import get_arch
        self.arch = get_arch(arch)
        self.t: Dict[str, torch.Tensor] = {k: _t(v) for k, v in folded}

    def __getitem__(self, k: str) -> torch.Tensor:
        return self.t[k]


# ---- (value, error) building blocks; activations are NHWC float64 ---------------------------------------------------

def _held16(val, err):
    return err + U * val.abs() + TINY16


def _silu(val, err):
    y = val * torch.sigmoid(val)
    return y, SILU_LIP * err + ACT_REL * y.abs()


def _sigmoid(val, err):
    y = torch.sigmoid(val)
    return y, SIGMOID_LIP * err + ACT_REL * y


def _linear(x, ex, w, b):
    """y[..., n] = sum_k x[..., k] w[n, k] + b[n] over the last axis (1x1 conv / FC)."""
    K = w.shape[1]
    wa = w.abs().T
    val = x @ w.T + b
    mag = x.abs() @ wa
    err = ex @ wa + U * mag + (K + 4) * V * (mag + b.abs())
    return val, err


def _pad_hw(x, k, s, value=None):
    (pt, pb), (pl, pr) = same_pad(x.shape[1], k, s), same_pad(x.shape[2], k, s)
    if value is None:
        return torch.nn.functional.pad(x, (0, 0, pl, pr, pt, pb))
    out = value.to(F64).expand(x.shape[0], x.shape[1] + pt + pb, x.shape[2] + pl + pr, x.shape[3]).clone()
    out[:, pt:pt + x.shape[1], pl:pl + x.shape[2], :] = x
    return out


def _depthwise(x, ex, w, b, s):
    """w [C][k][k]; same-pad with zeros (the padding lives in the depthwise's own input domain)."""
    k = w.shape[-1]
    Ho, Wo = -(-x.shape[1] // s), -(-x.shape[2] // s)
    xp, ep = _pad_hw(x, k, s), _pad_hw(ex, k, s)
    val = torch.zeros(x.shape[0], Ho, Wo, x.shape[3], dtype=F64)
    mag = torch.zeros_like(val)
    err = torch.zeros_like(val)
    for ky in range(k):
        for kx in range(k):
            sl = (slice(None), slice(ky, ky + (Ho - 1) * s + 1, s), slice(kx, kx + (Wo - 1) * s + 1, s))
            t, ta = w[:, ky, kx], w[:, ky, kx].abs()
            val += xp[sl] * t
            mag += xp[sl].abs() * ta
            err += ep[sl] * ta
    val = val + b
    err = err + U * mag + (k * k + 4) * V * (mag + b.abs())
    return val, err


def _stem_conv(W: Weights, patches):
    """u8 patches -> stem conv + bias (pre-activation), (value, error)."""
    x = _t(np.asarray(patches, dtype=np.float64) - 128.0)
    pv = W["stem.padval"].view(1, 1, 1, 3)
    xp = _pad_hw(x, 3, 2, value=pv)
    ep = _pad_hw(torch.zeros_like(x), 3, 2, value=U * pv.abs())      # rule 4: the padding value is held in fp16
    w = W["stem.weight"].view(-1, 3, 3, 3)                            # [n][ky][kx][c]
    b = W["stem.bias"]
    Ho = -(-x.shape[1] // 2)
    val = torch.zeros(x.shape[0], Ho, Ho, w.shape[0], dtype=F64)
    mag = torch.zeros_like(val)
    err = torch.zeros_like(val)
    for ky in range(3):
        for kx in range(3):
            sl = (slice(None), slice(ky, ky + 2 * Ho - 1, 2), slice(kx, kx + 2 * Ho - 1, 2))
            t = w[:, ky, kx, :].T
            val += xp[sl] @ t
            mag += xp[sl].abs() @ t.abs()
            err += ep[sl] @ t.abs()
    val = val + b
    err = err + U * mag + (27 + 4) * V * (mag + b.abs())
    return val, err


def _out(val, err):
    return val.numpy(), err.numpy()


def _block(W: Weights, i: int):
    k, s, e, cin, cout = W.arch.blocks[i]
    return k, s, e, cin, cout


# ---- the stages --------------------------------------------------------------------------------------------------

def stem(W: Weights, patches):
    """uint8 patches -> stem conv + SiLU (the unfused schedules' and B4's ``stem``)."""
    y, e = _silu(*_stem_conv(W, patches))
    return _out(y, _held16(y, e))


def expand(W: Weights, i: int, x):
    """block input -> 1x1 expand conv + SiLU (``b{i}.expand``, unfused)."""
    x = _t(x)
    y, e = _silu(*_linear(x, torch.zeros_like(x), W[f"b{i}.expand.weight"], W[f"b{i}.expand.bias"]))
    return _out(y, _held16(y, e))


def dw(W: Weights, i: int, x):
    """depthwise input (the expanded tensor; the block input where the expand ratio is 1) -> depthwise + SiLU."""
    x = _t(x)
    s = _block(W, i)[1]
    y, e = _silu(*_depthwise(x, torch.zeros_like(x), W[f"b{i}.dw.weight"], W[f"b{i}.dw.bias"], s))
    return _out(y, _held16(y, e))


def _expand_dw(W: Weights, i: int, x, ex):
    s = _block(W, i)[1]
    y, e = _silu(*_linear(x, ex, W[f"b{i}.expand.weight"], W[f"b{i}.expand.bias"]))
    e = _held16(y, e)                                                  # the expanded tensor in LDS
    y, e = _silu(*_depthwise(y, e, W[f"b{i}.dw.weight"], W[f"b{i}.dw.bias"], s))
    return y, _held16(y, e)


def fused_dw(W: Weights, i: int, x):
    """block input -> expand + SiLU, held in fp16, -> depthwise + SiLU (``b{i}.dw`` of the fused schedules)."""
    x = _t(x)
    return _out(*_expand_dw(W, i, x, torch.zeros_like(x)))


def stem_dw(W: Weights, patches):
    """uint8 patches -> stem + SiLU, held in fp16, -> block 0's depthwise + SiLU (B0 fused ``b0.dw``)."""
    y, e = _silu(*_stem_conv(W, patches))
    e = _held16(y, e)
    y, e = _silu(*_depthwise(y, e, W["b0.dw.weight"], W["b0.dw.bias"], _block(W, 0)[1]))
    return _out(y, _held16(y, e))


def _gated_project(W: Weights, i: int, d, g, skip=None):
    gd = d * g[:, None, None, :]
    e = U * gd.abs() + TINY16                                           # fp16(g d)
    w, b = W[f"b{i}.project.weight"], W[f"b{i}.project.bias"]
    y, e = _linear(gd, e, w, b)
    e = e + TINY16 * d.abs().sum(-1, keepdim=True)                      # thin_proj: fp16(g w), absolute part times |d|
    if skip is not None:
        y = y + skip
        e = e + (w.shape[1] + 4) * V * skip.abs()
    return y, e


def b1_fused(W: Weights, d0, g0):
    """B0 fused ``b1.dw``: block 0's depthwise output and gate -> fp16(g d), project, held in fp16, block 1's expand +
    SiLU, held in fp16, depthwise + SiLU."""
    y, e = _gated_project(W, 0, _t(d0), _t(g0))
    return _out(*_expand_dw(W, 1, y, _held16(y, e)))


def gate(W: Weights, i: int, d):
    """``b{i}.dw`` -> mean over HW_out, FC1 + SiLU, FC2, sigmoid: (N, Ce) fp32."""
    d = _t(d)
    hw = d.shape[1] * d.shape[2]
    p = d.mean(dim=(1, 2))
    pa = d.abs().mean(dim=(1, 2))
    e = U * pa + (hw + 4) * V * pa                                      # rule 6 + the pool's own summation
    r, e = _silu(*_linear(p, e, W[f"b{i}.se.reduce.weight"], W[f"b{i}.se.reduce.bias"]))
    z, e = _linear(r, e, W[f"b{i}.se.expand.weight"], W[f"b{i}.se.expand.bias"])
    g, e = _sigmoid(z, e)
    return _out(g, e + V * g)


def out(W: Weights, i: int, d, g, skip=None):
    """``b{i}.dw``, the device's ``b{i}.gate`` (and the block input where the block has a skip) -> fp16(g d), project + bias
    (+ skip)."""
    y, e = _gated_project(W, i, _t(d), _t(g), None if skip is None else _t(skip))
    return _out(y, _held16(y, e))


# ---- rule 7: the fp8 project conv on replicated e4m3 operands ------------------------------------------------------------

LOG2E = 1.4426950408889634
AMBIGUOUS_ULPS = 4
AMBIGUOUS_MAX = 1e-4      # largest share of a stage's activation operands that may sit on a rounding boundary


def e4m3_decode(codes) -> np.ndarray:
    """OCP e4m3fn codes (uint8) -> float32: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities, 0x7F / 0xFF are NaN."""
    c = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e - 10.0))
    mag = np.where((e == 15) & (m == 7), np.nan, mag)
    return np.where(c & 0x80, -mag, mag).astype(np.float32)


_E4M3_VALUES = e4m3_decode(np.arange(127)).astype(np.float64)             # 0 .. 448, ascending
_E4M3_MIDS = 0.5 * (_E4M3_VALUES[:-1] + _E4M3_VALUES[1:])                  # the 126 rounding boundaries (exact)


def e4m3_encode(x) -> np.ndarray:
    """float32 -> OCP e4m3fn codes: round to nearest, ties to the even code, saturating at +-448, subnormals down to 2**-9
    (below half of that, and at the tie 2**-10: zero); NaN -> 0x7F."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):                                    # a signalling NaN stays a NaN
        a = np.abs(x).astype(np.float64)
    idx = np.searchsorted(_E4M3_MIDS, a, side="left")                      # boundaries strictly below |x|; NaN sorts last
    tie = (idx < 126) & (a == _E4M3_MIDS[np.minimum(idx, 125)])
    idx = np.where(tie & (idx % 2 == 1), idx + 1, idx)
    code = np.where(np.isnan(a), 0x7F, idx).astype(np.uint8)
    return code | np.where(np.signbit(x) & ~np.isnan(a), 0x80, 0).astype(np.uint8)


def _e4m3_ambiguity(t: np.ndarray) -> np.ndarray:
    """float32 values about to be encoded -> the e4m3 step at the rounding boundary within AMBIGUOUS_ULPS fp32 ulps, else 0."""
    a = np.abs(t).astype(np.float64)
    ulp = np.spacing(np.abs(t)).astype(np.float64)
    hi = np.minimum(np.searchsorted(_E4M3_MIDS, a, side="left"), 125)
    lo = np.maximum(hi - 1, 0)
    j = np.where(np.abs(a - _E4M3_MIDS[lo]) < np.abs(a - _E4M3_MIDS[hi]), lo, hi)
    near = np.abs(a - _E4M3_MIDS[j]) <= AMBIGUOUS_ULPS * ulp
    return np.where(near, _E4M3_VALUES[j + 1] - _E4M3_VALUES[j], 0.0)


def fp8_weight_codes(w):
    """folded fp32 project weight [N][K] -> (codes uint8 [N][K], sw float32 [N]) exactly as ``pack_fp8`` quantises it."""
    w = np.asarray(w, dtype=np.float32)
    amax = np.abs(w).max(axis=1)
    sc = np.where(amax > 0, amax / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    codes = e4m3_encode(w / sc[:, None])
    sw = (sc.astype(np.float64) / LOG2E).astype(np.float32)
    return codes, sw


def fp8_activation_rows(d, g):
    """``read_activation``'s ``b{i}.dw`` (N, H, W, K) and ``b{i}.gate`` (N, K) -> the kernel's gated rows in float32, (N H W, K):
    v = float32(d16) g on the recovered fp16 tensor."""
    read = np.asarray(d, dtype=np.float32)
    d16 = (read * np.float32(LOG2E)).astype(np.float16)
    back = d16.astype(np.float32) * np.float32(1.0 / LOG2E)                # mmc_backbone_read_activation's factor
    if not np.array_equal(back.view(np.uint32), read.view(np.uint32)):
        raise ValueError("the depthwise tensor is not fp16 times the library's fp32 1 / log2(e): the fp16 bits cannot be recovered")
    n, h, w_, k = read.shape
    v = d16.astype(np.float32) * np.asarray(g, dtype=np.float32)[:, None, None, :]
    return v.reshape(n * h * w_, k)


def fp8_activation_codes(v):
    """gated rows float32 (M, K) -> (codes uint8 (M, K), sx float32 (M,), t = v inv float32 (M, K)), the kernel's recipe."""
    v = np.asarray(v, dtype=np.float32)
    mx = np.abs(v).max(axis=1)
    pos = mx > 0
    safe = np.where(pos, mx, np.float32(1.0)).astype(np.float32)
    inv = np.where(pos, np.float32(447.0) / safe, np.float32(0.0)).astype(np.float32)
    sx = np.where(pos, mx * (np.float32(1.0) / np.float32(447.0)), np.float32(0.0)).astype(np.float32)
    t = v * inv[:, None]
    return e4m3_encode(t), sx, t


class Fp8Info(NamedTuple):
    ambiguous: int     # activation operands within AMBIGUOUS_ULPS fp32 ulps of an e4m3 rounding boundary
    operands: int      # rows x K

    @property
    def share(self) -> float:
        return self.ambiguous / max(self.operands, 1)


def out_fp8(W: Weights, i: int, d, g, skip=None):
    """``b{i}.dw``, the device's ``b{i}.gate`` (and the block input where the block has a skip) -> the project conv on e4m3
    operands (rule 7): ``(ref, bound, Fp8Info)``."""
    w = W[f"b{i}.project.weight"].numpy()
    b = W[f"b{i}.project.bias"].numpy()
    n_out, K = w.shape
    cw, sw = fp8_weight_codes(w)
    cx, sx, t = fp8_activation_codes(fp8_activation_rows(d, g))
    qw, qx = e4m3_decode(cw).astype(np.float64), e4m3_decode(cx).astype(np.float64)
    scale = sx.astype(np.float64)[:, None] * sw.astype(np.float64)[None, :]
    y = (qx @ qw.T) * scale + b
    mag = (np.abs(qx) @ np.abs(qw).T) * scale + np.abs(b)
    step = _e4m3_ambiguity(t)
    amb = (step @ np.abs(qw).T) * scale
    shape = tuple(np.shape(d)[:3]) + (n_out,)
    y, mag, amb = y.reshape(shape), mag.reshape(shape), amb.reshape(shape)
    if skip is not None:
        s = np.asarray(skip, dtype=np.float64)
        y = y + s
        mag = mag + np.abs(s)
    err = (K + 4) * V * mag + amb
    bound = err + U * np.abs(y) + TINY16                                   # rule 4: the stored fp16 output
    return y, bound, Fp8Info(int(np.count_nonzero(step)), int(step.size))


def features(W: Weights, x):
    """last block output -> head conv + SiLU + mean over HW: ``extract``'s return value, (N, F) fp32."""
    x = _t(x)
    hw = x.shape[1] * x.shape[2]
    y, e = _silu(*_linear(x, torch.zeros_like(x), W["head.weight"], W["head.bias"]))
    f = y.mean(dim=(1, 2))
    e = e.mean(dim=(1, 2)) + (hw + 4) * V * y.abs().mean(dim=(1, 2))
    return _out(f, e + V * f.abs())


# ---- which stages a schedule has, from the tensors it keeps -------------------------------------------------------------

class Stage(NamedTuple):
    name: str          # the tensor it produces
    kind: str          # stem | expand | dw | fused_dw | stem_dw | b1_fused | gate | out | out_fp8 | features
    block: int         # -1 for stem / features
    inputs: Tuple[str, ...]


def plan(arch, have, fp8_blocks=()) -> List[Stage]:
    """The stage list of a schedule that keeps the tensors ``have``.  ``b{i}.expand``, ``stem`` and ``b0.out`` decide between
    the fused and unfused forms; any other absent tensor is an error.  The project convs of ``fp8_blocks`` run on e4m3
    operands: kind ``out_fp8``."""
    from mermaid_classifier_amd.weights import get_arch
    A = get_arch(arch)
    have = set(have)
    fp8 = set(fp8_blocks)
    st: List[Stage] = []
    if "stem" in have:
        st.append(Stage("stem", "stem", -1, ("patches",)))
    for i, (k, s, e, cin, cout) in enumerate(A.blocks):
        x_in = "stem" if i == 0 else f"b{i - 1}.out"
        for need in (f"b{i}.dw", f"b{i}.gate"):
            if need not in have:
                raise KeyError(f"{need} is not kept")
        if e != 1 and f"b{i}.expand" in have:
            if x_in not in have:
                raise KeyError(f"{x_in} is not kept")
            st.append(Stage(f"b{i}.expand", "expand", i, (x_in,)))
            st.append(Stage(f"b{i}.dw", "dw", i, (f"b{i}.expand",)))
        elif x_in in have:
            st.append(Stage(f"b{i}.dw", "dw" if e == 1 else "fused_dw", i, (x_in,)))
        elif i == 0:
            st.append(Stage("b0.dw", "stem_dw", 0, ("patches",)))
        elif i == 1 and A.name == "b0":
            st.append(Stage("b1.dw", "b1_fused", 1, ("b0.dw", "b0.gate")))
        else:
            raise KeyError(f"{x_in} is not kept")
        st.append(Stage(f"b{i}.gate", "gate", i, (f"b{i}.dw",)))
        if f"b{i}.out" in have:
            ins = (f"b{i}.dw", f"b{i}.gate") + ((x_in,) if s == 1 and cin == cout else ())
            if len(ins) == 3 and x_in not in have:
                raise KeyError(f"{x_in} is not kept")
            st.append(Stage(f"b{i}.out", "out_fp8" if i in fp8 else "out", i, ins))
        elif not (i == 0 and A.name == "b0"):
            raise KeyError(f"b{i}.out is not kept")
    st.append(Stage("features", "features", -1, (f"b{len(A.blocks) - 1}.out",)))
    return st


def tensor_shape(arch, name: str, n: int) -> Tuple[int, ...]:
    """Shape of a kept tensor in ``read_activation``'s layout."""
    from mermaid_classifier_amd.weights import get_arch
    A = get_arch(arch)
    if name == "features":
        return (n, A.feature_dim)
    h = 112
    if name == "stem":
        return (n, h, h, A.stem)
    for i, (k, s, e, cin, cout) in enumerate(A.blocks):
        ho = -(-h // s)
        shapes = {f"b{i}.expand": (n, h, h, cin * e), f"b{i}.dw": (n, ho, ho, cin * e), f"b{i}.gate": (n, cin * e),
                  f"b{i}.out": (n, ho, ho, cout)}
        if name in shapes:
            return shapes[name]
        h = ho
    raise KeyError(name)


def run_stage(W: Weights, st: Stage, get: Callable[[str], np.ndarray], info: Optional[dict] = None):
    """(ref, bound) of one stage on the inputs ``get(name)`` hands out (``"patches"``: the uint8 patches).  An ``out_fp8`` stage
    leaves its ``Fp8Info`` in ``info[st.name]``."""
    a = [get(n) for n in st.inputs]
    if st.kind == "out_fp8":
        ref, bound, amb = out_fp8(W, st.block, a[0], a[1], a[2] if len(a) == 3 else None)
        if info is not None:
            info[st.name] = amb
        return ref, bound
    if st.kind == "stem":
        return stem(W, a[0])
    if st.kind == "stem_dw":
        return stem_dw(W, a[0])
    if st.kind == "b1_fused":
        return b1_fused(W, a[0], a[1])
    if st.kind == "features":
        return features(W, a[0])
    if st.kind == "out":
        return out(W, st.block, a[0], a[1], a[2] if len(a) == 3 else None)
    return {"expand": expand, "dw": dw, "fused_dw": fused_dw, "gate": gate}[st.kind](W, st.block, a[0])


def border_patch() -> np.ndarray:
    """(224,224,3) uint8: constant 128 inside, a 1-pixel 0/255 checkerboard in a 16-pixel frame along all four edges."""
    p = np.full((224, 224, 3), 128, dtype=np.uint8)
    yy, xx = np.mgrid[0:224, 0:224]
    frame = (yy < 16) | (yy >= 208) | (xx < 16) | (xx >= 208)
    cb = (((yy + xx) & 1) * 255).astype(np.uint8)
    p[frame] = cb[frame][:, None]
    return p


def parity_patches() -> np.ndarray:
    """The three patches of the local-parity checks: image-like, white noise, border-heavy."""
    from oracle import efficientnet_b0_ref as ref
    return np.stack([ref.natural_patches(1, seed=7)[0], ref.synthetic_patches(1, seed=42)[0], border_patch()])


def exceed_report(got: np.ndarray, ref: np.ndarray, bound: np.ndarray, factor: float = 2.0) -> Optional[str]:
    """None when |got - ref| <= factor * bound everywhere; otherwise the worst element and where the excesses sit."""
    diff = np.abs(got.astype(np.float64) - ref)
    over = diff > factor * bound
    if not over.any():
        return None
    ratio, idx = worst_ratio(got, ref, bound)
    axes = {4: ("patch", "row", "col", "channel"), 2: ("patch", "channel")}[got.ndim]
    where = ", ".join(f"{a} {int(v)}" for a, v in zip(axes, idx))
    lines = [f"worst element ({where}): got {float(got[idx]):.7g} ref {float(ref[idx]):.7g} bound {float(bound[idx]):.3g} "
             f"(|got - ref| / bound = {ratio:.2f}); {int(over.sum())} of {over.size} elements over {factor:g} x bound"]
    pos = np.nonzero(over)

    def hist(label, v):
        c = np.bincount(v)
        nz = np.nonzero(c)[0]
        lines.append(f"  by {label}: " + " ".join(f"{int(k)}:{int(c[k])}" for k in nz[:40]) + (" ..." if len(nz) > 40 else ""))
    hist("patch", pos[0])
    if got.ndim == 4:
        hist("row", pos[1])
        hist("col", pos[2])
    hist("channel mod 16", pos[-1] % 16)
    return "\n".join(lines)


def worst_ratio(got: np.ndarray, ref: np.ndarray, bound: np.ndarray):
    """(max |got - ref| / bound, its index)."""
    diff = np.abs(got.astype(np.float64) - ref)
    r = np.where(bound > 0, diff / np.maximum(bound, 1e-300), np.where(diff > 0, np.inf, 0.0))
    idx = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[idx]), tuple(int(v) for v in idx)
