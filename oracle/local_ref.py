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
   - the expanded tensor in LDS (``k_mbconv.hip:434-437``, ``k_early.hip:562``, ``k_mid.hip:360``);
   - the gated operand fp16(g d) (``device_common.h:104-123`` ``gate_h8``; ``k_mid.hip:804``, ``k_tail.hip:490``, ``k_mbconv.hip:105``).
     ``thin_proj_kernel`` rounds fp16(g w) instead (``k_early.hip:24-27``, ``:66``): the same relative u on every product, and an
     absolute 2**-25 that multiplies |d| instead of |w| -- the project stage charges both;
   - the intermediate tensors of the fused B0 stem / block 0 / block 1 path (``k_early.hip:155``: gated block-0 operand;
     the projected block-0 output as the expand's MFMA operand; the stem tensor in LDS);
   - every stored fp16 output (``k_generic.hip:110``, ``k_early.hip:264``, ``k_mid.hip:203``, ``k_tail.hip:386``).
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

The comparison that uses these bounds (``tests/test_gpu_local.py``) allows 2 x bound per element: the factor covers the
second-order terms this first-order model drops.
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
    kind: str          # stem | expand | dw | fused_dw | stem_dw | b1_fused | gate | out | features
    block: int         # -1 for stem / features
    inputs: Tuple[str, ...]


def plan(arch, have) -> List[Stage]:
    """The stage list of a schedule that keeps the tensors ``have``.  ``b{i}.expand``, ``stem`` and ``b0.out`` decide between
    the fused and unfused forms; any other absent tensor is an error."""
    from mermaid_classifier_amd.weights import get_arch
    A = get_arch(arch)
    have = set(have)
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
            st.append(Stage(f"b{i}.out", "out", i, ins))
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


def run_stage(W: Weights, st: Stage, get: Callable[[str], np.ndarray]):
    """(ref, bound) of one stage on the inputs ``get(name)`` hands out (``"patches"``: the uint8 patches)."""
    a = [get(n) for n in st.inputs]
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
