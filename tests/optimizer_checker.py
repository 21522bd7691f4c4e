"""The float64 reference and the derived bounds of the trainer's optimiser options (include/mmc.h, "optimiser options"), and the
inputs ``tests/test_optimizer_host.py`` and ``tests/test_gpu_optimizer.py`` share.

Gradients.  ``oracle.mlp_step_ref.step_ref`` gives the float64 gradient ``g_ref`` of a step and a first-order bound ``e`` on every
element of the device's fp32 gradient ``g`` (|g - g_ref| <= e); everything below is derived from those two and the fp32 unit
roundoff v = 2^-24.

1. Norm.  The device sums x^2 over the 2L tensors: per tensor a chain of ``trips = ceil(n / 65536)`` fused multiply-adds per thread
   and a binary tree of depth 8 over the 256 threads, then over the 2L x 256 partials a chain of 2L additions per thread and the
   same tree.  Every term is non-negative and passes through at most D = trips + 8 + 2L + 8 roundings, so
   total_dev = sum x_i^2 (1 + t_i) with |t_i| <= D v (first order), sqrtf halves that and rounds once:
       | norm_dev - ||g||_2 |  <=  (D / 2 + 1) v ||g||_2
   and by the triangle inequality | ||g||_2 - ||g_ref||_2 | <= ||g - g_ref||_2 <= ||e||_2.  So
       norm_bound = ||e||_2 + (D / 2 + 1) v (||g_ref||_2 + ||e||_2).
2. Coefficient.  coef = fminf(1, fl(M) / fl(norm + fl(1e-6))): four roundings (M, 1e-6, the add, the division) on top of the norm's
   error, so where the reference clips (coef_ref < 1)
       coef_bound = coef_ref (norm_bound / (norm_ref + 1e-6) + 4 v).
3. Clipped gradient.  The device writes fl(g coef); against coef_ref g_ref, per element and first order,
       clip_bound = coef_ref e + (|g_ref| + e) coef_bound + v coef_ref |g_ref|.
4. Averaged weights.  s' = s + om_d (p - s) with om_d = (float)(1.0 - decay) is three fp32 operations in a written order with nothing
   fused: numpy float32 replays it bit for bit (``ema_replay``), so there is no bound to derive.

``emulate_norm`` replays the device's summation order in numpy float32 (the fused multiply-add as the float32 of the float64
x * x + s, which is exact up to a double rounding); the host tests hold it to bounds 1 and 2 with e = 0, which is how the bounds are
shown to be sound before any GPU run.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import mlp_step_ref as sr

V = sr.V
F32, F64 = np.float32, np.float64
STRIDE = 256 * 256            # elements one trip of sumsq_kernel's fixed 256 x 256 grid covers

# ---- the shapes -------------------------------------------------------------------------------------------------------------------
# 1028 x 65 = 66 820 weights: a ragged second trip of the 65 536-thread grid; 65 and 130 cross a 64-wide GEMM tile; the biases are
# shorter than one block; 164 rows in mini-batches of 67: three steps, the last one of 30 rows.
WIDTHS = (1028, 65, 130)
MB, ROWS = 67, 164
ALPHA = 20.0                  # alpha / mb W is then a third of a weight: the L2 term is a visible part of the norm
# seeds for which step_ref's margin condition holds on rows [0, 67) (tests/test_optimizer_host.py checks it on the CPU)
SEEDS = {5: 5, 108: 29}


def dims_of(K: int) -> Tuple[int, ...]:
    return WIDTHS + (K,)


def make_case(K: int, seed: Optional[int] = None):
    """-> (weights, biases, class weights or None, X [164][1028], y) for K = 5 (class weights, one of them zero) or K = 108.

    The rows are small (0.05 x Gaussian), the first hidden layer's biases are 0.3 x Gaussian and the second's lie outside (-1, 1):
    the first layer's ReLU mask varies with the row while no pre-activation sits within the fp32 error of 0 -- at an input width
    of 1028 ``step_ref``'s margin condition fails for plain Gaussian rows on every seed."""
    rng = np.random.default_rng([77, K, SEEDS[K] if seed is None else seed])
    ws, bs = sr.make_params(rng, dims_of(K))
    bs[0] = (0.3 * rng.standard_normal(bs[0].shape)).astype(F32)
    bs[1] = (rng.choice([-1.0, 1.0], bs[1].shape) * (1.0 + 0.3 * np.abs(rng.standard_normal(bs[1].shape)))).astype(F32)
    cw = sr.make_weights(rng, K) if K == 5 else None
    X, y = sr.make_rows(rng, ROWS, WIDTHS[0], K, cw)
    X = (F32(0.05) * X).astype(F32)
    if cw is not None:                      # every mini-batch of the pass carries weight
        for start in range(0, ROWS, MB):
            y[start] = int(np.flatnonzero(cw > 0)[0])
    return ws, bs, cw, X, y


def grad_names(L: int) -> List[str]:
    """The order of the device's sum: gW0, gb0, gW1, gb1, ..."""
    return [n for l in range(L) for n in (f"gW{l}", f"gb{l}")]


# ---- 1-3: the float64 reference and its bounds -----------------------------------------------------------------------------------------

def depth(sizes: Sequence[int]) -> int:
    """D of the module docstring for tensors of these sizes (2L of them)."""
    trips = max(-(-int(n) // STRIDE) for n in sizes)
    return trips + 8 + len(sizes) + 8


def norm_ref(ref: Dict[str, np.ndarray], bound: Optional[Dict[str, np.ndarray]], L: int) -> Tuple[float, float]:
    """-> (||g_ref||_2, norm_bound) over gW / gb of ``step_ref``'s (ref, bound); ``bound=None``: e = 0 (the summation alone)."""
    names = grad_names(L)
    n = float(np.sqrt(sum(float((np.asarray(ref[k], F64) ** 2).sum()) for k in names)))
    e = 0.0 if bound is None else float(np.sqrt(sum(float((np.asarray(bound[k], F64) ** 2).sum()) for k in names)))
    D = depth([np.asarray(ref[k]).size for k in names])
    return n, e + (0.5 * D + 1.0) * V * (n + e)


def coef_ref(norm: float, max_norm: float) -> float:
    """torch.nn.utils.clip_grad_norm_'s coefficient in float64: min(1, max_norm / (norm + 1e-6))."""
    return min(1.0, float(max_norm) / (float(norm) + 1e-6))


def clip_ref(ref: Dict[str, np.ndarray], bound: Optional[Dict[str, np.ndarray]], L: int, max_norm: float):
    """-> (coef_ref, coef_bound, {name: coef_ref g_ref}, {name: clip_bound}) for a ``max_norm`` at which the reference clips."""
    n, nb = norm_ref(ref, bound, L)
    c = coef_ref(n, max_norm)
    assert c < 1.0 and nb < 0.01 * n, "clip_ref is derived for a clipping step whose norm is known to well under a percent"
    cb = c * (nb / (n + 1e-6) + 4.0 * V)
    out, ob = {}, {}
    for k in grad_names(L):
        g = np.asarray(ref[k], F64)
        e = np.zeros_like(g) if bound is None else np.asarray(bound[k], F64)
        out[k] = c * g
        ob[k] = c * e + (np.abs(g) + e) * cb + V * c * np.abs(g)
    return c, cb, out, ob


# ---- the device's summation order in numpy float32 -----------------------------------------------------------------------------------

def _tree(red: np.ndarray) -> np.ndarray:
    """The LDS tree over the last axis of 256 float32 partials -> the value left in element 0."""
    red = np.array(red, F32)
    o = 128
    while o >= 1:
        red[..., :o] = red[..., :o] + red[..., o:2 * o]
        o >>= 1
    return red[..., 0]


def emulate_partials(x: np.ndarray) -> np.ndarray:
    """sumsq_kernel's 256 partial sums of squares of one tensor."""
    x = np.asarray(x, F32).ravel()
    trips = max(1, -(-x.size // STRIDE))
    padded = np.zeros(trips * STRIDE, F32)
    padded[:x.size] = x                                   # a thread past the end adds nothing; adding 0^2 is the same value
    s = np.zeros(STRIDE, F32)
    for k in range(trips):
        xs = padded[k * STRIDE:(k + 1) * STRIDE].astype(F64)
        s = (xs * xs + s.astype(F64)).astype(F32)         # fmaf(x, x, s)
    return _tree(s.reshape(256, 256))                     # [block][thread] -> [block]


def emulate_norm(tensors: Sequence[np.ndarray]) -> np.float32:
    """gnorm_finalize_kernel's norm of the tensors in ``grad_names`` order."""
    parts = np.stack([emulate_partials(t) for t in tensors])   # [2L][256]: thread i adds parts[0][i], parts[1][i], ... in order
    s = np.zeros(256, F32)
    for row in parts:
        s = s + row
    return np.sqrt(_tree(s), dtype=F32)


def clip_f64(grads: Sequence[np.ndarray], max_norm: float) -> Tuple[float, List[np.ndarray]]:
    """clip_grad_norm_ on float64 gradients -> (total norm, clipped gradients)."""
    g = [np.asarray(t, F64) for t in grads]
    n = float(np.sqrt(sum(float((t ** 2).sum()) for t in g)))
    c = coef_ref(n, max_norm)
    return n, [t * c for t in g]


# ---- 4: the averaged weights ----------------------------------------------------------------------------------------------------------

def ema_replay(shadow: np.ndarray, p_new: np.ndarray, decay: float) -> np.ndarray:
    """adam_opt_kernel's shadow update in numpy float32."""
    s, p = np.asarray(shadow, F32), np.asarray(p_new, F32)
    out = s + F32(1.0 - decay) * (p - s)
    assert out.dtype == F32
    return out
