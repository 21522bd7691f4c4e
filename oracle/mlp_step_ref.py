"""Float64 reference of ONE step of the MLP trainer (``csrc/trainer.hip``): value AND per-element error bound.

TEST INFRASTRUCTURE ONLY (like the rest of ``oracle/``): only ``tests/`` imports this module.

``step_ref`` takes what the device gets -- the fp32 parameters, the class weights or none, alpha and the mini-batch ``(X, y)``, the
loss options at their plain defaults -- promotes it to float64 and returns ``(ref, bound)``, two dicts of arrays with the keys
``logits``, ``loss``, ``gW0..``, ``gb0..``.  ``bound`` is a first-order forward error bound of an fp32 evaluation, carried next to
the value through the same products run on ``|W|``, ``|H|`` and ``|dZ|``.  With ``v = 2**-24`` (fp32 unit roundoff) the model is
(line numbers: ``mermaid_classifier_amd/csrc/trainer.hip``):

1. **Inputs.**  Parameters, class weights, rows and labels are the device's own fp32 values: exact.
2. **Dot products.**  A K-term dot product accumulated in fp32 in any order, fused or not (``v_mfma_f32_16x16x4_f32``, ``:97``; the
   zero padding of a ragged tile, ``:73-82``, adds exact zeros), followed by its epilogue carries
   <= (K + c) v (sum|a b| + |aux term|) on top of what its inputs carry, which passes through ``|W|`` / ``|H|`` / ``|dZ|``:
   - forward, ``aux = b[n]``, c = 1: the one addition ``v + aux[n]`` (``:111-112``); ``fmaxf`` is exact;
   - dW, ``aux = (alpha / mb) W``, c = 2: the scalar ``(float)(alpha / mb)`` is rounded once on the host (``:713``) and
     ``fmaf(scale, aux, v)`` rounds once (``:114``);
   - dZ, no aux term, c = 0: the mask selects ``v`` or an exact 0 (``:113``).
3. **ReLU.**  1-Lipschitz: errors pass unchanged where the pre-activation is positive, and where it is negative the value is an
   exact 0 on both sides.  That, and the mask ``H > 0`` of the dZ epilogue (``:113``), need the sign of every hidden
   pre-activation to be the reference's: the **margin condition** ``|z| > 2 bound(z)``, or ``z == 0`` with ``bound(z) == 0`` (a unit
   whose weights and bias are all zero is an exact 0 everywhere).  ``step_ref`` raises ``MarginError`` for an input that violates it;
   nothing is ever excluded from a comparison.
4. **Loss stage** (``ce_grad_rows<false>``, ``:232-248``).  On its own input it carries the bounds ``tests/loss_checker.py`` derives
   (``bounds``: 128 v g w_max on ``dlogits``, 96 v (|l_i g| + g w_max) on ``row_loss``; they include ``inv_wsum``, the float of a double
   quotient, ``:827`` / ``:975``).  Its input carries the logits' bound e, which the softmax passes on to first order as
   ``g w_t p_c (e_c + sum_j p_j e_j)`` on ``dlogits[c]`` and ``g w_t (e_t + sum_j p_j e_j)`` on ``row_loss``.  The value is the
   checker's own (``loss_checker.checker`` on the float64 logits): it is reused, not restated.
5. **Column sums** (``colsum_cols``, ``:278-287``).  M values in four chains and a two-level tree: every value passes through at most
   M - 1 additions whatever the order, so <= M v sum|dZ| (c = 0) plus the sum of the inputs' bounds.
6. **Loss sum** (``sumsq_slice`` ``:309-316``, ``loss_finalize_one`` ``:339-348``).  data + reg with
   - data = sum of ``row_loss``: a per-thread chain of ceil(M / 256) <= M additions, the ``fmaf`` that joins the two sums and the
     eight levels of the LDS tree: (M + 9) v sum|row_loss| plus the rows' bounds;
   - reg = (0.5 alpha / mb) sum_l sum W_l^2: per thread T = ceil(n_l / 65536) fused multiply-adds of the grid-stride loop (``:309``) and
     eight tree levels (``:312-315``) in a partial, then L partials per thread (``:341``), the scalar's rounding (``:701``), the
     ``fmaf`` (``:342``) and eight tree levels (``:344-347``): (T + L + 18) v reg, all terms being non-negative.
7. **Adam** (``adam_elems``, ``:369-384``).  Not bounded but reproduced: ``adam_f32`` is the kernel's written order in numpy fp32
   (two roundings each in ``m`` and ``v``, ``(om_beta2 g) g``, scalars made from doubles as ``:727-729`` / ``:739`` make them), which
   the device must match bit for bit; ``adam_param_ref`` bounds the parameter update (see there).

The comparison that uses these bounds (``tests/test_gpu_trainer_step.py``) allows 2 x bound per element: the factor covers the
second-order terms this first-order model drops.  ``tests/test_trainer_step_ref.py`` proves on the CPU that the numpy fp32 oracle
(another summation order) stays within 1 x bound and that wrong kernels exceed 2 x bound.
"""

from __future__ import annotations

import sys
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

V = 2.0 ** -24      # fp32 unit roundoff
F32, F64 = np.float32, np.float64
SUMSQ_STRIDE = 256 * 256    # elements one trip of sumsq_kernel's grid-stride loop covers (256 blocks of 256 threads)


class MarginError(ValueError):
    """A hidden pre-activation of the reference is too close to 0 for the device's ReLU mask to be known."""


def _loss_checker():
    try:
        import loss_checker
    except ImportError:
        sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
        import loss_checker
    return loss_checker


def launch_of(name: str, n_layers: int) -> str:
    """The launch of ``trainer_group_step`` that wrote the tensor ``name`` of ``step_ref``'s result."""
    if name == "logits":
        return f"tgemm_f32_kernel<TA=0,TB=1> EPI_BIAS, forward layer {n_layers - 1}"
    if name == "loss":
        return "loss_finalize_kernel (after ce_grad_kernel and sumsq_kernel)"
    l = int(name[2:])
    return f"tgemm_f32_kernel<TA=1,TB=0> EPI_L2, layer {l}" if name.startswith("gW") else f"colsum_kernel, layer {l}"


def step_ref(weights: Sequence[np.ndarray], biases: Sequence[np.ndarray], X: np.ndarray, y: np.ndarray, alpha: float,
             class_weight: Optional[np.ndarray] = None) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
    """-> (ref, bound): float64 value and first-order fp32 error bound of ``logits`` [mb][K], ``loss`` (0-d), ``gW{l}``, ``gb{l}``
    of the step on the mini-batch ``(X, y)`` at these parameters.  Raises ``MarginError`` (rule 3)."""
    lc = _loss_checker()
    W = [np.asarray(w, F32).astype(F64) for w in weights]
    b = [np.asarray(v, F32).astype(F64) for v in biases]
    cw = None if class_weight is None else np.asarray(class_weight, F32)
    y = np.asarray(y, np.int64)
    L, mb = len(W), int(np.shape(X)[0])
    h = np.asarray(X, F32).astype(F64)
    eh = np.zeros_like(h)
    hs, ehs = [h], [eh]
    for l in range(L):
        K = W[l].shape[1]
        aw = np.abs(W[l]).T
        z = h @ W[l].T + b[l]
        mag = np.abs(h) @ aw
        ez = eh @ aw + (K + 1) * V * (mag + np.abs(b[l]))
        if l == L - 1:
            break
        bad = ~((np.abs(z) > 2.0 * ez) | ((z == 0.0) & (ez == 0.0)))
        if bad.any():
            i = np.unravel_index(int(np.argmax(np.where(bad, ez / np.maximum(np.abs(z), 1e-300), 0.0))), z.shape)
            raise MarginError(f"layer {l}: {int(bad.sum())} of {z.size} pre-activations within 2 x bound of 0; the closest, at "
                              f"{tuple(int(v) for v in i)}: z {z[i]:.3g}, bound {ez[i]:.3g}")
        h, eh = np.maximum(z, 0.0), np.where(z > 0.0, ez, 0.0)
        hs.append(h)
        ehs.append(eh)
    ref, bound = {"logits": z}, {"logits": ez}

    # rule 4: the checker's value and bounds, plus the softmax's sensitivity to the logits' bound
    grad, rows, _, _ = lc.checker(z, y, cw)
    bd, bl = lc.bounds(y, cw, rows)
    g = 1.0 / lc.weight_sum(y, cw)
    wt = np.ones(mb) if cw is None else cw[y].astype(F64)
    zs = z - z.max(axis=1, keepdims=True)
    p = np.exp(zs) / np.exp(zs).sum(axis=1, keepdims=True)
    pe = (p * ez).sum(axis=1)
    edz = bd + g * wt[:, None] * p * (ez + pe[:, None])
    erl = bl + g * wt * (ez[np.arange(mb), y] + pe)

    # rule 6
    reg = 0.5 * alpha / mb * sum(float((w ** 2).sum()) for w in W)
    trips = max(-(-w.size // SUMSQ_STRIDE) for w in W)
    ref["loss"] = np.asarray(rows.sum() + reg)
    bound["loss"] = np.asarray(erl.sum() + (mb + 9) * V * np.abs(rows).sum() + (trips + L + 18) * V * reg)

    dz = grad
    for l in range(L - 1, -1, -1):
        h, eh = hs[l], ehs[l]
        aux = alpha / mb * W[l]
        adz = np.abs(dz)
        ref[f"gW{l}"] = dz.T @ h + aux
        bound[f"gW{l}"] = edz.T @ np.abs(h) + adz.T @ eh + (mb + 2) * V * (adz.T @ np.abs(h) + np.abs(aux))
        ref[f"gb{l}"] = dz.sum(axis=0)
        bound[f"gb{l}"] = edz.sum(axis=0) + mb * V * adz.sum(axis=0)
        if l > 0:
            live = hs[l] > 0.0
            no = W[l].shape[0]
            edz = np.where(live, edz @ np.abs(W[l]) + no * V * (adz @ np.abs(W[l])), 0.0)
            dz = np.where(live, dz @ W[l], 0.0)
    return ref, bound


def worst_ratio(got, ref, bound) -> Tuple[float, Tuple[int, ...]]:
    """(max |got - ref| / bound, its index); an element whose bound is 0 must be equal (ratio inf otherwise)."""
    diff = np.abs(np.asarray(got, F64) - ref)
    r = np.where(bound > 0, diff / np.maximum(bound, 1e-300), np.where(diff > 0, np.inf, 0.0))
    idx = np.unravel_index(int(np.argmax(r)), r.shape) if r.ndim else ()
    return float(r[idx]), tuple(int(v) for v in idx)


def exceed_report(name: str, n_layers: int, got, ref, bound, factor: float = 2.0) -> Optional[str]:
    """None when |got - ref| <= factor * bound on every element; otherwise the worst element and the launch that wrote it."""
    got = np.asarray(got, F64)
    over = np.abs(got - ref) > factor * bound
    if not over.any():
        return None
    ratio, idx = worst_ratio(got, ref, bound)
    return (f"{name} [{launch_of(name, n_layers)}]: worst element {idx}: got {float(got[idx]):.9g} ref {float(ref[idx]):.9g} bound "
            f"{float(bound[idx]):.3g} (|got - ref| / bound = {ratio:.2f}); {int(over.sum())} of {over.size} elements over {factor:g} x bound")


# ---- rule 7: the Adam update -------------------------------------------------------------------------------------------------

class AdamScalars(NamedTuple):
    om_beta1: np.float32
    beta2: np.float32
    om_beta2: np.float32
    eps: np.float32
    step_size: np.float32
    bc2_sqrt: np.float32


def adam_scalars(t: int, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, om_beta2_in_fp32=False) -> AdamScalars:
    """The fp32 scalars of step number ``t`` (the count after the increment), each the float of a double expression.
    ``om_beta2_in_fp32`` forms ``1.0f - (float)beta2`` instead of ``(float)(1.0 - beta2)``: the mutant the bit check must catch."""
    om2 = F32(1.0) - F32(beta2) if om_beta2_in_fp32 else F32(1.0 - beta2)
    return AdamScalars(F32(1.0 - beta1), F32(beta2), om2, F32(eps), F32(lr / (1.0 - beta1 ** t)), F32(np.sqrt(1.0 - beta2 ** t)))


def adam_f32(g: np.ndarray, m: np.ndarray, v: np.ndarray, s: AdamScalars) -> Tuple[np.ndarray, np.ndarray]:
    """``adam_elems``' moments in its written order, numpy fp32 (one rounding per operator, nothing fused) -> (m', v')."""
    g, m, v = (np.asarray(a, F32) for a in (g, m, v))
    m1 = m + s.om_beta1 * (g - m)
    v1 = v * s.beta2 + s.om_beta2 * g * g
    assert m1.dtype == F32 and v1.dtype == F32
    return m1, v1


def adam_param_ref(p: np.ndarray, m1: np.ndarray, v1: np.ndarray, s: AdamScalars) -> Tuple[np.ndarray, np.ndarray]:
    """-> (ref, bound) of the updated parameter ``fmaf(-step_size, m' / (sqrtf(v') / bc2_sqrt + eps), p)`` evaluated in float64
    from the fp32 ``p``, ``m'``, ``v'`` and scalars.  With one ulp = 2 v relative: ``sqrtf`` and each of the two divisions are within
    one ulp (2 v; half that where they are correctly rounded), ``+ eps`` rounds once (v), so the quotient q carries
    2 + 2 + 1 + 2 = 7 v relative = 3.5 ulp, and the fused multiply-add rounds the result once (v = half an ulp of p'):
    |p' - ref| <= v |ref| + 7 v |step_size q|."""
    p, m1, v1 = (np.asarray(a, F32).astype(F64) for a in (p, m1, v1))
    q = m1 / (np.sqrt(v1) / F64(s.bc2_sqrt) + F64(s.eps))
    upd = F64(s.step_size) * q
    ref = p - upd
    return ref, V * np.abs(ref) + 7.0 * V * np.abs(upd)


# ---- the cases both test files run ---------------------------------------------------------------------------------------------

ALPHA = 0.5     # the L2 term of dW is then far above its bound


class Case(NamedTuple):
    dims: Tuple[int, ...]
    mb: int
    weighted: bool
    seed: int
    what: str

    @property
    def id(self) -> str:
        return "x".join(map(str, self.dims)) + f"-mb{self.mb}" + ("-w" if self.weighted else "")


def make_params(rng, dims: Sequence[int]) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """Glorot-uniform weights and small non-zero biases, fp32."""
    ws, bs = [], []
    for i, o in zip(dims[:-1], dims[1:]):
        a = np.sqrt(6.0 / (i + o))
        ws.append(rng.uniform(-a, a, (o, i)).astype(F32))
        bs.append((0.1 * rng.standard_normal(o)).astype(F32))
    return ws, bs


def make_rows(rng, n: int, dim: int, K: int, class_weight: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """``n`` Gaussian rows with uniform labels; with class weights, row 0 carries a class of non-zero weight."""
    X = rng.standard_normal((n, dim)).astype(F32)
    y = rng.integers(0, K, size=n).astype(np.int32)
    if class_weight is not None:
        y[0] = int(np.flatnonzero(class_weight > 0)[0])
    return X, y


def make_weights(rng, K: int) -> np.ndarray:
    return _loss_checker().class_weights(rng, K)


def make_case(c: Case):
    """-> (weights, biases, class weights or None, X, y) of a case, from its seed alone."""
    rng = np.random.default_rng(c.seed)
    ws, bs = make_params(rng, c.dims)
    cw = make_weights(rng, c.dims[-1]) if c.weighted else None
    X, y = make_rows(rng, c.mb, c.dims[0], c.dims[-1], cw)
    return ws, bs, cw, X, y


# every seed below satisfies the margin condition (tests/test_trainer_step_ref.py checks it on the CPU); half of the cases carry a
# class-weight vector with one zero entry
_EDGE = (67, 129, 18, 7)
CASES = [
    Case(_EDGE, 1, False, 1, "a single row: K = mb = 1 in the dW GEMM, one wave of ce_grad, colsum's tail loop alone"),
    Case(_EDGE, 5, True, 1, "K = mb below the 16-deep step and no multiple of 4; mb % 4 != 0 in colsum and ce_grad"),
    Case(_EDGE, 64, False, 1, "M = mb on the tile edge; N = 129, K = 67 one past; K = no = 18 and 7 in the dZ GEMM"),
    Case(_EDGE, 65, True, 1, "M = mb one past a tile: a second row of workgroups with one live row"),
    Case(_EDGE, 77, False, 1, "ragged in every dimension of every launch"),
    Case((64, 64, 16, 4), 64, True, 2, "every dimension exactly on a boundary"),
    Case((64, 64, 16, 4), 128, False, 2, "every dimension on a boundary, two tiles of rows"),
    Case((10, 16, 5), 50, True, 1, "the odd-width host path of mmc_trainer_partial_fit"),
    Case((67, 7), 13, False, 1, "no hidden layer: no mask GEMM, last-layer epilogue only"),
    Case((260, 260, 3), 9, True, 6, "67 600 weights: second grid-stride trip of sumsq_kernel; N = 260 > 256 in colsum; K = 3"),
]

RAGGED_SEEDS = {67: 3, 68: 2}    # feature width -> seed of ragged_pass
GROUP_SEED = 1


def ragged_pass(dim0: int):
    """A pass of 64 + 13 rows in mini-batches of 64 over dims [dim0, 129, 18, 7], class weights, a non-identity visiting order
    -> (weights, biases, class weights, X, y, order): step s of the pass sees rows ``order[64 s : 64 s + 64]``."""
    rng = np.random.default_rng([RAGGED_SEEDS[dim0], dim0])
    dims = (dim0,) + _EDGE[1:]
    ws, bs = make_params(rng, dims)
    cw = make_weights(rng, dims[-1])
    X, y = make_rows(rng, 77, dim0, dims[-1])
    live = int(np.flatnonzero(cw > 0)[0])
    order = rng.permutation(77).astype(np.int64)
    y[order[0]] = y[order[64]] = live          # both mini-batches carry weight
    return ws, bs, cw, X, y, order


def group_pass():
    """Three members of different depth and width over one set of 100 rows (dim 67, 7 classes), one step each
    -> (X, y, [(weights, biases, class weights or None, visit)])."""
    rng = np.random.default_rng([GROUP_SEED, 3])
    X, y = make_rows(rng, 100, 67, 7)
    members = []
    for dims, rows, weighted in ((_EDGE, 77, True), ((67, 7), 13, False), ((67, 300, 7), 64, True)):
        ws, bs = make_params(rng, dims)
        cw = make_weights(rng, 7) if weighted else None
        visit = rng.permutation(100)[:rows].astype(np.int64)
        if weighted and not (cw[y[visit]] > 0).any():
            raise ValueError("a member's rows carry no class weight")
        members.append((ws, bs, cw, visit))
    return X, y, members
