"""What tests/test_regularizers_host.py and tests/test_gpu_regularizers.py share: a numpy Philox4x32-10, the dropout masks of
include/mmc.h ("regularisers"), the mixed rows and mixed loss, and a float64 restatement of ONE trainer step with given masks and
mixed targets that returns ``(ref, bound)`` in the manner of ``oracle/mlp_step_ref.py``.  Not a test module.

The error model is that module's (items 2-6, v = 2**-24), with these additions:

* **Mask multiply, forward.**  ``H = relu(z) * scale`` where kept: ``scale = (float)(1 / (1 - p))`` is rounded once on the host and the
  product once in the epilogue, so a kept element carries ``scale * bound(relu(z)) + 2 v |H|``; a dropped one is an exact +0 on both
  sides.  Which elements are kept is a function of integers alone: exact.  The margin condition is that of the unmasked pre-activation.
* **Mask multiply, dZ epilogue.**  ``dZ(l) = (dZ(l+1) W(l)) * scale`` where ``H(l) > 0``: the same two roundings on top of the scaled
  bound of the product; ``H(l) > 0`` is "alive and kept", which the margin condition and the exact mask make the reference's.
* **Input mask.**  ``X * scale`` where kept: ``2 v |X scale|`` on the first layer's input.
* **Mixed loss.**  With ``la = lam``, ``lb = 1.0f - lam`` (the device's own fp32 scalars: exact) the value is
  ``g (la dl(ya) + lb dl(yb))`` with ``loss_checker.checker``'s unnormalised terms and ``g = 1 / sum_i (la w[ya_i] + lb w[yb_i])``.  Each
  target's term carries ``loss_checker.bounds`` at the mixed ``g``; the combination adds two products and one sum: 3 v of the
  magnitudes.  So ``bound(dlogits) = (la + lb) 128 v g w_max + 3 v g (la |dl(ya)| + lb |dl(yb)|)`` and alike for ``row_loss``.
* **Label smoothing in a full step.**  The logits' bound e passes through the smoothed loss as
  ``g A p_c (e_c + sum_j p_j e_j)`` on ``dlogits`` with ``A = (1 - eps) w_t + (eps / K) W`` (the Jacobian of both terms is
  ``p_c (delta_cj - p_j)`` times their weight), and as ``g [(1 - eps) w_t (e_t + pe) + (eps / K) (W pe + sum_j w_j e_j)]`` on ``row_loss``.
  Focal modulation and a logit prior are held per element at the loss stage alone (``mixed_loss``), not through a full step.
"""

import math

import numpy as np

import loss_checker as lc
from oracle import mlp_step_ref as sr

V, F32, F64 = sr.V, np.float32, np.float64
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 of ``counter`` (..., 4) and ``key`` (2,) -> (..., 4) uint32.  Vectorised over the leading dimensions."""
    c = np.asarray(counter, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(key[0]) & _MASK, int(key[1]) & _MASK
    mask = np.uint64(_MASK)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2          # < 2^64: exact in uint64
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c1, c3, c0, c2 = p1 & mask, p0 & mask, n0, n2
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def thresh(p: float) -> int:
    return int(math.floor(float(p) * 2.0 ** 32))


def keep_mask(seed: int, step: int, site: int, M: int, N: int, p: float, width=None) -> np.ndarray:
    """keep[m][n] of site ``site`` at step ``step``: word 0 of Philox((lo e, hi e, lo step, site), (lo seed, hi seed)) >= thresh(p), with
    e = m N + n.  ``width`` replaces N in e (the padded-width fault)."""
    W = N if width is None else width
    e = (np.arange(M, dtype=np.uint64)[:, None] * np.uint64(W) + np.arange(N, dtype=np.uint64)[None, :])
    ctr = np.stack([e & np.uint64(_MASK), e >> np.uint64(32), np.full_like(e, step & _MASK), np.full_like(e, site)], axis=-1)
    x0 = philox4x32_10(ctr, (seed & _MASK, (seed >> 32) & _MASK))[..., 0]
    return x0 >= np.uint32(thresh(p)) if thresh(p) else np.ones((M, N), bool)


def scale32(p: float) -> np.float32:
    return F32(1.0 / (1.0 - float(p)))


def step_masks(seed, step, dims, mb, p_input, p_hidden, width=None):
    """The masks of one step -> a list of ``len(dims) - 1`` entries, entry s for site s: ``(keep, p)`` or None when that site does not
    drop (the logits are no site)."""
    out = []
    for s in range(len(dims) - 1):
        p = p_hidden if s else p_input
        pad = None if width is None else width(dims[s])
        out.append((keep_mask(seed, step, s, mb, dims[s], p, pad), p) if thresh(p) else None)
    return out


def dropped_input(X, keep, p):
    """``X * scale`` where kept, +0 elsewhere, as the device forms it: one fp32 multiply."""
    return np.where(keep, np.asarray(X, F32) * scale32(p), F32(0)).astype(F32)


def mix_rows(X, a, b, lam) -> np.ndarray:
    """``lam X[a] + oml X[b]`` in fp32: two rounded products and one rounded add, ``oml = 1.0f - lam``; ``lam`` per row or scalar."""
    la = np.asarray(lam, F32).reshape(-1, 1) if np.ndim(lam) else F32(lam)
    lb = F32(1.0) - la
    out = la * np.asarray(X, F32)[a] + lb * np.asarray(X, F32)[b]
    assert out.dtype == F32
    return out


def _lams(lam):
    la = F32(lam)
    return float(la), float(F32(1.0) - la)


def mixed_weight_sum(ya, yb, lam, w) -> float:
    la, lb = _lams(lam)
    s = 0.0
    for a, b in zip(np.asarray(ya).tolist(), np.asarray(yb).tolist()):
        s += la * (1.0 if w is None else float(w[a])) + lb * (1.0 if w is None else float(w[b]))
    return s


def mixed_loss(z, ya, yb, lam, w=None, prior=None, eps=0.0, gamma=0.0):
    """-> (dlogits fp64, row_loss fp64, bound on dlogits, bound on row_loss) of the mixed loss stage on the fp32 logits ``z``."""
    la, lb = _lams(lam)
    ya, yb = np.asarray(ya, np.int64), np.asarray(yb, np.int64)
    g = 1.0 / mixed_weight_sum(ya, yb, lam, w)
    parts = []
    for y in (ya, yb):
        grad, rows, _, _ = lc.checker(z, y, w, prior, eps, gamma)
        own = lc.weight_sum(y, w)                                   # checker normalised by its own weight sum: undo it
        parts.append((grad * own, rows * own))
    (da, ra), (db, rb) = parts
    wmax = 1.0 if w is None else float(np.max(w))
    grad = g * (la * da + lb * db)
    rows = g * (la * ra + lb * rb)
    bd = (la + lb) * lc.DLOGITS_UNITS * V * g * wmax + 3.0 * V * g * (la * np.abs(da) + lb * np.abs(db))
    bl = lc.ROW_LOSS_UNITS * V * g * (la * (np.abs(ra) + wmax) + lb * (np.abs(rb) + wmax)) + 3.0 * V * g * (la * np.abs(ra) + lb * np.abs(rb))
    return grad, rows, bd, bl


def step(weights, biases, X, y, alpha, class_weight=None, masks=None, y2=None, lam=None, eps=0.0):
    """``mlp_step_ref.step_ref`` with dropout masks, mixed targets and label smoothing -> (ref, bound).

    ``X``: the fp32 rows the first layer (or the input mask) reads -- for a mixed step the rows ``mix_rows`` made.  ``masks``:
    ``step_masks``' list or None.  ``y2`` / ``lam``: the partner labels and the mini-batch's lam of a mixed step.  With no mask, no
    mixing and ``eps = 0`` every operation is ``step_ref``'s, in its order: the same values."""
    W = [np.asarray(w, F32).astype(F64) for w in weights]
    b = [np.asarray(v, F32).astype(F64) for v in biases]
    cw = None if class_weight is None else np.asarray(class_weight, F32)
    y = np.asarray(y, np.int64)
    L, mb = len(W), int(np.shape(X)[0])
    masks = [None] * L if masks is None else list(masks)
    assert len(masks) == L
    mult = [None if m is None else np.where(m[0], 1.0 / (1.0 - float(m[1])), 0.0) for m in masks]
    h = np.asarray(X, F32).astype(F64)
    eh = np.zeros_like(h)
    if mult[0] is not None:
        h = h * mult[0]
        eh = 2.0 * V * np.abs(h)
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
            raise sr.MarginError(f"layer {l}: {int(bad.sum())} of {z.size} pre-activations within 2 x bound of 0")
        h, eh = np.maximum(z, 0.0), np.where(z > 0.0, ez, 0.0)
        if mult[l + 1] is not None:
            h = h * mult[l + 1]
            eh = eh * mult[l + 1] + 2.0 * V * np.abs(h)
        hs.append(h)
        ehs.append(eh)
    ref, bound = {"logits": z}, {"logits": ez}

    mixed = y2 is not None
    W_tot = float(z.shape[1]) if cw is None else float(sum(float(v) for v in cw))
    eps_k = eps / z.shape[1]

    def coef(t):
        wt = np.ones(mb) if cw is None else cw[t].astype(F64)
        return (1.0 - eps) * wt if eps else wt

    if mixed:
        la, lb = _lams(lam)
        y2 = np.asarray(y2, np.int64)
        grad, rows, bd, bl = mixed_loss(z, y, y2, lam, cw, eps=eps)
        g = 1.0 / mixed_weight_sum(y, y2, lam, cw)
        targets = [(la, y), (lb, y2)]
    else:
        grad, rows, _, _ = lc.checker(z, y, cw, eps=eps)
        bd, bl = lc.bounds(y, cw, rows)
        g = 1.0 / lc.weight_sum(y, cw)
        targets = [(None, y)]
    zs = z - z.max(axis=1, keepdims=True)
    p = np.exp(zs) / np.exp(zs).sum(axis=1, keepdims=True)
    pe = (p * ez).sum(axis=1)
    if mixed:
        A = sum(f * coef(t) for f, t in targets)
        hit = sum(f * coef(t) * (ez[np.arange(mb), t] + pe) for f, t in targets)
    else:
        A = coef(y)
        hit = None
    if eps:
        A = A + eps_k * W_tot
    edz = bd + g * A[:, None] * p * (ez + pe[:, None])
    if mixed:
        erl = bl + g * hit
    else:
        erl = bl + g * coef(y) * (ez[np.arange(mb), y] + pe)
    if eps:
        wj = np.ones(z.shape[1]) if cw is None else cw.astype(F64)
        erl = erl + g * eps_k * (W_tot * pe + (ez * wj[None, :]).sum(axis=1))

    reg = 0.5 * alpha / mb * sum(float((w ** 2).sum()) for w in W)
    trips = max(-(-w.size // sr.SUMSQ_STRIDE) for w in W)
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
            if masks[l] is not None:
                sc = 1.0 / (1.0 - float(masks[l][1]))
                dz = dz * sc
                edz = edz * sc + 2.0 * V * np.abs(dz)
    return ref, bound


def emulate_step(weights, biases, X, y, alpha, class_weight=None, masks=None, y2=None, lam=None, eps=0.0, fault=None):
    """One step in numpy fp32 (BLAS products: another summation order than the device's) -> {name: tensor} as ``step`` names them.
    ``fault``: "mask ignored in backward", "scale missing" or "oml on the wrong target" -- three of the wrong steps the bounds have
    to catch (the other two are wrong masks, which the caller builds)."""
    ws = [np.asarray(w, F32) for w in weights]
    bs = [np.asarray(v, F32) for v in biases]
    cw = None if class_weight is None else np.asarray(class_weight, F32)
    y = np.asarray(y, np.int64)
    L, mb = len(ws), int(np.shape(X)[0])
    masks = [None] * L if masks is None else list(masks)

    def sc(m):
        return F32(1.0) if fault == "scale missing" else scale32(m[1])

    h = np.asarray(X, F32)
    if masks[0] is not None:
        h = np.where(masks[0][0], h * sc(masks[0]), F32(0))
    hs, alive = [h], [None]
    for l in range(L):
        z = hs[-1] @ ws[l].T + bs[l]
        if l == L - 1:
            break
        h = np.maximum(z, F32(0))
        alive.append(h > 0)
        if masks[l + 1] is not None:
            h = np.where(masks[l + 1][0], h * sc(masks[l + 1]), F32(0))
        hs.append(h)
    if y2 is None:
        dz, rows = lc.emulate(z, y, cw, eps=eps)
    else:
        la = F32(lam)
        lb = F32(1.0) - la
        if fault == "oml on the wrong target":
            la, lb = lb, la
        y2 = np.asarray(y2, np.int64)
        parts = []
        for t in (y, y2):
            d, r = lc.emulate(z, t, cw, eps=eps)
            own = F32(lc.weight_sum(t, cw))                          # the emulation normalised by its own weight sum: undo it
            parts.append((d * own, r * own))
        g = F32(1.0 / mixed_weight_sum(y, y2, lam, cw))
        dz = g * (la * parts[0][0] + lb * parts[1][0])
        rows = (la * parts[0][1] + lb * parts[1][1]) * g
    out = {"logits": z}
    reg = F32(0.5 * alpha / mb) * sum(F32((w * w).sum(dtype=F32)) for w in ws)
    out["loss"] = np.asarray(F32(rows.sum(dtype=F32) + reg))
    for l in range(L - 1, -1, -1):
        out[f"gW{l}"] = dz.T @ hs[l] + F32(alpha / mb) * ws[l]
        out[f"gb{l}"] = dz.sum(axis=0, dtype=F32)
        if l > 0:
            live = alive[l] if fault == "mask ignored in backward" else hs[l] > 0
            dz = (dz @ ws[l]) * live
            if masks[l] is not None:
                dz = dz * sc(masks[l])
    for v in out.values():
        assert v.dtype == F32
    return out


# ---- the cases both test files run ---------------------------------------------------------------------------------------------
# Shapes: the smallest that cross a 64-wide tile with a ragged edge in every launch -- widths 70, 65, 130, 132, K = 5 and 108,
# mini-batches of 67 rows.  Every seed satisfies the margin condition (tests/test_regularizers_host.py checks it on the CPU).

MB = 67
MASK_SEED = 0x9E3779B97F4A7C15          # both key words in use
ALPHA = sr.ALPHA


class DropCase:
    def __init__(self, dims, p, weighted, eps, step0, seed):
        self.dims, self.p, self.weighted, self.eps, self.step0, self.seed = tuple(dims), p, weighted, eps, step0, seed

    @property
    def id(self):
        return f"L{len(self.dims) - 1}-p{self.p:g}-" + ("weights" if self.weighted else f"smooth{self.eps:g}") + f"-t{self.step0}"


_D2, _D3 = (70, 130, 5), (132, 65, 130, 108)
DROP_CASES = [DropCase(d, p, weighted, 0.0 if weighted else 0.1, step0, seed)
              for d, p, weighted, step0, seed in ((_D2, 0.1, True, 0, 1), (_D2, 0.1, False, 3, 2), (_D2, 0.5, True, 3, 1), (_D2, 0.5, False, 0, 2),
                                                  (_D3, 0.1, True, 3, 32), (_D3, 0.1, False, 0, 87), (_D3, 0.5, True, 0, 4), (_D3, 0.5, False, 3, 78))]


def make_drop_case(c: DropCase):
    """-> (weights, biases, class weights or None, X, y, masks) of a hidden-dropout case: one mini-batch of MB rows at step ``c.step0``."""
    rng = np.random.default_rng([c.seed, len(c.dims), int(c.p * 10), int(c.weighted)])
    ws, bs = sr.make_params(rng, c.dims)
    cw = sr.make_weights(rng, c.dims[-1]) if c.weighted else None
    X, y = sr.make_rows(rng, MB, c.dims[0], c.dims[-1], cw)
    return ws, bs, cw, X, y, step_masks(MASK_SEED, c.step0, c.dims, MB, 0.0, c.p)


MIXED_SEED = 3


def mixed_step_case():
    """One mixed step over a set of 100 rows, dims (70, 130, 65, 5), class weights, hidden dropout 0.25 at step 1
    -> (weights, biases, class weights, X, y, visit, partner, lam, masks): position i mixes rows visit[i] and partner[i]."""
    dims = (70, 130, 65, 5)
    rng = np.random.default_rng([MIXED_SEED, 7])
    ws, bs = sr.make_params(rng, dims)
    cw = sr.make_weights(rng, dims[-1])
    X, y = sr.make_rows(rng, 100, dims[0], dims[-1])
    visit = rng.permutation(100)[:MB].astype(np.int64)
    partner = visit[rng.permutation(MB)]
    lam = np.asarray([0.3], F32)
    return ws, bs, cw, X, y, visit, partner, lam, step_masks(MASK_SEED, 1, dims, MB, 0.0, 0.25)
