"""What tests/test_feature_transform_host.py and tests/test_gpu_feature_transform.py share: a float64 (long double for the moments)
numpy evaluation of the "feature transforms" definition of include/mmc.h, the per-element bounds derived from it, and an honest
numpy emulation of csrc/features.hip's scatter kernel with its classic bugs switchable.  Not a test module.

The checker takes the DEVICE's own fp32 centres, so the centred operands fl32(x - c) are replicated bit for bit (one IEEE fp32
subtraction) and the bounds hold accumulation error only.

Bounds (u24 = 2^-24, u53 = 2^-53; gamma_k = k u24 / (1 - k u24), Higham's bound for a chain of k fp32 fused multiply-adds):
  moments  mean: the fp64 sum of n_g terms, however it is bracketed, is off by at most (n_g - 1) u53 sum|x| to first order, the division
           adds one rounding: |mean - ref| <= 2 n_g u53 sum|x| / n_g.
           m2: d = fl(x - mean) and fma(d, d, acc) put at most n_g + 2 roundings on a term: <= 2 n_g u53 sum (x - mu)^2 for n_g >= 2
           (n_g = 1 is exact: d = 0).  The device's deviations are taken from ITS mean; about a mean that is off by at most e (the
           mean bound) the exact sum of squares is larger by exactly n_g (mean - mu)^2 <= n_g e^2 -- the cross term is a multiple of
           sum (x - mu) = 0 -- which is the term for the mean's own error.
  scatter  an element is, per chunk of R = 256 rows, one fp32 fmaf chain: <= gamma_R sum_rows |xc_j||xc_k| summed over the chunks;
           the fp64 adds of at most n / R + 16 chunk values: <= n u53 of the same sum.  Rigorous, so the gate is 1 x.
  transform one fp32 fmaf chain over dim: <= gamma_dim sum_j |xc_j||T_kj|.
"""

import numpy as np

U24, U53 = 2.0 ** -24, 2.0 ** -53
CHUNK, MAX_SPLITS, TILE = 256, 16, 128   # include/mmc.h: MMC_SCATTER_CHUNK_ROWS, MMC_SCATTER_MAX_SPLITS; features.hip: kST


def gamma(k):
    return k * U24 / (1.0 - k * U24)


# ---- moments ----------------------------------------------------------------------------------------------------------------------
def moments(X, yi, K):
    """-> counts (K,) int64; mean, m2, mean_bound, m2_bound ((K + 1), dim), the first two in long double (slot K: every row)."""
    X = np.asarray(X, np.float32).astype(np.longdouble)
    yi = np.asarray(yi)
    dim = X.shape[1]
    counts = np.bincount(yi, minlength=K).astype(np.int64)
    mean = np.zeros((K + 1, dim), np.longdouble)
    m2 = np.zeros_like(mean)
    mean_bound = np.zeros((K + 1, dim), np.float64)
    m2_bound = np.zeros_like(mean_bound)
    for g in range(K + 1):
        rows = X if g == K else X[yi == g]
        n_g = len(rows)
        if n_g == 0:
            continue
        mean[g] = rows.sum(axis=0) / n_g
        dev = rows - mean[g]
        m2[g] = (dev * dev).sum(axis=0)
        e = 2 * n_g * U53 * np.abs(rows).sum(axis=0).astype(np.float64) / n_g
        mean_bound[g] = e
        m2_bound[g] = 2 * n_g * U53 * m2[g].astype(np.float64) + n_g * e * e
    return counts, mean, m2, mean_bound, m2_bound


# ---- scatter ----------------------------------------------------------------------------------------------------------------------
def centred(X, centres32, yi=None):
    """fl32(x - c) bit for bit: ``centres32`` (dim,) float32, or (K, dim) float32 indexed by the row's label ``yi``."""
    X = np.asarray(X, np.float32)
    c = np.asarray(centres32)
    assert c.dtype == np.float32
    return X - (c if c.ndim == 1 else c[np.asarray(yi)])


def scatter(Xc):
    """-> (S, bound): the float64 scatter of the replicated operands and the per-element bound of the device's arithmetic."""
    A = np.asarray(Xc, np.float32).astype(np.float64)
    n = A.shape[0]
    S = A.T @ A
    absum = np.abs(A).T @ np.abs(A)
    return S, (gamma(CHUNK) + n * U53) * absum


def scatter_splits(n, dim):
    chunks = -(-n // CHUNK)
    tiles = -(-dim // TILE)
    return max(1, min(MAX_SPLITS, 512 // (tiles * (tiles + 1) // 2), chunks))


def _chain32(A, B):
    """sum_k A[k, :, None] * B[k, None, :] as one fp32 fused-multiply-add chain in k order: the fp32 x fp32 product is exact in
    float64, so each step rounds once to float64 (53 bits, far below the fp32 ulp) and once to fp32."""
    acc = np.zeros((A.shape[1], B.shape[1]), np.float32)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    for k in range(A.shape[0]):
        acc = (acc.astype(np.float64) + A64[k][:, None] * B64[k][None, :]).astype(np.float32)
    return acc


def emulate_scatter(X, centres32, yi=None, bug=None):
    """csrc/features.hip's scatter in numpy: tile pairs tile_m <= tile_n, contiguous chunk ranges, fp32 chains of 256 rows folded
    into float64, the ranges added in ascending order, the triangle mirrored.  ``bug`` restates one wrong kernel:
    ``drop_last_chunk`` (a ragged last chunk is never staged), ``centre_after_pad`` (the rows that pad the last 16-row stage are
    zero BEFORE centring), ``neighbour_centre`` (class y + 1's centre), ``no_mirror`` (the lower block of an off-diagonal tile pair
    stays zero), ``split_twice`` (the second range's partial is added twice), ``no_clear`` (the fp32 accumulator is not cleared
    at a chunk's end)."""
    X = np.asarray(X, np.float32)
    n, dim = X.shape
    c = np.asarray(centres32, np.float32)
    if bug == "neighbour_centre":
        yi = (np.asarray(yi) + 1) % c.shape[0]
    Xc = centred(X, c, yi)
    if bug == "centre_after_pad" and n % 16:
        pad = np.zeros((16 - n % 16, dim), np.float32) - (c if c.ndim == 1 else c[np.asarray(yi)[-1]])
        Xc = np.concatenate([Xc, pad])
    chunks = -(-n // CHUNK)
    S = scatter_splits(n, dim)
    tiles = -(-dim // TILE)
    out = np.zeros((dim, dim), np.float64)
    for tm in range(tiles):
        for tn in range(tm, tiles):
            ms, ns = slice(tm * TILE, min(dim, (tm + 1) * TILE)), slice(tn * TILE, min(dim, (tn + 1) * TILE))
            total = np.zeros((ms.stop - ms.start, ns.stop - ns.start), np.float64)
            for s in range(S):
                part = np.zeros_like(total)
                acc = np.zeros(total.shape, np.float32)
                for ch in range(s * chunks // S, (s + 1) * chunks // S):
                    rows = Xc[ch * CHUNK:(ch + 1) * CHUNK]
                    if bug == "drop_last_chunk" and ch == chunks - 1 and n % CHUNK:
                        continue
                    if bug == "no_clear":
                        acc = (acc.astype(np.float64) + _chain32(rows[:, ms], rows[:, ns]).astype(np.float64)).astype(np.float32)
                        part += acc.astype(np.float64)
                    else:
                        part += _chain32(rows[:, ms], rows[:, ns]).astype(np.float64)
                total += part
                if bug == "split_twice" and s == 1:
                    total += part
            if tm == tn:
                total = np.triu(total) + np.triu(total, 1).T
            out[ms, ns] = total
            if tm != tn and bug != "no_mirror":
                out[ns, ms] = total.T
    return out


# ---- transform --------------------------------------------------------------------------------------------------------------------
def transform(Xc, T32):
    """-> (Y, bound): the float64 product of the replicated operands with T (m, dim) float32, and gamma_dim sum_j |xc_j||T_kj|."""
    A = np.asarray(Xc, np.float32).astype(np.float64)
    T = np.asarray(T32, np.float32).astype(np.float64)
    return A @ T.T, gamma(A.shape[1]) * (np.abs(A) @ np.abs(T).T)


def emulate_transform(Xc, T32):
    return _chain32(np.ascontiguousarray(np.asarray(Xc, np.float32).T), np.ascontiguousarray(np.asarray(T32, np.float32).T))


# ---- the calibrated head in float64 -----------------------------------------------------------------------------------------------
def head_f64(X, weights, biases, a, b):
    """The calibrated head's formula (calibration.build_head_module) in float64 on the parameters as given."""
    x = np.asarray(X, np.float64)
    for i, (w, v) in enumerate(zip(weights, biases)):
        if i:
            x = np.maximum(x, 0.0)
        x = x @ np.asarray(w, np.float64).T + np.asarray(v, np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    q = 1.0 / (1.0 + np.exp(np.asarray(a, np.float64) * p + np.asarray(b, np.float64)))
    total = q.sum(axis=1, keepdims=True)
    return np.where(total > 0, q / np.where(total > 0, total, 1.0), 1.0 / q.shape[1])


def reef_like(n, dim, K, seed, rank=None):
    """Seeded correlated non-negative features with column means of several standard deviations (what pooled post-SiLU
    activations look like) and labels; class ``K - 1`` shifts a few columns."""
    rng = np.random.default_rng(seed)
    r = rank or max(2, dim // 4)
    mix = rng.normal(0, 1, (r, dim))
    base = rng.uniform(3.0, 9.0, dim)
    yi = rng.integers(0, K, n)
    shift = rng.normal(0, 0.7, (K, dim))
    X = base + shift[yi] + 0.6 * rng.normal(0, 1, (n, r)) @ mix / np.sqrt(r) + 0.3 * rng.normal(0, 1, (n, dim))
    return np.maximum(X, 0.0).astype(np.float32), yi.astype(np.int64)
