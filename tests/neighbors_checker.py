"""The float64 checker of mmc_featureset_knn (include/mmc.h "nearest neighbours"): reference scores with per-pair error bounds, the
order rule, the acceptance rule for a device result, and a numpy emulation of the kernel's arithmetic and of its tile / split /
merge walk with switchable classic bugs.  Not a test module.

Bounds.  u = 2^-24, gamma_n = n u / (1 - n u).  The inputs are fp32 and are taken as exact.  With A = sum_i |q_i b_i|:

DOT     the device's d is one fp32 fmaf chain over dim terms: |d^ - d| <= gamma_dim A (Higham, Accuracy and Stability, section 3.1;
        an fma chain has one rounding per term).
COSINE  s^ = fl(fl(d^ r^q) r^b) with r^ = r (1 + e), |e| <= u (the fp64 evaluation of r is within a few 2^-53 of it: covered by the
        slack below).  Four factors (1 + e_i), |e_i| <= u, multiply the value: |s^ - s| <= rq rb (gamma_dim A + gamma_4 (|d| + gamma_dim A)).
L2      s = -(sq + sb - 2 d).  s^q = sq (1 + e1), s^b = sb (1 + e2), t = fl(s^q + s^b): |t - (sq + sb)| <= gamma_2 (sq + sb); the final fma
        rounds t - 2 d^ once: |s^ - s| <= (1 + u)(2 gamma_dim A + gamma_2 (sq + sb)) + u |s|.
Slack   the float64 reference itself (a numpy matmul) is within dim 2^-52 A of the exact value; every bound adds dim 2^-50 A + 2^-45 |s|.
        Underflow is not modelled: the inputs of the tests are of order 1.
"""

from __future__ import annotations

import numpy as np

U = 2.0 ** -24
DOT, COSINE, L2 = 0, 1, 2
METRIC_NAMES = {DOT: "dot", COSINE: "cosine", L2: "l2"}
TILE, CHUNK, MAX_SPLITS, MAX_K = 128, 8192, 16, 32     # include/mmc.h: MMC_KNN_TILE_ROWS, _CHUNK_ROWS, _MAX_SPLITS, _MAX_K
BUGS = ("ties_descending", "raw_bit_keys", "padding_rows", "exclude_after", "merge_drops_short", "first_ignored", "index_absolute")


def gamma(n: int) -> float:
    return n * U / (1 - n * U)


def splits(nq: int, nb: int) -> int:
    """include/mmc.h: S = min(MMC_KNN_MAX_SPLITS, T_b, max(1, 1024 / T_q))"""
    tq = (min(nq, CHUNK) + TILE - 1) // TILE
    tb = (nb + TILE - 1) // TILE
    return max(1, min(MAX_SPLITS, tb, max(1, 1024 // tq if tq else 1)))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def clustered(n: int, dim: int, K: int, seed: int, negate_from=None, centres_seed: int = 0, noise: float = 0.35):
    """n fp32 rows with labels: a centre out of K in the positive orthant, times a per-row amplitude log-uniform in [0.3, 3], plus
    noise -- nearly every dot product of two such rows is positive, and the amplitudes spread the scores of all three metrics far
    wider than the bounds, so the float64 top-k sets are settled.  Rows from ``negate_from`` on are negated: their scores against the
    others are negative, and a zero row would beat every real one."""
    rng = np.random.default_rng(seed)
    centres = np.abs(np.random.default_rng(centres_seed).normal(0, 1, (K, dim))) + 0.5
    y = rng.integers(0, K, n).astype(np.int32)
    a = np.exp(rng.uniform(np.log(0.3), np.log(3.0), n))
    X = a[:, None] * centres[y] + noise * rng.normal(0, 1, (n, dim))
    if negate_from is not None:
        X[negate_from:] *= -1
    return np.ascontiguousarray(X.astype(np.float32)), y


def integer_rows(n: int, dim: int, seed: int, K: int = 4):
    """n fp32 rows of integers in -8 .. 8 (every fp32 chain over them is exact; equal scores are plentiful) with labels"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.integers(-8, 9, (n, dim)).astype(np.float32)), rng.integers(0, K, n).astype(np.int32)


FIRST_Q, FIRST_B, NQ_MAX, NB_MAX, TAIL = 3, 6, 129, 700, 6
NB_TWO_TILES = (2 * MAX_SPLITS) * TILE - 5    # 129 queries are 2 query tiles: S = MAX_SPLITS, and every split holds two base tiles


def bounded_inputs(dim: int, seed: int, nb_max: int = NB_MAX):
    """-> (Xq, yq, Xb, yb): a query set and a base set whose ranges under test start at FIRST_Q / FIRST_B.  Queries 64.. are negated
    (negative scores against every base row).  The base rows around the range are decoys -- copies of queries 0, 1 and 128, plain and
    times 3 -- that would head those queries' lists by every metric if a range were ignored; so are the rows of the range past a
    shorter nb.  The query rows around the range are far off."""
    rng = np.random.default_rng(seed + 7)
    noise = 0.35 if dim <= 128 else 1.5      # the bounds grow with dim: wider inputs keep the sets settled
    q, yq = clustered(NQ_MAX, dim, 4, seed, negate_from=64, noise=noise)
    b, yb = clustered(nb_max, dim, 4, seed + 1, noise=noise)
    decoys = np.concatenate([np.stack([q[i], 3 * q[i]]) for i in (0, 1, 128)])
    far = (10 * rng.normal(0, 1, (FIRST_Q + TAIL, dim))).astype(np.float32)
    Xq = np.concatenate([far[:FIRST_Q], q, far[FIRST_Q:]])
    Xb = np.concatenate([decoys[:FIRST_B], b, decoys[:TAIL]])
    yq = np.concatenate([np.zeros(FIRST_Q, np.int32), yq, np.zeros(TAIL, np.int32)])
    yb = np.concatenate([np.zeros(FIRST_B, np.int32), yb, np.zeros(TAIL, np.int32)])
    return np.ascontiguousarray(Xq), yq, np.ascontiguousarray(Xb), yb


# ---- the float64 reference --------------------------------------------------------------------------------------------------------
def reference(Q, B, metric: int):
    """fp32 rows Q (nq, dim), B (nb, dim) -> (s64, beta): the float64 score of every pair and the bound on the device's error"""
    Q64, B64 = np.asarray(Q, np.float64), np.asarray(B, np.float64)
    dim = Q64.shape[1]
    d = Q64 @ B64.T
    A = np.abs(Q64) @ np.abs(B64).T
    ssq, ssb = (Q64 * Q64).sum(1), (B64 * B64).sum(1)
    g = gamma(dim)
    if metric == DOT:
        s, beta = d, g * A
    elif metric == COSINE:
        with np.errstate(divide="ignore"):
            rq, rb = np.where(ssq > 0, 1 / np.sqrt(ssq), 0.0), np.where(ssb > 0, 1 / np.sqrt(ssb), 0.0)
        rr = rq[:, None] * rb[None, :]
        s, beta = d * rr, rr * (g * A + gamma(4) * (np.abs(d) + g * A))
    elif metric == L2:
        tot = ssq[:, None] + ssb[None, :]
        s = -(tot - 2 * d)
        beta = (1 + U) * (2 * g * A + gamma(2) * tot) + U * np.abs(s)
    else:
        raise ValueError(metric)
    return s, beta + dim * 2.0 ** -50 * A + 2.0 ** -45 * np.abs(s)


def eligibility(nq, nb, q_group=None, b_group=None, self_shift=None):
    """(nq, nb) bool.  self_shift = q_first - b_first of a self-search with EXCLUDE_SELF: base row j is query i itself when
    i + self_shift == j."""
    ok = np.ones((nq, nb), bool)
    if q_group is not None:
        ok &= np.asarray(q_group)[:, None] != np.asarray(b_group)[None, :]
    if self_shift is not None:
        i = np.arange(nq)
        j = i + self_shift
        hit = (j >= 0) & (j < nb)
        ok[i[hit], j[hit]] = False
    return ok


def reference_topk(s64, elig, k: int):
    """The order rule in float64: score descending, equal scores by ascending row, NaN below every number, ineligible rows never.
    -> (index (nq, k) int32, -1 in the tail; score (nq, k) float64, -inf in the tail)"""
    nq, nb = s64.shape
    index = np.full((nq, k), -1, np.int32)
    score = np.full((nq, k), -np.inf)
    for i in range(nq):
        rows = np.flatnonzero(elig[i])
        s = s64[i, rows]
        nan = np.isnan(s)
        order = np.lexsort((rows, np.where(nan, 0, -s), nan))[:k]      # last key first: non-NaN, then score descending, then row
        index[i, :len(order)] = rows[order]
        score[i, :len(order)] = s[order]
    return index, score


def ambiguous_share(s64, beta, elig, k: int) -> float:
    """The share of queries whose float64 top-k SET the bounds cannot settle: some omitted eligible row's s + beta reaches the
    smallest s - beta of the chosen rows."""
    index, _ = reference_topk(s64, elig, k)
    bad = 0
    for i in range(len(s64)):
        chosen = index[i][index[i] >= 0]
        out = elig[i].copy()
        out[chosen] = False
        if out.any() and len(chosen):
            bad += bool((s64[i, out] + beta[i, out]).max() >= (s64[i, chosen] - beta[i, chosen]).min())
    return bad / max(1, len(s64))


# ---- the key --------------------------------------------------------------------------------------------------------------------
def score_word(s32):
    """include/mmc.h: 1 for NaN, else the fp32 bits (of s + 0: -0 is +0) with the sign bit set for s >= 0, all bits inverted for s < 0"""
    s = np.asarray(s32, np.float32) + np.float32(0)
    u = s.view(np.uint32)
    w = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(s), np.uint32(1), w).astype(np.uint32)


def word_score(w):
    w = np.asarray(w, np.uint32)
    u = np.where(w & np.uint32(0x80000000), w ^ np.uint32(0x80000000), ~w).astype(np.uint32)
    u = np.where(w == 0, np.uint32(0xFF800000), np.where(w == 1, np.uint32(0x7FC00000), u)).astype(np.uint32)
    return u.view(np.float32)


def device_key(score32, index):
    """the 64-bit key of a returned (score, index) pair; 0 for a tail entry"""
    key = (score_word(score32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(index).astype(np.int64).astype(np.uint64))
    return np.where(np.asarray(index) < 0, np.uint64(0), key)


# ---- the acceptance rule ----------------------------------------------------------------------------------------------------------
def accept(index, score, s64, beta, elig, k: int, what: str = "") -> float:
    """Raises AssertionError unless every query's list passes the rule of the issue; -> the worst |score - s64| / beta."""
    index, score = np.asarray(index), np.asarray(score)
    nq, nb = s64.shape
    assert index.shape == (nq, k) and score.shape == (nq, k), f"{what}: shapes {index.shape} {score.shape}"
    assert index.dtype == np.int32 and score.dtype == np.float32, f"{what}: dtypes"
    worst = 0.0
    for i in range(nq):
        want = min(k, int(elig[i].sum()))
        got, sc = index[i, :want], score[i, :want]
        tag = f"{what} query {i}"
        assert int((index[i] >= 0).sum()) == want, f"{tag}: {int((index[i] >= 0).sum())} entries, {want} rows are eligible"
        assert np.all(index[i, want:] == -1) and np.all(np.isneginf(score[i, want:])), f"{tag}: the tail past {want} entries is not (-1, -inf)"
        assert np.all(got >= 0) and np.all(got < nb), f"{tag}: an index outside [0, {nb}): {got}"
        assert len(np.unique(got)) == want, f"{tag}: repeated rows {got}"
        assert np.all(elig[i, got]), f"{tag}: an ineligible row was returned: {got[~elig[i, got]]}"
        keys = device_key(sc, got)
        assert np.all(keys[:-1] > keys[1:]), f"{tag}: not sorted by (score descending, row ascending)"
        err = np.abs(sc.astype(np.float64) - s64[i, got])
        assert np.all(err <= beta[i, got]), f"{tag}: score error {err.max():.3g} over its bound ({(err / beta[i, got]).max():.3g} x)"
        if want:
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, float(np.nanmax(np.where(beta[i, got] > 0, err / beta[i, got], 0.0))))
            out = elig[i].copy()
            out[got] = False
            if out.any():
                last = got[-1]
                better = (s64[i] - beta[i] > s64[i, last] + beta[i, last]) & out
                assert not better.any(), f"{tag}: rows {np.flatnonzero(better)[:5]} beat the last entry beyond the bounds but are missing"
    return worst


def assert_exact(index, score, s64, elig, k: int, what: str = ""):
    """the integer-valued cases: index and score equal the float64 reference bit for bit, tie order included"""
    r_index, r_score = reference_topk(s64, elig, k)
    assert np.array_equal(np.asarray(index), r_index), f"{what}: index differs from the float64 reference"
    want = (r_score.astype(np.float32) + np.float32(0)).view(np.uint32)
    assert np.array_equal(np.asarray(score, np.float32).view(np.uint32), want), f"{what}: score bits differ"


# ---- the emulation ----------------------------------------------------------------------------------------------------------------
def fmaf_chain(Q, B):
    """(nq, nb) float32: acc = fl32(acc + q_c b_c) for c ascending.  The product of two fp32 is exact in float64; the sum is rounded to
    float64 and then to float32, which differs from the one rounding of an fmaf only when the float64 sum lands exactly on a float32
    midpoint that the exact sum missed -- never for the integer-valued inputs, and within the bounds otherwise."""
    Q64, B64 = np.asarray(Q, np.float32).astype(np.float64), np.asarray(B, np.float32).astype(np.float64)
    acc = np.zeros((Q64.shape[0], B64.shape[0]), np.float32)
    for c in range(Q64.shape[1]):
        acc = (acc.astype(np.float64) + Q64[:, c, None] * B64[None, :, c]).astype(np.float32)
    return acc


def norms(X):
    """(s, r) float32 per row: fl32 of the float64 sum of squares in column order, fl32(1 / sqrt) of it, 0 for a zero row"""
    X64 = np.asarray(X, np.float32).astype(np.float64)
    acc = np.zeros(len(X64))
    for c in range(X64.shape[1]):
        acc = acc + X64[:, c] * X64[:, c]        # x * x is exact in float64: the fma's one rounding
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(acc > 0, 1.0 / np.sqrt(acc), 0.0)
    return acc.astype(np.float32), r.astype(np.float32)


def scores32(Q, B, metric: int):
    d = fmaf_chain(Q, B)
    if metric == DOT:
        return d
    sq, rq = norms(Q)
    sb, rb = norms(B)
    if metric == COSINE:
        return (d * rq[:, None]) * rb[None, :]
    t = (sq[:, None] + sb[None, :]).astype(np.float32)
    return (-((np.float32(-2) * d).astype(np.float64) + t.astype(np.float64))).astype(np.float32)   # -2 d is exact: one rounding


def emulate(Xq, q_first, nq, Xb, b_first, nb, k, metric, q_group=None, b_group=None, exclude_self=False, bug=None, chunk=CHUNK):
    """The walk of mmc_featureset_knn in numpy on whole-set arrays Xq, Xb: chunks of queries, 128 x 128 tiles, splits, per-split lists
    of keys, the merge.  ``bug``: None or one of BUGS.  -> (index int32, score float32), each (nq, k)."""
    assert bug is None or bug in BUGS
    if bug == "first_ignored":
        q_first = b_first = 0
    Q = np.asarray(Xq, np.float32)[q_first:q_first + nq]
    B = np.asarray(Xb, np.float32)[b_first:b_first + nb]
    dim = Q.shape[1]
    self_shift = (q_first - b_first) if exclude_self else None
    index = np.full((nq, k), -1, np.int32)
    score = np.full((nq, k), -np.inf, np.float32)
    if nq == 0 or nb == 0:
        return index, score
    S, tb = splits(nq, nb), (nb + TILE - 1) // TILE
    padded = np.zeros((tb * TILE, dim), np.float32)
    padded[:nb] = B
    for c0 in range(0, nq, chunk):
        cn = min(chunk, nq - c0)
        Qc = Q[c0:c0 + cn]
        elig = eligibility(cn, nb, None if q_group is None else np.asarray(q_group)[c0:c0 + cn], b_group,
                           None if self_shift is None else self_shift + c0)
        elig_p = np.zeros((cn, tb * TILE), bool)
        elig_p[:, :nb] = elig
        if bug == "padding_rows":
            elig_p[:, nb:] = True
        per_split = []
        for s in range(S):
            lists = np.zeros((cn, k), np.uint64)
            for t in range(s * tb // S, (s + 1) * tb // S):
                cols = np.arange(t * TILE, (t + 1) * TILE)
                sc = scores32(Qc, padded[cols], metric)
                word = sc.view(np.uint32) if bug == "raw_bit_keys" else score_word(sc)
                low = cols.astype(np.uint64) if bug == "ties_descending" else np.uint64(0xFFFFFFFF) - cols.astype(np.uint64)
                keys = (word.astype(np.uint64) << np.uint64(32)) | low[None, :]
                if bug != "exclude_after":
                    keys = np.where(elig_p[:, cols], keys, np.uint64(0))
                lists = np.sort(np.concatenate([lists, keys], axis=1), axis=1)[:, ::-1][:, :k]
            per_split.append(lists)
        merged = np.zeros((cn, k), np.uint64)
        for lists in per_split:
            if bug == "merge_drops_short":
                lists = np.where(lists[:, -1:] == 0, np.uint64(0), lists)
            merged = np.sort(np.concatenate([merged, lists], axis=1), axis=1)[:, ::-1][:, :k]
        word = (merged >> np.uint64(32)).astype(np.uint32)
        low = (merged & np.uint64(0xFFFFFFFF)).astype(np.int64)
        row = low if bug == "ties_descending" else 0xFFFFFFFF - low
        have = merged != 0
        if bug == "exclude_after":   # the mask meets the finished list: what it removes leaves a hole, the rest moves up
            have &= np.take_along_axis(elig_p, np.where(have, row, 0), axis=1)
            order = np.argsort(~have, axis=1, kind="stable")
            have, row, word = (np.take_along_axis(a, order, axis=1) for a in (have, row, word))
        sc = word.view(np.float32) if bug == "raw_bit_keys" else word_score(word)
        index[c0:c0 + cn] = np.where(have, row, -1)
        score[c0:c0 + cn] = np.where(have, sc, -np.inf)
    if bug == "index_absolute":
        index = np.where(index >= 0, index + b_first, index)
    return index, score
