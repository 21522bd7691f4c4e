"""The definition of a head ensemble (include/mmc.h, "head ensembles") in numpy, for the host and the GPU tests.

Input is what each member's own ``mmc_head_predict`` writes: ``member_proba`` of shape (M, n_points * G, K), float32.  Everything
the device must reproduce bit for bit is computed here in float32 with the same operation order (left to right, one division);
the entropies are float64 and come with a bound derived below.

The bound on the three stats
----------------------------
The kernel computes, for a float32 row p of K classes, S = sum_c t_c with t_c = -p_c log p_c (0 when p_c == 0), in double:
  * p_c -> double is exact; log is the double-precision library log (at most 1 ulp), the product one more rounding (1/2 ulp), the
    negation exact: each term has a relative error of at most 2 u, u = 2^-53.  We allow 4 u.
  * the K terms are non-negative and are added in some fixed order (lane-strided partials, then a 6-level butterfly): any order of
    K - 1 double additions of non-negative terms is within (K - 1) u S of the exact sum, to first order.
  So |S_dev - S| <= (K + 3) u S, and S <= log K.  The float64 reference here obeys the same bound, so the two differ by at most
  2 (K + 3) u log K.  The expected member entropy adds M such sums (M - 1 additions) and divides once: (M + 1) u log K more on
  each side.  Together: D(K, M) = 2 (K + M + 8) u log K, an absolute error, for stats[0] and stats[1]; the mutual information is
  the difference of the two doubles (one more rounding, covered by the 8) and gets 2 D.
  * the result is rounded to float32 once: at most half a float32 ulp, i.e. 2^-24 |value| (2^-149 in the subnormal range).
  bound(value) = 2^-24 |value| + 2^-149 + D      (2 D for the mutual information)
The bound depends on K, M and the reference value alone, never on what the device returned.
"""

import numpy as np

U64 = 2.0 ** -53
STATS = 3


def member_means(member_proba, G):
    """(M, n_points * G, K) float32 -> m (M, n_points, K) float32: (v_0 + ... + v_{G-1}) / float32(G), left to right."""
    v = np.ascontiguousarray(member_proba, dtype=np.float32)
    M, rows, K = v.shape
    assert rows % G == 0
    v = v.reshape(M, rows // G, G, K)
    acc = v[:, :, 0, :].copy()
    for g in range(1, G):
        acc = (acc + v[:, :, g, :]).astype(np.float32)
    return (acc / np.float32(G)).astype(np.float32)


def ensemble_mean(m):
    """m (M, n_points, K) float32 -> e (n_points, K) float32: (m_0 + ... + m_{M-1}) / float32(M), left to right."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    acc = m[0].copy()
    for j in range(1, m.shape[0]):
        acc = (acc + m[j]).astype(np.float32)
    return (acc / np.float32(m.shape[0])).astype(np.float32)


def topk(e, k):
    """Score descending, equal scores in class order (a stable sort): (idx (n, k) int32, scores (n, k) float32)."""
    order = np.argsort(-e.astype(np.float64), axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(e, order, 1)


def entropy(p):
    """H(p) = -sum_c p_c log p_c over the last axis in float64; a class with p_c == 0 adds 0 (NaN stays NaN)."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p == 0, 0.0, -p * np.log(p))
    return t.sum(axis=-1)


def first_max(p):
    """The first maximum per row, as numpy.argmax and a stable descending sort give it."""
    return np.argmax(p, axis=-1).astype(np.int32)


def stats_and_votes(m, e):
    """-> (stats (n, 3) float64: H(e), mean_j H(m_j), their difference; votes (n,) int32)."""
    M = m.shape[0]
    h_e = entropy(e)
    h_m = np.zeros_like(h_e)
    for j in range(M):          # member order
        h_m = h_m + entropy(m[j])
    h_m = h_m / M
    best = first_max(e)
    votes = np.zeros(e.shape[0], np.int32)
    for j in range(M):
        votes += (first_max(m[j]) == best).astype(np.int32)
    return np.stack([h_e, h_m, h_e - h_m], axis=1), votes


def double_term(K, M):
    return 2.0 * (K + M + 8) * U64 * np.log(K)


def stats_bound(ref_stats, K, M):
    """The bound on |device float32 - reference float64| for each of the three stats (see the module docstring)."""
    ref = np.asarray(ref_stats, dtype=np.float64)
    d = double_term(K, M) * np.array([1.0, 1.0, 2.0])
    return 2.0 ** -24 * np.abs(ref) + 2.0 ** -149 + d


def jensen_slack(K, M):
    """What float32 rounding of e can take from H(e) >= mean_j H(m_j): e_c is within (M + 1) 2^-24 e_c of the exact mean (M - 1
    additions and one division, each half an ulp of a partial sum <= M e_c ... bounded loosely by (M + 1) ulps of e_c), and
    |dH| <= sum_c |1 + log e_c| |de_c| <= (M + 1) 2^-24 (sum_c e_c + H(e)) <= (M + 1) 2^-24 (1 + 1e-4 + log K)."""
    return (M + 1) * 2.0 ** -24 * (1.0001 + np.log(K))


def definition(member_proba, G, k):
    """Everything at once: dict with m, e, idx, scores, stats (float64), votes."""
    m = member_means(member_proba, G)
    e = ensemble_mean(m)
    idx, scores = topk(e, k)
    stats, votes = stats_and_votes(m, e)
    return {"m": m, "e": e, "idx": idx, "scores": scores, "stats": stats, "votes": votes}


def risk_coverage(correct, uncertainty, levels):
    """Accuracy of the rows kept when the most uncertain are set aside: rows are ordered by uncertainty ascending with a stable
    sort (ties by row), coverage c keeps the first ceil(c n) of them (at least one).  -> accuracies, one per level."""
    correct = np.asarray(correct, dtype=np.float64)
    order = np.argsort(np.asarray(uncertainty, dtype=np.float64), kind="stable")
    n = len(order)
    out = []
    for c in levels:
        keep = max(1, int(np.ceil(c * n - 1e-12)))
        out.append(float(correct[order[:keep]].mean()))
    return np.array(out)
