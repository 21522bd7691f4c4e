"""The nearest-neighbour checker against itself, and neighbors.py's host algebra against brute-force numpy; no device.

The honest emulation of the kernel's walk (tests/neighbors_checker.py) passes the acceptance rule on the inputs the GPU tests use,
each of the seven classic bugs fails it, the derived bounds hold for the emulated fp32 arithmetic, and the float64 top-k sets of
those inputs are settled by the bounds for at least 95 % of the queries."""

import re

import numpy as np
import pytest

import neighbors_checker as ck
from conftest import ROOT

DIMS = (8, 72)
METRICS = (ck.DOT, ck.COSINE, ck.L2)


def _case(dim, metric, nq, nb, nb_max=ck.NB_MAX):
    Xq, yq, Xb, yb = ck.bounded_inputs(dim, seed=10 * dim, nb_max=nb_max)
    s64, beta = ck.reference(Xq[ck.FIRST_Q:ck.FIRST_Q + nq], Xb[ck.FIRST_B:ck.FIRST_B + nb], metric)
    return Xq, Xb, s64, beta


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_honest_emulation_passes_the_rule_and_the_bounds_hold(dim, metric):
    for nq in (1, 129):
        for nb in (1, 127, 128, 129, 700):
            Xq, Xb, s64, beta = _case(dim, metric, nq, nb)
            s32 = ck.scores32(Xq[ck.FIRST_Q:ck.FIRST_Q + nq], Xb[ck.FIRST_B:ck.FIRST_B + nb], metric)
            assert np.all(np.abs(s32.astype(np.float64) - s64) <= beta)              # the bounds hold for the emulated arithmetic
            elig = ck.eligibility(nq, nb)
            for k in (1, 5, 32):
                index, score = ck.emulate(Xq, ck.FIRST_Q, nq, Xb, ck.FIRST_B, nb, k, metric)
                ck.accept(index, score, s64, beta, elig, k, f"dim {dim} {ck.METRIC_NAMES[metric]} nq {nq} nb {nb} k {k}")


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_at_most_five_percent_of_the_reference_sets_are_ambiguous(dim, metric):
    """the cap of the issue, on the reference alone: the clustered inputs must let the bounds settle the top-k set"""
    for nb in (129, 700):
        _, _, s64, beta = _case(dim, metric, 129, nb)
        for k in (1, 5, 32):
            share = ck.ambiguous_share(s64, beta, ck.eligibility(129, nb), k)
            assert share <= 0.05, (dim, metric, nb, k, share)
    Xq, yq, Xb, yb = ck.bounded_inputs(1280, seed=5, nb_max=300)
    s64, beta = ck.reference(Xq[ck.FIRST_Q:ck.FIRST_Q + 129], Xb[ck.FIRST_B:ck.FIRST_B + 300], metric)
    assert ck.ambiguous_share(s64, beta, ck.eligibility(129, 300), 5) <= 0.05


def test_emulation_with_splits_chunks_groups_and_self_exclusion():
    dim, nb = 8, ck.NB_TWO_TILES
    assert ck.splits(129, nb) == ck.MAX_SPLITS and (nb + ck.TILE - 1) // ck.TILE == 2 * ck.MAX_SPLITS
    Xq, Xb, s64, beta = _case(dim, ck.L2, 129, nb, nb_max=nb)
    index, score = ck.emulate(Xq, ck.FIRST_Q, 129, Xb, ck.FIRST_B, nb, 5, ck.L2)
    ck.accept(index, score, s64, beta, ck.eligibility(129, nb), 5, "two tiles per split")
    again, _ = ck.emulate(Xq, ck.FIRST_Q, 129, Xb, ck.FIRST_B, nb, 5, ck.L2, chunk=50)     # another chunking: the same lists
    assert np.array_equal(index, again)
    # a self-search on overlapping ranges with groups that knock out base tile 1 for the queries of group 7
    X, _ = ck.clustered(400, dim, 4, seed=3, negate_from=200)
    q_first, nq, b_first, nb = 10, 129, 4, 300
    bg = np.arange(nb, dtype=np.int32) % 5
    bg[128:256] = 7
    qg = np.where(np.arange(nq) % 3 == 0, 7, 100 + np.arange(nq)).astype(np.int32)
    elig = ck.eligibility(nq, nb, qg, bg, q_first - b_first)
    assert not elig[0, 128:256].any() and not elig[1, 1 + 6]
    for metric in METRICS:
        s64, beta = ck.reference(X[q_first:q_first + nq], X[b_first:b_first + nb], metric)
        index, score = ck.emulate(X, q_first, nq, X, b_first, nb, 32, metric, qg, bg, exclude_self=True)
        ck.accept(index, score, s64, beta, elig, 32, f"self-search {ck.METRIC_NAMES[metric]}")


def test_integer_cases_match_float64_bit_for_bit():
    X, _ = ck.integer_rows(450, 8, seed=1)
    for metric in (ck.DOT, ck.L2):
        for nq, nb, k in ((129, 300, 5), (129, 129, 32), (1, 127, 1)):
            s64, _ = ck.reference(X[2:2 + nq], X[20:20 + nb], metric)
            elig = ck.eligibility(nq, nb, self_shift=2 - 20)
            assert len(np.unique(s64[0])) < nb or nb < 50                              # ties are plentiful
            index, score = ck.emulate(X, 2, nq, X, 20, nb, k, metric, exclude_self=True)
            ck.assert_exact(index, score, s64, elig, k, f"{ck.METRIC_NAMES[metric]} {nq} x {nb} k {k}")


def _bug_fails(bug, match, X, q_first, nq, b_first, nb, k, metric, qg=None, bg=None, exclude_self=False, Xb=None):
    Xb = X if Xb is None else Xb
    s64, beta = ck.reference(X[q_first:q_first + nq], Xb[b_first:b_first + nb], metric)
    elig = ck.eligibility(nq, nb, qg, bg, q_first - b_first if exclude_self else None)
    index, score = ck.emulate(X, q_first, nq, Xb, b_first, nb, k, metric, qg, bg, exclude_self)
    ck.accept(index, score, s64, beta, elig, k, "honest")
    index, score = ck.emulate(X, q_first, nq, Xb, b_first, nb, k, metric, qg, bg, exclude_self, bug=bug)
    with pytest.raises(AssertionError, match=match):
        ck.accept(index, score, s64, beta, elig, k, bug)


def test_each_classic_bug_fails_where_its_fault_is():
    Xi, _ = ck.integer_rows(300, 8, seed=2)
    Xq, yq, Xb, yb = ck.bounded_inputs(8, seed=80)
    FQ, FB = ck.FIRST_Q, ck.FIRST_B
    _bug_fails("ties_descending", "not sorted", Xi, 0, 40, 0, 300, 5, ck.DOT)                     # equal scores in the wrong order
    _bug_fails("raw_bit_keys", "not sorted|beat the last", Xq, FQ, 129, FB, 300, 5, ck.DOT, Xb=Xb)  # queries 64..: negative scores
    _bug_fails("padding_rows", r"outside \[0, 127\)", Xq, FQ, 129, FB, 127, 5, ck.COSINE, Xb=Xb)  # a zero row's 0 beats them
    bg = (np.arange(300) % 2).astype(np.int32)
    qg = (np.arange(129) % 2).astype(np.int32)
    _bug_fails("exclude_after", "entries, .* rows are eligible", Xq, FQ, 129, FB, 300, 5, ck.L2, qg, bg, Xb=Xb)   # short lists
    _bug_fails("merge_drops_short", "beat the last entry", Xq, FQ, 129, FB, 129, 32, ck.L2, Xb=Xb)  # the 1-row split is dropped
    _bug_fails("first_ignored", "score error|beat the last", Xq, FQ, 129, FB, 300, 5, ck.COSINE, Xb=Xb)      # decoys and far rows answer
    _bug_fails("index_absolute", "score error|outside|beat the last", Xq, FQ, 129, FB, 300, 5, ck.L2, Xb=Xb)
    # and bit for bit: the tie order alone is enough
    s64, _ = ck.reference(Xi[:40], Xi, ck.DOT)
    index, score = ck.emulate(Xi, 0, 40, Xi, 0, 300, 5, ck.DOT, bug="ties_descending")
    with pytest.raises(AssertionError, match="index differs"):
        ck.assert_exact(index, score, s64, ck.eligibility(40, 300), 5)


def test_key_orders_like_the_rule():
    s = np.array([np.nan, -np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, np.inf], np.float32)
    w = ck.score_word(s)
    assert w[0] == 1 and w[1] == 0x007FFFFF and w[-1] == 0xFF800000 and w[4] == w[5] == 0x80000000
    assert np.all(w[:4].astype(np.int64) < w[1:5].astype(np.int64)) and np.all(np.diff(w[5:].astype(np.int64)) > 0) and np.all(w > 0)
    back = ck.word_score(w)
    assert np.isnan(back[0]) and np.array_equal(back[1:].view(np.uint32), (s[1:] + np.float32(0)).view(np.uint32))
    assert np.isneginf(ck.word_score(np.uint32(0)))


def test_split_rule_in_python_equals_the_header():
    from mermaid_classifier_amd import _lib
    from mermaid_classifier_amd.neighbors import knn_splits
    header = (ROOT / "include" / "mmc.h").read_text()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MMC_KNN_[A-Z0-9_]+) (\d+)u?\b", header)}
    assert consts == {"MMC_KNN_MAX_K": 32, "MMC_KNN_DOT": 0, "MMC_KNN_COSINE": 1, "MMC_KNN_L2": 2, "MMC_KNN_EXCLUDE_SELF": 4,
                      "MMC_KNN_TILE_ROWS": 128, "MMC_KNN_CHUNK_ROWS": 8192, "MMC_KNN_MAX_SPLITS": 16}
    for name, value in consts.items():
        assert getattr(_lib, name) == value, name
    assert (ck.TILE, ck.CHUNK, ck.MAX_SPLITS, ck.MAX_K) == (128, 8192, 16, 32)
    assert "S = min(MMC_KNN_MAX_SPLITS, T_b, max(1, 1024 / T_q))" in header
    for nq, nb in ((1, 1), (1, 129), (129, 700), (129, ck.NB_TWO_TILES), (8192, 10 ** 5), (20000, 200000), (200000, 200000), (5000, 3000)):
        tq, tb = -(-min(nq, 8192) // 128), -(-nb // 128)
        want = min(16, tb, max(1, 1024 // tq))
        assert knn_splits(nq, nb) == want == ck.splits(nq, nb), (nq, nb)


# ---- neighbors.py on hand-made lists ------------------------------------------------------------------------------------------------
def _hand_made(seed=0, nq=40, k=6, K=5):
    from mermaid_classifier_amd.neighbors import Neighbors
    rng = np.random.default_rng(seed)
    index = rng.integers(0, 1000, (nq, k)).astype(np.int32)
    score = np.sort(rng.uniform(0.1, 1.0, (nq, k)).astype(np.float32), axis=1)[:, ::-1].copy()
    label = rng.integers(0, K, (nq, k)).astype(np.int32)
    for i in range(nq):                      # short lists, an empty one included
        cut = k if i % 4 else int(rng.integers(0, k))
        if i == 3:
            cut = 0
        index[i, cut:], score[i, cut:], label[i, cut:] = -1, -np.inf, -1
    classes = np.array([3, 10, 11, 40, 77])
    return Neighbors(index, score, label, classes), rng


def test_votes_predict_agreement_against_brute_force():
    nb, rng = _hand_made()
    K = len(nb.classes)
    for weights in ("uniform", "score"):
        want = np.zeros((len(nb), K))
        for i in range(len(nb)):
            for j in range(nb.k):
                if nb.index[i, j] >= 0:
                    want[i, nb.label[i, j]] += 1.0 if weights == "uniform" else float(nb.score[i, j])
        got = nb.votes(weights)
        assert got.shape == (len(nb), K) and np.allclose(got, want, rtol=1e-15, atol=0)
        pred = nb.predict(weights)
        for i in range(len(nb)):
            best = [c for c in range(K) if want[i, c] == want[i].max()][0]          # ties: class order
            assert pred[i] == nb.classes[best]
    tie = type(nb)([[5, 6]], [[0.5, 0.5]], [[3, 1]], nb.classes)
    assert tie.predict()[0] == nb.classes[1]
    y = nb.classes[rng.integers(0, K, len(nb))]
    agree = nb.agreement(y)
    for i in range(len(nb)):
        lab = [nb.classes[nb.label[i, j]] for j in range(nb.k) if nb.index[i, j] >= 0]
        if lab:
            assert agree[i] == sum(v == y[i] for v in lab) / len(lab)
        else:
            assert np.isnan(agree[i])
    assert np.isnan(agree[3])
    with pytest.raises(ValueError, match="not in classes"):
        nb.agreement(np.full(len(nb), 4))
    with pytest.raises(ValueError, match="weights"):
        nb.votes("rank")
    with pytest.raises(ValueError, match="one .nq, k. shape"):
        type(nb)(nb.index, nb.score[:, :2], nb.label, nb.classes)


def test_audit_table_and_duplicate_pairs_against_brute_force():
    from mermaid_classifier_amd.neighbors import audit_table, confusion_table, duplicate_pairs
    nb, rng = _hand_made(seed=4)
    K = len(nb.classes)
    y = nb.classes[rng.integers(0, K, len(nb))]
    t = audit_table(nb, y)
    agree = nb.agreement(y)
    key = [(np.inf if np.isnan(a) else a, i) for i, a in enumerate(agree)]
    order = [i for _, i in sorted(key)]
    assert t["row"].tolist() == order and np.array_equal(t["label"], y[order])
    assert np.array_equal(t["agreement"], agree[order], equal_nan=True)
    for pos, i in enumerate(order):
        counts = np.bincount(nb.label[i][nb.index[i] >= 0], minlength=K)
        if counts.sum():
            assert t["majority"][pos] == nb.classes[int(np.argmax(counts))] and t["majority_share"][pos] == counts.max() / counts.sum()
        else:
            assert np.isnan(t["majority_share"][pos])
    d = duplicate_pairs(nb, 0.8)
    want = [(i, int(nb.index[i, j]), nb.score[i, j]) for i in range(len(nb)) for j in range(nb.k)
            if nb.index[i, j] >= 0 and nb.score[i, j] >= np.float32(0.8)]
    assert list(zip(d["a"].tolist(), d["b"].tolist(), d["score"].tolist())) == [(a, b, float(s)) for a, b, s in want] and len(want) > 5
    gt, est, src = rng.integers(0, K, 200), rng.integers(0, K, 200), rng.integers(0, 3, 200)
    c = confusion_table(gt, est, K)
    cs = confusion_table(gt, est, K, src, 4)
    assert c.sum() == 200 and cs.shape == (4, K, K) and np.array_equal(cs.sum(0), c) and not cs[3].any()
    for a, b, s in zip(gt[:20], est[:20], src[:20]):
        assert cs[s, a, b] >= 1
    assert c[gt[0], est[0]] == int(((gt == gt[0]) & (est == est[0])).sum())


def test_nearest_rejects_bad_arguments_before_a_device_is_touched():
    from mermaid_classifier_amd import FeatureSet, nearest
    a, b = FeatureSet(8, [0, 1]), FeatureSet(9, [0, 1])
    with pytest.raises(ValueError, match="features"):
        nearest(a, b, 3)
    with pytest.raises(ValueError, match="metric"):
        nearest(a, a, 3, "manhattan")
    for k in (0, 33, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            nearest(a, a, k)
    with pytest.raises(ValueError, match="same set"):
        nearest(a, FeatureSet(8, [0, 1]), 3, exclude_self=True)
    with pytest.raises(ValueError, match="both, or neither"):
        nearest(a, a, 3, query_groups=np.zeros(0, np.int32))
    with pytest.raises(ValueError, match="FeatureSets"):
        nearest(np.zeros((2, 8)), a, 3)
    assert a._h is None and b._h is None
