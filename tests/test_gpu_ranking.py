"""-m gpu: ranking validation on the device (rank_rows_kernel behind mmc_head_evaluate_ranked / _set, ranking.ranking_validate).

The checker is ``restate_ranked`` of test_ranking_host.py applied to the probabilities ``mmc_head_predict`` returns for the same
rows on the same handle.  Every comparison is integer equality: ``class_rank_hist`` and ``hier_hist`` against the restatement;
``hier_hist`` again from the classes ``mmc_head_topk(k = kmax)`` names; column sums = ``rank_hist``, row sums = scored rows per class,
first column = the diagonal of ``confusion``; every row of ``hier_hist`` sums to the scored rows and its cumulative counts from the
top level never shrink with j.
Shapes: K = 5 (fewer classes than lanes, kmax = K), 108 (no multiple of 64), 70 (all probabilities equal), 2100 (row in global
memory, lanes own 33 classes); 70 000 rows (two chunks, the second partial); kmax 1 and 16, n_levels 1 and 256; unknown and NaN
rows; either table alone."""

import numpy as np
import pytest

from conftest import GOLDEN
from test_ranking_host import restate_ranked

pytestmark = pytest.mark.gpu

PER_ROW = ("est", "score", "rank", "p_true")
EVAL_TABLES = ("totals", "confusion", "rank_hist")


def _load(name):
    from mermaid_classifier_amd import load_predictor
    return load_predictor(GOLDEN / name / "model.pt", GOLDEN / name / "model.json")


def _ptr(a):
    return None if a is None else a.ctypes.data


def _levels(rng, K, n_levels):
    """random level codes that use every level the table has room for, the top one on the diagonal"""
    lv = rng.integers(0, n_levels, (K, K)).astype(np.uint8)
    lv.flat[:min(n_levels, K * K)] = np.arange(min(n_levels, K * K))
    np.fill_diagonal(lv, n_levels - 1)
    return np.ascontiguousarray(lv)


def c_ranked(head, X, y, levels=None, n_levels=1, kmax=1, lmap=None, fs=None, first=0, want_class=True, want_hier=None, expect=0):
    """mmc_head_evaluate_ranked on host rows, or _set on rows [first, first + len(y)) of ``fs``; every output starts from -7.
    -> dict of outputs (``hier_hist`` is kmax x n_levels when both are in range)."""
    from mermaid_classifier_amd import _lib
    K, n = head.n_classes, len(y)
    y = np.ascontiguousarray(y, np.int32)
    sized = 1 <= n_levels <= 256 and 1 <= kmax <= 16
    o = dict(est=np.full(n, -7, np.int32), score=np.full(n, -7, np.float32), rank=np.full(n, -7, np.int32), p_true=np.full(n, -7, np.float32),
             totals=np.full(5, -7, np.int64), confusion=np.full((K, K), -7, np.int64), rank_hist=np.full(K, -7, np.int64),
             class_rank_hist=np.full((K, K), -7, np.int64), hier_hist=np.full((kmax, n_levels) if sized else (16, 256), -7, np.int64))
    want_hier = levels is not None if want_hier is None else want_hier
    common = [_ptr(lmap), 0 if lmap is None else len(lmap)] + [o[k].ctypes.data for k in PER_ROW + EVAL_TABLES] + \
             [_ptr(levels), n_levels, kmax, o["class_rank_hist"].ctypes.data if want_class else None, o["hier_hist"].ctypes.data if want_hier else None]
    lib = _lib.lib()
    if fs is not None:
        status = lib.mmc_head_evaluate_ranked_set(head._h, fs._handle(), first, n, *common, None)
    else:
        X = np.ascontiguousarray(X, np.float32)
        status = lib.mmc_head_evaluate_ranked(head._h, X.ctypes.data, y.ctypes.data, n, *common, _lib.MMC_IN_HOST, None)
    assert status == expect, lib.mmc_last_error()
    o["sized"] = sized
    if not want_class:
        assert (o.pop("class_rank_hist") == -7).all()
    if not want_hier:
        assert (o.pop("hier_hist") == -7).all()
    return o


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        va, vb = np.asarray(a[k]), np.asarray(b[k])
        assert va.dtype == vb.dtype and va.tobytes() == vb.tobytes(), k


def matches_checker(o, head, X, g, levels, n_levels, kmax, what):
    """``g``: the head's class of a row with a known class, else -1.  Rows with a non-finite probability are unscored too."""
    K = head.n_classes
    X = np.ascontiguousarray(X, np.float32)
    proba, _ = head.predict(X)
    g = np.where(np.isfinite(proba).all(1), np.asarray(g, np.int64), -1)
    ok = g >= 0
    n_scored = int(ok.sum())
    want_class, want_hier = restate_ranked(proba, g, K, kmax, levels, n_levels)
    if "class_rank_hist" in o:
        ch = o["class_rank_hist"]
        assert np.array_equal(ch, want_class), f"{what}: class_rank_hist"
        assert np.array_equal(ch.sum(0), o["rank_hist"]), f"{what}: column sums"
        assert np.array_equal(ch.sum(1), np.bincount(g[ok], minlength=K)), f"{what}: row sums"
        assert np.array_equal(ch[:, 0], np.diag(o["confusion"])), f"{what}: first column"
    if "hier_hist" in o:
        hh = o["hier_hist"]
        assert hh.shape == (kmax, n_levels) and np.array_equal(hh, want_hier), f"{what}: hier_hist"
        idx, _ = head.topk(X, kmax)                                                 # independently: the classes mmc_head_topk names
        m = np.maximum.accumulate(levels[g[ok][:, None], idx[ok]].astype(np.int64), axis=1)
        assert np.array_equal(hh, np.stack([np.bincount(m[:, j], minlength=n_levels) for j in range(kmax)])), f"{what}: hier_hist from top-k"
        assert (hh.sum(1) == n_scored).all(), f"{what}: rows of hier_hist"
        from_top = hh[:, ::-1].cumsum(1)
        assert (np.diff(from_top, axis=0) >= 0).all(), f"{what}: hier_hist shrinks with j"
    assert int(o["totals"][0] - o["totals"][2] - o["totals"][3]) == n_scored, what
    print(f"{what}: {len(X)} rows ({n_scored} scored), K = {K}, kmax = {kmax}, {n_levels} levels: every table equal")


def _set_of(head, X, y, n_classes=None):
    from mermaid_classifier_amd import FeatureSet
    return FeatureSet(head.input_dim, list(range(head.n_classes if n_classes is None else n_classes))).append(X, y)


def _labels(rng, arg, K):
    """true classes that agree with the head in about 60 % of the rows"""
    return np.where(rng.random(len(arg)) < 0.6, arg, rng.integers(0, K, len(arg))).astype(np.int32)


# ---- 1. the two heads, both routes, twice; the evaluation keeps its bits ----

@pytest.mark.parametrize("name,kmax,n_levels", [("head_fixture", 5, 5), ("head108", 10, 7)])
def test_ranked_tables_match_the_restatement(name, kmax, n_levels):
    from test_gpu_validation import c_evaluate
    head = _load(name)._head
    K = head.n_classes
    rng = np.random.default_rng(21)
    X = np.load(GOLDEN / f"{name}_io.npz")["X"]
    y = _labels(rng, head.predict(X)[1], K)
    levels = _levels(rng, K, n_levels)
    assert K == (5 if name == "head_fixture" else 108) and kmax <= K
    host = c_ranked(head, X, y, levels, n_levels, kmax)
    matches_checker(host, head, X, y, levels, n_levels, kmax, f"{name} host rows")
    fs = _set_of(head, X, y)
    same_bits(host, c_ranked(head, None, y, levels, n_levels, kmax, fs=fs))
    same_bits(host, c_ranked(head, X, y, levels, n_levels, kmax))                   # a repeat call: identical bytes
    same_bits(host, c_ranked(head, None, y, levels, n_levels, kmax, fs=fs))
    plain = c_evaluate(head, X, y)                                                  # the seven shared outputs: mmc_head_evaluate's bytes
    for k in PER_ROW + EVAL_TABLES:
        assert plain[k].dtype == host[k].dtype and plain[k].tobytes() == host[k].tobytes(), k
    m = len(X) - 3                                                                  # a ragged last workgroup, a later first row
    assert m % 4 != 0
    part = c_ranked(head, None, y[3:], levels, n_levels, kmax, fs=fs, first=3)
    matches_checker(part, head, X[3:], y[3:], levels, n_levels, kmax, f"{name} rows [3, {len(X)}) of the set")
    fs.close()


# ---- 2. above the chunk ----

def test_ranked_above_the_65536_row_chunk():
    head = _load("head_fixture")._head
    X0 = np.load(GOLDEN / "head_fixture_io.npz")["X"]
    n, K = 70000, head.n_classes
    rng = np.random.default_rng(22)
    X = np.ascontiguousarray(np.tile(X0, (-(-n // len(X0)), 1))[:n])
    y = _labels(rng, head.predict(X)[1], K)
    levels = _levels(rng, K, 4)
    o = c_ranked(head, X, y, levels, 4, 3)
    matches_checker(o, head, X, y, levels, 4, 3, "two chunks, the second partial")
    parts = [c_ranked(head, X[a:b], y[a:b], levels, 4, 3) for a, b in ((0, 65536), (65536, n))]
    for k in ("class_rank_hist", "hier_hist", "confusion", "rank_hist", "totals"):  # integer tables: calls add up to the whole
        assert np.array_equal(parts[0][k] + parts[1][k], o[k]), k


# ---- 3. a head wider than the LDS row; the largest kmax and n_levels ----

def test_ranked_of_a_head_wider_than_the_lds_row():
    from mermaid_classifier_amd.inference import DeviceHead, HeadParams
    rng = np.random.default_rng(23)
    K = 2100
    head = DeviceHead(HeadParams([rng.normal(0, 0.5, (K, 8)).astype(np.float32)], [rng.normal(0, 0.1, K).astype(np.float32)],
                                 rng.uniform(-30, -5, K).astype(np.float32), rng.uniform(1, 4, K).astype(np.float32)))
    X = rng.normal(0, 1, (37, 8)).astype(np.float32)
    _, arg = head.predict(X)
    y = arg.copy()
    y[::3] = (7 * np.arange(len(y[::3])) * 41) % K
    levels = _levels(rng, K, 256)
    o = c_ranked(head, X, y, levels, 256, 16)
    matches_checker(o, head, X, y, levels, 256, 16, "K = 2100, row in global memory")
    same_bits(o, c_ranked(head, X, y, levels, 256, 16))
    from test_gpu_validation import c_evaluate
    plain = c_evaluate(head, X, y)
    for k in PER_ROW + EVAL_TABLES:
        assert plain[k].tobytes() == o[k].tobytes(), k
    head.close()


# ---- 4. the ends of kmax and n_levels ----

@pytest.mark.parametrize("name,kmax,n_levels", [("head_fixture", 1, 1), ("head108", 16, 256), ("head108", 1, 256), ("head108", 16, 1)])
def test_ranked_at_the_ends_of_kmax_and_n_levels(name, kmax, n_levels):
    head = _load(name)._head
    K = head.n_classes
    rng = np.random.default_rng(24)
    X = np.load(GOLDEN / f"{name}_io.npz")["X"][:203]
    y = _labels(rng, head.predict(X)[1], K)
    levels = _levels(rng, K, n_levels)
    o = c_ranked(head, X, y, levels, n_levels, kmax)
    matches_checker(o, head, X, y, levels, n_levels, kmax, f"{name} kmax = {kmax}, n_levels = {n_levels}")
    if n_levels == 1:
        assert (o["hier_hist"] == len(X)).all()


# ---- 5. ties ----

def test_all_probabilities_equal_picks_classes_in_order():
    """A one-layer head of zero weights and equal calibrators: every row's K probabilities are equal, so the picks are classes
    0 .. kmax - 1 in order.  levels[g][c] = c + 1 for c < 16 and 0 beyond: the running maximum at round j must be j + 1."""
    from mermaid_classifier_amd.inference import DeviceHead, HeadParams
    K, n, kmax = 70, 50, 16
    head = DeviceHead(HeadParams([np.zeros((K, 8), np.float32)], [np.zeros(K, np.float32)], np.full(K, -6, np.float32), np.full(K, 1.5, np.float32)))
    X = np.random.default_rng(25).normal(0, 1, (n, 8)).astype(np.float32)
    proba, _ = head.predict(X)
    assert (proba.view(np.uint32) == proba.view(np.uint32)[0, 0]).all()
    idx, _ = head.topk(X, kmax)
    assert (idx == np.arange(kmax)).all()
    y = np.full(n, K - 1, np.int32)                                                 # a true class that is never picked
    levels = np.zeros((K, K), np.uint8)
    levels[:, :16] = np.arange(1, 17)
    o = c_ranked(head, X, y, levels, 17, kmax)
    want = np.zeros((kmax, 17), np.int64)
    want[np.arange(kmax), np.arange(kmax) + 1] = n
    assert np.array_equal(o["hier_hist"], want)
    assert o["class_rank_hist"][K - 1, K - 1] == n and o["class_rank_hist"].sum() == n   # the last class ranks last
    matches_checker(o, head, X, y, levels, 17, kmax, "all probabilities equal")
    y2 = (np.arange(n) % K).astype(np.int32)                                        # the true class ranks y + 1
    o2 = c_ranked(head, X, y2, levels, 17, kmax)
    assert np.array_equal(o2["class_rank_hist"], np.diag(np.bincount(y2, minlength=K)))
    matches_checker(o2, head, X, y2, levels, 17, kmax, "all probabilities equal, every class true")
    head.close()


# ---- 6. unscored rows ----

def test_unknown_class_rows_enter_neither_table():
    head = _load("head_fixture")._head
    X = np.load(GOLDEN / "head_fixture_io.npz")["X"]
    K, n = head.n_classes, len(X)
    rng = np.random.default_rng(26)
    lmap = np.array([3, -1, 0, 4, 1, -1, 2], np.int32)                              # the caller's 7 labels; two of them unknown
    y = rng.integers(0, len(lmap), n).astype(np.int32)
    g = lmap[y]
    levels = _levels(rng, K, 6)
    o = c_ranked(head, X, y, levels, 6, 4, lmap=lmap)
    assert o["totals"][2] == int((g < 0).sum()) > 0
    matches_checker(o, head, X, g, levels, 6, 4, "label map with unknown classes")
    known = g >= 0
    clean = c_ranked(head, X[known], g[known], levels, 6, 4)                        # the same tables as the known rows alone
    for k in ("class_rank_hist", "hier_hist", "confusion", "rank_hist"):
        assert np.array_equal(o[k], clean[k]), k
    fs = _set_of(head, X, y, n_classes=len(lmap))
    same_bits(o, c_ranked(head, None, y, levels, 6, 4, lmap=lmap, fs=fs))
    fs.close()


def test_nan_rows_enter_neither_table():
    """A one-layer head, so that a NaN feature reaches the probabilities (a hidden ReLU would turn it into 0)."""
    from mermaid_classifier_amd.inference import DeviceHead, HeadParams
    rng = np.random.default_rng(27)
    K = 5
    head = DeviceHead(HeadParams([rng.normal(0, 0.7, (K, 8)).astype(np.float32)], [rng.normal(0, 0.1, K).astype(np.float32)],
                                 rng.uniform(-12, -4, K).astype(np.float32), rng.uniform(0.5, 2, K).astype(np.float32)))
    X = rng.normal(0, 1, (41, 8)).astype(np.float32)
    y = rng.integers(0, K, 41).astype(np.int32)
    levels = _levels(rng, K, 3)
    bad = X.copy()
    bad[[2, 17, 40]] = np.nan
    bad[9, 6] = np.nan
    keep = np.setdiff1d(np.arange(41), [2, 9, 17, 40])
    o = c_ranked(head, bad, y, levels, 3, 5)
    assert o["totals"].tolist()[:4] == [41, o["totals"][1], 0, 4]
    matches_checker(o, head, bad, y, levels, 3, 5, "NaN rows")
    clean = c_ranked(head, X[keep], y[keep], levels, 3, 5)
    for k in ("class_rank_hist", "hier_hist", "confusion", "rank_hist"):
        assert np.array_equal(o[k], clean[k]), k
    assert o["hier_hist"].sum(1).tolist() == [37] * 5 and o["class_rank_hist"].sum() == 37
    head.close()


# ---- 7. either table alone ----

def test_either_table_alone():
    head = _load("head108")._head
    K = head.n_classes
    rng = np.random.default_rng(28)
    X = np.load(GOLDEN / "head108_io.npz")["X"]
    y = _labels(rng, head.predict(X)[1], K)
    levels = _levels(rng, K, 9)
    both = c_ranked(head, X, y, levels, 9, 10)
    only_class = c_ranked(head, X, y, None, 1, 1)                                   # sim_level NULL: no selection, class_rank_hist only
    assert "hier_hist" not in only_class
    matches_checker(only_class, head, X, y, None, 1, 1, "class_rank_hist only")
    only_hier = c_ranked(head, X, y, levels, 9, 10, want_class=False)               # class_rank_hist NULL
    assert "class_rank_hist" not in only_hier
    matches_checker(only_hier, head, X, y, levels, 9, 10, "hier_hist only")
    for k in PER_ROW + EVAL_TABLES:
        assert both[k].tobytes() == only_class[k].tobytes() == only_hier[k].tobytes(), k
    assert np.array_equal(both["class_rank_hist"], only_class["class_rank_hist"]) and np.array_equal(both["hier_hist"], only_hier["hier_hist"])
    neither = c_ranked(head, X, y, None, 1, 1, want_class=False)                    # no table asked for: the plain evaluation
    for k in PER_ROW + EVAL_TABLES:
        assert both[k].tobytes() == neither[k].tobytes(), k


# ---- 8. rejections ----

def test_rejected_calls_launch_nothing_and_zero_the_tables():
    from mermaid_classifier_amd import _lib
    head = _load("head_fixture")._head
    K = head.n_classes
    X = np.load(GOLDEN / "head_fixture_io.npz")["X"][:20]
    y = (7 * np.arange(20) % K).astype(np.int32)
    levels = _levels(np.random.default_rng(29), K, 4)
    good = c_ranked(head, X, y, levels, 4, 3)
    lib = _lib.lib()

    def rejected(msg, **kw):
        args = dict(X=X, y=y, levels=levels, n_levels=4, kmax=3)
        args.update(kw)
        o = c_ranked(head, args.pop("X"), args.pop("y"), args.pop("levels"), expect=_lib.MMC_ERR_ARG, **args)
        assert msg.encode() in lib.mmc_last_error(), (msg, lib.mmc_last_error())
        for k in EVAL_TABLES + ("class_rank_hist",):
            assert not o[k].any(), (msg, k)
        if "hier_hist" in o and o["sized"]:
            assert not o["hier_hist"].any(), msg
        for k in PER_ROW:
            assert (o[k] == -7).all(), (msg, k)                                      # nothing ran

    rejected("n_levels = 0 outside [1, 256]", n_levels=0)
    rejected("n_levels = 257 outside [1, 256]", n_levels=257)
    rejected("kmax = 0 outside [1, 5]", kmax=0)
    rejected("kmax = 6 outside [1, 5]", kmax=6)                                     # above K, within MMC_RANKED_MAX_K: hier_hist is zeroed
    rejected("kmax = 17 outside [1, 5]", kmax=17)
    lv = levels.copy()
    lv[3, 2] = 4
    rejected("sim_level[17] = 4 outside [0, 4)", levels=lv)
    rejected("sim_level without hier_hist", want_hier=False)
    rejected("hier_hist without sim_level", levels=None, want_hier=True)
    rejected("label index y[0] = 5 outside [0, 5)", y=np.where(np.arange(20) == 0, 5, y).astype(np.int32))
    # kmax is bounded by MMC_RANKED_MAX_K on a head with more classes
    big = _load("head108")._head
    Xb = np.load(GOLDEN / "head108_io.npz")["X"][:8]
    ob = c_ranked(big, Xb, np.zeros(8, np.int32), _levels(np.random.default_rng(1), 108, 2), 2, 17, expect=_lib.MMC_ERR_ARG)
    assert b"kmax = 17 outside [1, 16]" in lib.mmc_last_error() and not ob["class_rank_hist"].any() and not ob["totals"].any()
    # n == 0 is MMC_OK with zeroed tables
    empty = c_ranked(head, np.zeros((0, 8), np.float32), np.zeros(0, np.int32), levels, 4, 3)
    assert not empty["class_rank_hist"].any() and not empty["hier_hist"].any() and not empty["totals"].any()
    same_bits(good, c_ranked(head, X, y, levels, 4, 3))                             # a good call after the rejected ones


# ---- 9. the Python layer ----

def test_ranking_validate_agrees_with_validate_and_the_restatement():
    from mermaid_classifier_amd import FeatureSet, RankedValidation, ranking_validate, similarity_levels, validate
    pred = _load("head108")
    K = len(pred.classes)
    n = 1000
    rng = np.random.default_rng(30)
    X0 = np.load(GOLDEN / "head108_io.npz")["X"]
    X = np.ascontiguousarray(np.tile(X0, (-(-n // len(X0)), 1))[:n])
    proba, arg = pred._head.predict(X)
    yi = _labels(rng, arg, K)
    labels = np.asarray(pred.classes)[yi]
    category = (np.arange(K) // 27).astype(np.int64)
    S = np.array([0.0, 1 / 3, 1 / 2, 2 / 3])[rng.integers(0, 4, (K, K))]
    S = np.where(category[:, None] == category[None, :], np.maximum(S, 1 / 3), 0.0)
    S = np.maximum(S, S.T)
    np.fill_diagonal(S, 1.0)
    levels, values = similarity_levels(S)
    plain = validate(pred, (X, labels))
    rv = ranking_validate(pred, (X, labels), similarity=S, rows=True)
    for name in ("gt", "est", "scores", "ranks", "p_true", "confusion", "rank_hist"):
        assert np.array_equal(getattr(rv.validation, name), getattr(plain, name)), name
    for name in ("classes", "n", "n_correct", "n_unknown", "n_nonfinite", "nll_q32", "accuracy", "log_loss", "mrr"):
        assert getattr(rv.validation, name) == getattr(plain, name), name
    want_class, want_hier = restate_ranked(proba, yi, K, 10, levels, len(values))
    assert rv.kmax == 10 and np.array_equal(rv.level_values, values)
    assert np.array_equal(rv.class_rank_hist, want_class) and np.array_equal(rv.hier_hist, want_hier)
    want = RankedValidation(plain, want_class, want_hier, values)
    assert rv.by_category(category) == want.by_category(category) and len(rv.by_category(category)) == 4
    assert rv.hierarchical() == want.hierarchical() and rv.scalars() == want.scalars()
    assert sum(r["n_samples"] for r in rv.by_category(category, min_samples=1)) == n
    hier = rv.hierarchical()
    assert hier[0]["hit_exact"] == plain.accuracy and [r["mean_max_similarity"] for r in hier] == sorted(r["mean_max_similarity"] for r in hier)
    # a resident set with one class more than the model goes through a label map; totals only; without a similarity
    fs = FeatureSet(pred.input_dim, list(pred.classes) + ["zz::extra"]).append(X, labels)
    rs = ranking_validate(pred, fs, similarity=S, max_k=3)
    assert not rs.validation.has_rows and rs.validation.nll_q32 == plain.nll_q32 and rs.kmax == 3
    assert np.array_equal(rs.class_rank_hist, rv.class_rank_hist) and np.array_equal(rs.hier_hist, rv.hier_hist[:3])
    bare = ranking_validate(pred, fs)
    assert bare.hier_hist is None and bare.level_values is None and np.array_equal(bare.class_rank_hist, rv.class_rank_hist)
    assert "hierarchical_top_5_mean_similarity" not in bare.scalars() and bare.scalars()["mrr"] == plain.mrr
    two = ranking_validate(pred, [(X[:300], labels[:300]), (X[300:], labels[300:])], similarity=S)   # batches add up
    assert np.array_equal(two.class_rank_hist, rv.class_rank_hist) and np.array_equal(two.hier_hist, rv.hier_hist)
    fs.close()
