"""CPU tests of ranking validation (``mmc_head_evaluate_ranked*``, ``ranking.ranking_validate``): the ABI surface, the argument
checks that fire before a device is touched, ``similarity_levels``, and the derivations of ``RankedValidation`` against what the
reference's own ``compute_ranking`` returned on the seeded data of tests/golden/ranking_fixture.npz
(tests/golden/make_ranking_golden.py).  The raw tables come from ``restate_ranked`` below, a numpy restatement of the device pass;
the GPU tests (test_gpu_ranking.py) compare the kernel with the same function.

Bounds.  Category order, ``n_samples`` and every ``hit_*`` column: equal (a count over the same n).  ``mrr``, ``top_k`` and
``mean_max_similarity``: |d| <= 1e-12 (fp64 sums of at most 3 000 terms in [0, 1] in another order err below 3000 * 2^-53 < 4e-13
before the division by n)."""

import ctypes as C
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT


def restate_ranked(proba, g, K, kmax, levels, n_levels=None):
    """The two tables of mmc_head_evaluate_ranked from a probability matrix.  ``proba`` float32 [n, K]; ``g`` the true class of a
    scored row, -1 otherwise; ``levels`` uint8 [K, K] (row = true class) or None.  The order of a row is the descending order of
    ``topk_key`` = (float bits << 32) | (0xFFFFFFFF - class): score descending, equal scores in class order.
    -> (class_rank_hist [K, K], hier_hist [kmax, n_levels] or None), int64."""
    P = np.ascontiguousarray(proba, np.float32)
    g = np.asarray(g, np.int64)
    assert P.shape == (len(g), K)
    ok = g >= 0
    P, g = P[ok], g[ok]
    key = (P.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(K, dtype=np.uint64))[None, :]
    order = np.argsort(key, axis=1)[:, ::-1]                      # (keys are distinct: no tie left to a sort's stability)
    rank = 1 + np.argmax(order == g[:, None], axis=1) if len(g) else np.zeros(0, np.int64)
    class_hist = np.bincount(g * K + rank - 1, minlength=K * K).reshape(K, K).astype(np.int64)
    if levels is None:
        return class_hist, None
    levels = np.asarray(levels)
    assert levels.shape == (K, K) and levels.dtype == np.uint8
    n_levels = int(levels.max()) + 1 if n_levels is None else n_levels
    m = np.maximum.accumulate(levels[g[:, None], order[:, :kmax]].astype(np.int64), axis=1)
    hier = np.stack([np.bincount(m[:, j], minlength=n_levels) for j in range(kmax)]).astype(np.int64)
    return class_hist, hier


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN / "ranking_fixture.npz"))


@pytest.fixture(scope="module")
def ranked(fx):
    """RankedValidation built from the restatement's tables on the fixture's probabilities (max_k = 10)."""
    from mermaid_classifier_amd import RankedValidation, Validation, similarity_levels
    from test_validation_host import check_rows
    P, gt = fx["proba"], fx["gt"]
    K = P.shape[1]
    levels, values = similarity_levels(fx["similarity"])
    class_hist, hier = restate_ranked(P, gt, K, 10, levels, len(values))
    rows = check_rows(P, gt)
    val = Validation(fx["classes"].tolist(), None, None, None, None, None, rows["confusion"], rows["rank_hist"], len(gt), rows["n_correct"], 0, 0,
                     rows["nll_q32"])
    return RankedValidation(val, class_hist, hier, values)


# ---- the ABI surface ----

def test_library_and_package_export_the_ranked_entry_points():
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    header = (ROOT / "include" / "mmc.h").read_text()
    kinds = {"mmc_head*": C.c_void_p, "mmc_featureset*": C.c_void_p, "void*": C.c_void_p, "int64_t": C.c_int64, "int": C.c_int,
             "unsigned": C.c_uint}
    for sym in ("mmc_head_evaluate_ranked", "mmc_head_evaluate_ranked_set"):
        assert sym in _lib.SYMBOLS and hasattr(lib, sym), sym
        decl = re.search(r"\bint " + sym + r"\(([^;]*)\);", header).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl)
        want = []
        for arg in decl.split(","):
            words = arg.replace("const ", "").split()
            typ = words[0] if "*" not in arg and "[" not in arg else ("void*" if words[0] not in ("mmc_head*", "mmc_featureset*") else words[0])
            want.append(kinds[typ])
        fn = getattr(lib, sym)
        assert fn.restype is C.c_int and list(fn.argtypes) == want, sym
    # a NULL handle: MMC_ERR_ARG, and what the arguments size (totals, kmax x n_levels) is zeroed
    tot, hier = np.full(_lib.MMC_EVAL_TOTALS, 9, np.int64), np.full((3, 4), 9, np.int64)
    sim = np.zeros((5, 5), np.uint8)
    extra = [sim.ctypes.data, 4, 3, None, hier.ctypes.data]
    assert lib.mmc_head_evaluate_ranked(None, None, None, 1, None, 0, None, None, None, None, tot.ctypes.data, None, None, *extra, 0,
                                        None) == _lib.MMC_ERR_ARG
    assert b"head handle is NULL" in lib.mmc_last_error() and not tot.any() and not hier.any()
    tot[:], hier[:] = 9, 9
    assert lib.mmc_head_evaluate_ranked_set(None, None, 0, 1, None, 0, None, None, None, None, tot.ctypes.data, None, None, *extra,
                                            None) == _lib.MMC_ERR_ARG
    assert b"head handle is NULL" in lib.mmc_last_error() and not tot.any() and not hier.any()
    assert int(re.search(r"#define MMC_RANKED_MAX_K (\d+)", header).group(1)) == 16 == _lib.MMC_RANKED_MAX_K
    import mermaid_classifier_amd as m
    from mermaid_classifier_amd import ranking
    assert ranking.MAX_K == _lib.MMC_RANKED_MAX_K
    for name in ("ranking_validate", "RankedValidation", "similarity_levels"):
        assert name in m.__all__ and getattr(m, name) is not None, name


# ---- similarity_levels ----

def test_similarity_levels_round_trip_and_limits(fx):
    from mermaid_classifier_amd import similarity_levels
    S = fx["similarity"]
    levels, values = similarity_levels(S)
    assert levels.dtype == np.uint8 and levels.shape == S.shape and levels.flags["C_CONTIGUOUS"] and values.dtype == np.float64
    assert values.tolist() == [0.0, 1 / 3, 1 / 2, 2 / 3, 1.0]                        # ascending, exact
    assert np.array_equal(values[levels], S)                                        # the round trip is exact
    assert np.array_equal(levels < levels.T, S < S.T)                               # monotone codes
    one = similarity_levels(np.full((3, 3), 0.25))
    assert one[1].tolist() == [0.25] and not one[0].any()
    S256 = ((np.arange(400) % 256) * (1 / 3)).reshape(20, 20)                       # 256 distinct values, 144 of them twice
    lv, vals = similarity_levels(S256)
    assert len(vals) == 256 and np.array_equal(vals[lv], S256)
    S257 = S256.copy()
    S257[19, 19] = -1.0
    with pytest.raises(ValueError, match="257 distinct values: at most 256"):
        similarity_levels(S257)
    Sn = S.copy()
    Sn[2, 3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        similarity_levels(Sn)
    for bad in (np.zeros((3, 4)), np.zeros(9), np.zeros((2, 2, 2)), np.zeros((0, 0))):
        with pytest.raises(ValueError, match="K x K"):
            similarity_levels(bad)


# ---- the restatement on rows made by hand ----

def test_restatement_orders_ties_by_class_and_skips_unscored_rows():
    P = np.array([[0.1, 0.4, 0.4, 0.1],      # order 1 2 0 3
                  [0.25, 0.25, 0.25, 0.25],  # order 0 1 2 3
                  [0.7, 0.1, 0.1, 0.1],      # unscored
                  [0.0, 0.2, 0.3, 0.5]], np.float32)   # order 3 2 1 0
    g = np.array([2, 3, -1, 0])
    levels = np.array([[3, 0, 1, 2], [0, 3, 1, 0], [0, 1, 3, 0], [2, 0, 0, 3]], np.uint8)
    ch, hh = restate_ranked(P, g, 4, 3, levels)
    want = np.zeros((4, 4), np.int64)
    want[2, 1] = want[3, 3] = want[0, 3] = 1
    assert np.array_equal(ch, want)
    # row 0 (g = 2): levels of 1, 2, 0 = 1, 3, 0 -> running 1, 3, 3; row 1 (g = 3): 2, 0, 0 -> 2, 2, 2; row 3 (g = 0): 2, 1, 0 -> 2, 2, 2
    assert hh.tolist() == [[0, 1, 2, 0], [0, 0, 2, 1], [0, 0, 2, 1]]
    assert restate_ranked(P, g, 4, 3, None)[1] is None
    ch0, hh0 = restate_ranked(P, np.full(4, -1), 4, 2, levels, 5)
    assert not ch0.any() and hh0.shape == (2, 5) and not hh0.any()


# ---- the derivations against the reference's outputs ----

def test_by_category_matches_per_category_topk(fx, ranked):
    rows = ranked.by_category(fx["category_of_class"])
    assert [r["category"] for r in rows] == fx["cat_category"].tolist()             # by top_1 descending; the 24-row category is out
    assert [r["n_samples"] for r in rows] == fx["cat_n_samples"].tolist()
    assert 3 not in [r["category"] for r in rows] and len(rows) == 3
    assert list(rows[0]) == ["category", "n_samples", "mrr", "top_1", "top_3", "top_5", "top_10"]
    for k in ("mrr", "top_1", "top_3", "top_5", "top_10"):
        gap = np.abs(np.array([r[k] for r in rows]) - fx[f"cat_{k}"]).max()
        print(f"per category {k}: max |d| = {gap:.3g} (allowed 1e-12)")
        assert gap <= 1e-12, k
    # the small category comes back with a lower bar, with its own exact shares
    low = ranked.by_category(fx["category_of_class"], ks=(1, 2), min_samples=1)
    small = [r for r in low if r["category"] == 3]
    m = np.isin(fx["gt"], np.flatnonzero(fx["category_of_class"] == 3))
    assert len(low) == 4 and small[0]["n_samples"] == int(m.sum()) == 24 and set(small[0]) == {"category", "n_samples", "mrr", "top_1", "top_2"}
    assert [r["top_1"] for r in low] == sorted((r["top_1"] for r in low), reverse=True)
    # classes left out with a negative id
    cat = fx["category_of_class"].copy()
    cat[cat == 0] = -1
    assert sorted(r["category"] for r in ranked.by_category(cat)) == [1, 2]
    with pytest.raises(ValueError, match="must be 12 integers"):
        ranked.by_category([0, 1])
    with pytest.raises(ValueError, match="must be 12 integers"):
        ranked.by_category(np.zeros(12))
    with pytest.raises(ValueError, match="every k must be an integer >= 1"):
        ranked.by_category(fx["category_of_class"], ks=(0,))


def test_hierarchical_matches_hierarchical_topk(fx, ranked):
    rows = ranked.hierarchical()
    assert [r["k"] for r in rows] == fx["hier_k"].tolist() == [1, 3, 5, 10]
    assert list(rows[0]) == ["k", "mean_max_similarity", "hit_exact", "hit_sibling_0.75", "hit_family_0.5"]
    for k in ("hit_exact", "hit_sibling_0.75", "hit_family_0.5"):
        assert [r[k] for r in rows] == fx[f"hier_{k}"].tolist(), k
    gap = np.abs(np.array([r["mean_max_similarity"] for r in rows]) - fx["hier_mean_max_similarity"]).max()
    print(f"hierarchical mean_max_similarity: max |d| = {gap:.3g} (allowed 1e-12)")
    assert gap <= 1e-12
    assert ranked.kmax == 10
    # a k above kmax answers with kmax, as the reference's sims[:k]
    assert ranked.hierarchical(ks=(12,))[0]["mean_max_similarity"] == rows[3]["mean_max_similarity"]
    # top-1 exact hits are the correct rows
    assert rows[0]["hit_exact"] == ranked.validation.n_correct / ranked.validation.n
    other = ranked.hierarchical(ks=(2,), thresholds=((1 / 3, "any"),))
    assert list(other[0]) == ["k", "mean_max_similarity", "any"] and 0 < other[0]["any"] <= 1


def test_scalars_match_the_reference(fx, ranked):
    sc = ranked.scalars()
    names = ("top_1_accuracy", "top_3_accuracy", "top_5_accuracy", "top_10_accuracy", "mrr", "hierarchical_top_5_mean_similarity")
    assert tuple(sc) == names
    for name in names:
        gap = abs(sc[name] - float(fx[f"scalar_{name}"]))
        print(f"{name}: |d| = {gap:.3g} (allowed 1e-12)")
        assert gap <= 1e-12, name
    from mermaid_classifier_amd import RankedValidation
    bare = RankedValidation(ranked.validation, ranked.class_rank_hist)
    assert bare.hier_hist is None and bare.level_values is None and bare.kmax == 0
    assert "hierarchical_top_5_mean_similarity" not in bare.scalars() and bare.scalars()["mrr"] == sc["mrr"]
    with pytest.raises(ValueError, match="no hierarchical table"):
        bare.hierarchical()
    assert np.array_equal(ranked.class_rank_hist.sum(0), ranked.validation.rank_hist)
    with pytest.raises(ValueError, match="expected"):
        RankedValidation(ranked.validation, np.zeros((3, 3)))
    with pytest.raises(ValueError, match="both or neither"):
        RankedValidation(ranked.validation, ranked.class_rank_hist, ranked.hier_hist)
    with pytest.raises(ValueError, match="does not fit"):
        RankedValidation(ranked.validation, ranked.class_rank_hist, np.zeros((10, 4)), ranked.level_values)


# ---- argument checks ----

def test_ranking_validate_argument_errors_come_before_the_device():
    from mermaid_classifier_amd import FeatureSet, ranking_validate
    from test_validation_host import _predictor
    pred = _predictor()
    X = np.zeros((6, 8), np.float32)
    y = ["c0", "c1", "c3", "c0", "c2", "c1"]
    S = np.eye(4)
    for bad in (0, 17, 2.5, True, -3, None):
        with pytest.raises(ValueError, match=r"max_k must be an integer in \[1, 16\]"):
            ranking_validate(pred, (X, y), similarity=S, max_k=bad)
    with pytest.raises(ValueError, match=r"similarity has shape \(3, 3\), the model has 4 classes"):
        ranking_validate(pred, (X, y), similarity=np.eye(3))
    with pytest.raises(ValueError, match="K x K"):
        ranking_validate(pred, (X, y), similarity=np.zeros((4, 5)))
    with pytest.raises(ValueError, match="NaN"):
        ranking_validate(pred, (X, y), similarity=S * np.nan)
    with pytest.raises(ValueError, match="rows must be True or False"):
        ranking_validate(pred, (X, y), rows=1)
    with pytest.raises(ValueError, match="X has 9 features, expected 8"):
        ranking_validate(pred, (np.zeros((6, 9), np.float32), y))
    with pytest.raises(ValueError, match=r"Labels \['zz'\] are not in the model's classes"):
        ranking_validate(pred, (X, ["c0", "zz", "c1", "c0", "c0", "c0"]), similarity=S)
    with pytest.raises(ValueError, match="no rows"):
        ranking_validate(pred, (np.zeros((0, 8), np.float32), []))
    with pytest.raises(ValueError, match="must be a CalibratedMLP or a Predictor"):
        ranking_validate(object(), (X, y))
    with pytest.raises(ValueError, match="the feature set has 9 features, expected 8"):
        ranking_validate(pred, FeatureSet(9, ["c0", "c1"]))
    with pytest.raises(ValueError, match="no rows"):
        ranking_validate(pred, FeatureSet(8, ["c0", "c1"]))
