"""CPU tests of the taxonomic metric group (``taxonomy.TaxonomicScores``) and of per-category calibration
(``mmc_head_evaluate_categories*``, ``GroupedValidation.category_reliability`` / ``.category_calibration``): the ABI surface, the
argument checks that fire before a device is touched, and the derivations against what the reference's own ``compute_taxonomic`` and
``compute_calibration`` returned on the seeded data of tests/golden/taxonomic_fixture.npz (tests/golden/make_taxonomic_golden.py).
The per-category integer tables come from ``restate_categories`` below, a numpy restatement of the device pass; the GPU tests
(test_gpu_categories.py) compare the kernels with the same function.

Bounds.  Every count and every percent: equal.  The floats -- the four scalars, ``pct_of_errors``, the rounded precision / recall /
f1, and ``ece`` / ``accuracy`` / ``avg_confidence`` of the per-category table: |d| <= 1e-12, the bound test_metrics_host.py uses for
``ece`` (conf_q32 is exact for scores >= 2^-9, and fp64 sums of a few thousand terms in another order err below 1e-14).  NaN equals NaN."""

import numpy as np
import pytest

from conftest import GOLDEN
from test_metrics_host import restate

TOL = 1e-12
MAX_BINS = 20


def restate_categories(g, est, score, category_of_class, n_categories):
    """The category tables of mmc_head_evaluate_categories from per-row values.  ``g`` is the true class of a scored row and -1
    otherwise; ``score`` is float32.  Per category: a stable sort by the 31-bit key (bits(score) << 1) | (est == g), bins over the
    sorted positions np.linspace(0, n, nb + 1, dtype=int) with nb = min(20, max(2, n // 10))."""
    g, est = np.asarray(g, np.int64), np.asarray(est, np.int64)
    score = np.ascontiguousarray(score, np.float32)
    cat = np.asarray(category_of_class, np.int64)
    row_cat = np.where(g >= 0, cat[np.maximum(g, 0)], -1)
    key = (score.view(np.uint32).astype(np.int64) << 1) | (est == g)
    sq = np.rint(np.nan_to_num(score.astype(np.float64)) * 2.0 ** 32).astype(np.int64)   # (a NaN score: the row is not scored)
    out = dict(cat_rows=np.zeros(n_categories, np.int64), cat_n_bins=np.zeros(n_categories, np.int32),
               cat_bin_count=np.zeros((n_categories, MAX_BINS), np.int64), cat_bin_correct=np.zeros((n_categories, MAX_BINS), np.int64),
               cat_bin_conf_q32=np.zeros((n_categories, MAX_BINS), np.int64), cat_bin_conf_min=np.zeros((n_categories, MAX_BINS), np.float32),
               cat_bin_conf_max=np.zeros((n_categories, MAX_BINS), np.float32))
    for c in range(n_categories):
        rows = np.flatnonzero(row_cat == c)
        n = len(rows)
        if n == 0:
            continue
        nb = min(20, max(2, n // 10))
        rows = rows[np.argsort(key[rows], kind="stable")]
        edges = np.linspace(0, n, nb + 1, dtype=int)
        assert np.array_equal(edges, np.arange(nb + 1) * n // nb)
        out["cat_rows"][c], out["cat_n_bins"][c] = n, nb
        for b in range(nb):
            r = rows[edges[b]:edges[b + 1]]
            if len(r):
                out["cat_bin_count"][c, b] = len(r)
                out["cat_bin_correct"][c, b] = (est[r] == g[r]).sum()
                out["cat_bin_conf_q32"][c, b] = sq[r].sum()
                out["cat_bin_conf_min"][c, b], out["cat_bin_conf_max"][c, b] = score[r[0]], score[r[-1]]
    return out


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN / "taxonomic_fixture.npz"))


def _scores_of(fx, gt=None, est=None):
    from mermaid_classifier_amd import TaxonomicScores
    K = len(fx["classes"])
    gt, est = fx["gt"] if gt is None else gt, fx["est"] if est is None else est
    conf = np.bincount(gt.astype(np.int64) * K + est, minlength=K * K).reshape(K, K)
    nodes = fx["nodes"].tolist()
    paths = [[nodes[i] for i in row if i >= 0] for row in fx["class_paths"]]
    gf = [None if i < 0 else fx["gfs"][i].item() for i in fx["gf_of_class"]]
    return TaxonomicScores(conf, paths, gf)


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), what
    gap = float(np.nanmax(np.abs(got - want))) if got.size and not np.isnan(want).all() else 0.0
    print(f"{what}: max |d| = {gap:.3g} (allowed {TOL})")
    assert gap <= TOL, what


# ---- the ABI surface ----

def test_library_and_package_export_the_category_entry_points():
    import ctypes as C
    import re
    from conftest import ROOT
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    header = (ROOT / "include" / "mmc.h").read_text()
    kinds = {"mmc_head*": C.c_void_p, "mmc_featureset*": C.c_void_p, "void*": C.c_void_p, "int64_t": C.c_int64, "int": C.c_int,
             "unsigned": C.c_uint}
    for sym in ("mmc_head_evaluate_categories", "mmc_head_evaluate_categories_set"):
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
    # the category arguments follow the grouped ones
    grouped = re.sub(r"\s+", " ", re.search(r"\bint mmc_head_evaluate_grouped\(([^;]*)\);", header).group(1))
    cats = re.sub(r"\s+", " ", re.search(r"\bint mmc_head_evaluate_categories\(([^;]*)\);", header).group(1))
    assert cats.startswith(grouped[:grouped.index("unsigned flags")])
    tot = np.full(_lib.MMC_EVAL_TOTALS, 9, np.int64)
    rows_out, bins_out = np.full(3, 9, np.int64), np.full((3, 20), 9, np.int64)
    tail = [None, 1, None, 0, 20] + [None] * 11 + [None, 3, rows_out.ctypes.data, None, bins_out.ctypes.data, None, None, None, None]
    assert lib.mmc_head_evaluate_categories(None, None, None, 1, None, 0, None, None, None, None, tot.ctypes.data, None, None, *tail, 0,
                                            None) == _lib.MMC_ERR_ARG
    assert b"head handle is NULL" in lib.mmc_last_error() and not tot.any() and not rows_out.any() and not bins_out.any()
    tot[:] = 9
    assert lib.mmc_head_evaluate_categories_set(None, None, 0, 1, None, 0, None, None, None, None, tot.ctypes.data, None, None, *tail,
                                                None) == _lib.MMC_ERR_ARG
    assert b"head handle is NULL" in lib.mmc_last_error() and not tot.any()
    for name, value in (("MMC_CATEGORY_MAX", 64), ("MMC_CATEGORY_MAX_BINS", 20), ("MMC_CATEGORY_MIN_BINS", 2), ("MMC_CATEGORY_ROWS_PER_BIN", 10)):
        line = re.search(r"#define " + name + r" +(\d+)(.*)", header)
        assert int(line.group(1)) == value == getattr(_lib, name), name
        assert name == "MMC_CATEGORY_MAX" or "calibration.py:137" in line.group(2), name
    import mermaid_classifier_amd as m
    for name in ("TaxonomicScores", "category_bins", "grouped_validate"):
        assert name in m.__all__ and getattr(m, name) is not None, name
    assert [m.category_bins(n) for n in (0, 1, 19, 20, 29, 30, 39, 40, 199, 200, 10 ** 6)] == [0, 2, 2, 2, 2, 3, 3, 4, 19, 20, 20]


# ---- the taxonomic group against the reference's outputs ----

def test_error_attribution_matches_the_reference(fx):
    ea = _scores_of(fx).error_attribution()
    nodes = fx["nodes"].tolist()
    want = [(-int(n), str(None if i < 0 else nodes[i]), None if i < 0 else nodes[i], None if b < 0 else nodes[b], int(n), float(p), int(s))
            for i, b, n, p, s in zip(fx["ea_lca_node"], fx["ea_branch"], fx["ea_error_count"], fx["ea_pct_of_errors"], fx["ea_classes_in_subtree"])]
    got = [(-r["error_count"], str(r["lca_node"]), r["lca_node"], r["branch"], r["error_count"], r["pct_of_errors"], r["classes_in_subtree"])
           for r in ea["rows"]]
    want.sort(key=lambda r: r[:2])
    got.sort(key=lambda r: r[:2])
    assert [r[2:5] + r[6:] for r in got] == [r[2:5] + r[6:] for r in want]
    _close([r[5] for r in got], [r[5] for r in want], "pct_of_errors")
    assert [r["error_count"] for r in ea["rows"]] == sorted((r["error_count"] for r in ea["rows"]), reverse=True)
    assert sum(r["error_count"] for r in ea["rows"]) == int((fx["gt"] != fx["est"]).sum())
    _close(ea["cross_branch_error_rate"], fx["scalar_cross_branch_error_rate"], "cross_branch_error_rate")
    _close(ea["within_branch_error_rate"], fx["scalar_within_branch_error_rate"], "within_branch_error_rate")
    # two classes of one benthic attribute with different growth forms meet in that attribute
    assert any(r["lca_node"] in ("b0", "b5") and r["classes_in_subtree"] == 1 for r in ea["rows"])


def test_equal_error_counts_keep_the_order_of_the_first_cell():
    """The documented tie rule: equal counts stand in the order of the first (g, est) cell, row-major, that produced the node."""
    from mermaid_classifier_amd import TaxonomicScores
    paths = [["t0", "m0", "a"], ["t0", "m0", "b"], ["t0", "c"], ["t1", "d"], ["t1", "e"]]
    conf = np.zeros((5, 5), np.int64)
    conf[0, 3] = 2                         # cross-branch, first cell
    conf[1, 0] = 1                         # m0 ...
    conf[2, 0] = 2                         # t0
    conf[3, 4] = 2                         # t1
    conf[4, 3] = 1                         # t1 again: 3 in all
    conf[1, 0] += 1                        # ... m0: 2
    conf[2, 2] = 7
    ea = TaxonomicScores(conf, paths, [None] * 5).error_attribution()
    assert [(r["lca_node"], r["error_count"]) for r in ea["rows"]] == [("t1", 3), (None, 2), ("m0", 2), ("t0", 2)]
    assert [r["branch"] for r in ea["rows"]] == ["t1", None, "t0", "t0"]
    assert [r["classes_in_subtree"] for r in ea["rows"]] == [2, 0, 2, 3]
    assert ea["cross_branch_error_rate"] == 2 / 9 and ea["within_branch_error_rate"] == 7 / 9
    # the transposed errors meet the nodes in another order
    ea = TaxonomicScores(conf.T.copy(), paths, [None] * 5).error_attribution()
    assert [(r["lca_node"], r["error_count"]) for r in ea["rows"]] == [("t1", 3), ("m0", 2), ("t0", 2), (None, 2)]


def test_top_level_confusion_matches_the_reference(fx):
    tl = _scores_of(fx).top_level_confusion()
    tops = fx["tops"].tolist()
    assert tl["categories"] == [tops[i] for i in fx["tl_categories"]]
    assert tl["categories"][-1] == "t5" and tl["matrix"][-1].sum() == 0         # seen only as a prediction: appended last
    assert tl["percent"].dtype == np.int64 and np.array_equal(tl["percent"], fx["tl_percent"])
    T = len(tops)
    top = fx["top_of_class"].astype(np.int64)
    cm = np.bincount(top[fx["gt"]] * T + top[fx["est"]], minlength=T * T).reshape(T, T)
    order = fx["tl_categories"]
    assert np.array_equal(tl["matrix"], cm[np.ix_(order, order)])
    assert [r["true"] for r in tl["rows"]] == [tops[i] for i in fx["tl_true"]]
    assert [r["predicted"] for r in tl["rows"]] == [tops[i] for i in fx["tl_predicted"]]
    assert [r["row_normalized_pct"] for r in tl["rows"]] == fx["tl_row_normalized_pct"].tolist()
    assert [r["sample_count"] for r in tl["rows"]] == fx["tl_sample_count"].tolist()
    # the float floor: 29 of 100 is 28, as in the reference
    cell = [r for r in tl["rows"] if (r["true"], r["predicted"]) == ("t2", "t0")]
    assert cell == [{"true": "t2", "predicted": "t0", "row_normalized_pct": 28, "sample_count": 29}] and 29 * 100 // 100 == 29


def test_growth_forms_match_the_reference(fx):
    g = _scores_of(fx).growth_forms()
    gfs = fx["gfs"].tolist()
    assert g["labels"] == [gfs[i] for i in fx["gf_rows"]] == [gfs[i] for i in fx["gf_columns"][:-1]] and fx["gf_columns"][-1] == -1
    assert [r["growth_form"] for r in g["table"]] == [gfs[i] for i in fx["gf_growth_form"]]
    assert [r["support"] for r in g["table"]] == fx["gf_support"].tolist()
    for k in ("precision", "recall", "f1"):
        _close([r[k] for r in g["table"]], fx[f"gf_{k}"], f"growth-form {k}")
    assert g["percent"].dtype == np.int64 and np.array_equal(g["percent"], fx["gf_percent"])
    gf = fx["gf_of_class"].astype(np.int64)
    tg, pg = gf[fx["gt"]], gf[fx["est"]]
    L = len(g["labels"])
    col = np.where(pg < 0, L, np.searchsorted(fx["gf_rows"], pg))                  # (gf_rows is 0 .. L-1 here)
    assert fx["gf_rows"].tolist() == list(range(L))
    keep = (tg >= 0) & (pg < L)                                                    # g4 is no label: its predictions are dropped
    want = np.bincount(tg[keep] * (L + 1) + col[keep], minlength=L * (L + 1)).reshape(L, L + 1)
    assert np.array_equal(g["matrix"], want) and ((tg >= 0) & (pg >= L)).any()
    _close(g["gf_accuracy_gf_relevant"], fx["scalar_gf_accuracy_gf_relevant"], "gf_accuracy_gf_relevant")
    _close(g["within_ba_gf_accuracy"], fx["scalar_within_ba_gf_accuracy"], "within_ba_gf_accuracy")


def test_scalars_match_the_reference(fx):
    from mermaid_classifier_amd.taxonomy import SCALAR_NAMES
    sc = _scores_of(fx).scalars()
    assert tuple(sc) == SCALAR_NAMES
    for name in SCALAR_NAMES:
        _close(sc[name], fx[f"scalar_{name}"], name)


def test_tables_without_errors_and_without_growth_forms(fx):
    from mermaid_classifier_amd import TaxonomicScores
    right = _scores_of(fx, est=fx["gt"])
    ea = right.error_attribution()
    assert ea == {"rows": [], "cross_branch_error_rate": 0.0, "within_branch_error_rate": 0.0}
    tl = right.top_level_confusion()
    assert tl["rows"] == [] and tl["categories"] == ["t0", "t1", "t2", "t3", "t4"] and np.array_equal(tl["percent"], np.eye(5, dtype=np.int64) * 100)
    assert right.scalars()["gf_accuracy_gf_relevant"] == 1.0 and right.scalars()["within_ba_gf_accuracy"] == 1.0
    conf = np.array([[3, 1, 0], [0, 2, 2], [1, 0, 5]])
    paths = [["t0", "a"], ["t0", "b"], ["t1", "c"]]
    none = TaxonomicScores(conf, paths, [None, None, None]).growth_forms()
    assert none["gf_accuracy_gf_relevant"] == 0.0 and none["within_ba_gf_accuracy"] == 0.0 and none["table"] == [] and none["labels"] == []
    # every row with a growth form is predicted into another benthic attribute: no row qualifies within BA
    sc = TaxonomicScores(np.array([[0, 4, 0], [0, 3, 0], [0, 0, 2]]), paths, ["g", None, None]).scalars()
    assert sc["gf_accuracy_gf_relevant"] == 0.0 and np.isnan(sc["within_ba_gf_accuracy"])
    # a growth form that is never predicted: precision 0 by the zero-division rule
    g = TaxonomicScores(np.array([[0, 4, 0], [0, 3, 0], [0, 0, 2]]), paths, ["g", None, "h"]).growth_forms()
    assert g["table"] == [{"growth_form": "g", "precision": 0.0, "recall": 0.0, "f1": 0.0, "support": 4},
                          {"growth_form": "h", "precision": 1.0, "recall": 1.0, "f1": 1.0, "support": 2}]
    assert g["matrix"].tolist() == [[0, 0, 4], [0, 2, 0]] and g["percent"].tolist() == [[0, 0, 100], [0, 100, 0]]
    assert np.zeros((0, 0), np.int64).shape == TaxonomicScores(np.zeros((2, 2), np.int64), paths[:2], [None, "g"]).top_level_confusion()["matrix"].shape


def test_taxonomic_argument_errors():
    from mermaid_classifier_amd import TaxonomicScores
    paths = [["t0", "a"], ["t0", "b"]]
    with pytest.raises(ValueError, match="square table of integers"):
        TaxonomicScores(np.zeros((2, 3), np.int64), paths, [None, None])
    with pytest.raises(ValueError, match="square table of integers"):
        TaxonomicScores(np.zeros((2, 2)), paths, [None, None])
    with pytest.raises(ValueError, match="negative count"):
        TaxonomicScores(np.array([[1, -1], [0, 0]]), paths, [None, None])
    with pytest.raises(ValueError, match="must have 2 entries"):
        TaxonomicScores(np.zeros((2, 2), np.int64), paths[:1], [None, None])
    with pytest.raises(ValueError, match="must have 2 entries"):
        TaxonomicScores(np.zeros((2, 2), np.int64), paths, [None])
    with pytest.raises(ValueError, match="at least the class's own benthic attribute"):
        TaxonomicScores(np.zeros((2, 2), np.int64), [["t0"], []], [None, None])


# ---- per-category calibration against the reference's table ----

def _grouped(fx, category_of_class, n_categories):
    from mermaid_classifier_amd import CoverStats, GroupedValidation, Reliability, Validation
    from mermaid_classifier_amd.metrics import category_bins
    K = len(fx["classes"])
    gt, est, scores = fx["gt"], fx["est"], fx["scores"]
    t = restate(gt, est, scores, scores, [len(gt)], None, 0, K, 20)
    conf = np.bincount(gt.astype(np.int64) * K + est, minlength=K * K).reshape(K, K)
    val = Validation(fx["classes"].tolist(), None, None, None, None, None, conf, np.zeros(K), len(gt), int((gt == est).sum()), 0, 0,
                     int(t["nll_q32"].sum()))
    c = restate_categories(gt, est, scores, np.where(np.asarray(category_of_class) < 0, -1, category_of_class), n_categories)
    assert [category_bins(int(n)) for n in c["cat_rows"]] == c["cat_n_bins"].tolist()
    rel = {i: Reliability(*(c[k][i, :nb] for k in ("cat_bin_count", "cat_bin_correct", "cat_bin_conf_q32", "cat_bin_conf_min", "cat_bin_conf_max")))
           for i, nb in enumerate(c["cat_n_bins"]) if c["cat_rows"][i] > 0}
    return GroupedValidation(val, CoverStats(t["cover"], t["n_images_used"]), None,
                             Reliability(t["bin_count"], t["bin_correct"], t["bin_conf_q32"], t["bin_conf_min"], t["bin_conf_max"]),
                             t["support"], t["nll_q32"], t["score_q32"], category_of_class, rel), c


def test_category_calibration_matches_the_reference(fx):
    gv, c = _grouped(fx, fx["top_of_class"], 6)
    assert c["cat_rows"].tolist() == [2200, 1643, 100, 35, 22, 0] and c["cat_n_bins"].tolist() == [20, 20, 10, 3, 2, 0]
    assert sorted(gv.category_reliability) == [0, 1, 2, 3, 4]
    rows = gv.category_calibration()
    assert [r["category"] for r in rows] == fx["pc_category"].tolist() and 4 not in [r["category"] for r in rows]    # 22 rows: below 30
    assert [r["n_samples"] for r in rows] == fx["pc_n_samples"].tolist()
    for k in ("ece", "accuracy", "avg_confidence"):
        _close([r[k] for r in rows], fx[f"pc_{k}"], f"per-category {k}")
    assert sorted(r["category"] for r in gv.category_calibration(min_samples=1)) == [0, 1, 2, 3, 4]
    assert len(gv.category_reliability[3].bins) == 3 and len(gv.category_reliability[2].bins) == 10
    _close(gv.reliability.ece, fx["scalar_ece"], "overall ece")


def test_a_class_without_a_category_and_equal_ece():
    from mermaid_classifier_amd import CoverStats, GroupedValidation, Reliability, Validation
    score = np.array([0.9, 0.3, 0.5, 0.7, 0.5, 1.0, 0.25, 0.75], np.float32)
    g, est = np.array([0, 1, 2, 0, 1, 2, 3, 3]), np.array([0, 1, 0, 0, 1, 2, 3, 0])
    cat = np.array([1, 1, -5, 0])                                                  # class 2 belongs to no category
    c = restate_categories(g, est, score, np.where(cat < 0, -1, cat), 2)
    assert c["cat_rows"].tolist() == [2, 4] and c["cat_n_bins"].tolist() == [2, 2] and c["cat_bin_count"].sum() == 6
    assert c["cat_bin_count"][1, :3].tolist() == [2, 2, 0] and c["cat_bin_conf_min"][1, :2].tolist() == [np.float32(0.3), np.float32(0.7)]
    t = restate(g, est, score, score, [8], None, 0, 4, 20)
    conf = np.bincount(g * 4 + est, minlength=16).reshape(4, 4)
    val = Validation(list("abcd"), None, None, None, None, None, conf, np.zeros(4), 8, 6, 0, 0, int(t["nll_q32"].sum()))
    cols = ("cat_bin_count", "cat_bin_correct", "cat_bin_conf_q32", "cat_bin_conf_min", "cat_bin_conf_max")
    main = Reliability(t["bin_count"], t["bin_correct"], t["bin_conf_q32"], t["bin_conf_min"], t["bin_conf_max"])

    def gv(rel):
        return GroupedValidation(val, CoverStats(t["cover"], 1), None, main, t["support"], t["nll_q32"], t["score_q32"], cat, rel)

    rows = gv({i: Reliability(*(c[k][i, :2] for k in cols)) for i in (0, 1)}).category_calibration(min_samples=1)
    assert [(r["category"], r["n_samples"]) for r in sorted(rows, key=lambda r: r["category"])] == [(0, 2), (1, 4)]
    assert rows[0]["ece"] >= rows[1]["ece"] and sum(r["n_samples"] for r in rows) == 6
    by_id = {r["category"]: r for r in rows}
    assert by_id[0]["accuracy"] == 0.5 and by_id[1]["accuracy"] == 1.0
    assert by_id[0]["avg_confidence"] == pytest.approx(0.5, abs=1e-9) and by_id[1]["avg_confidence"] == pytest.approx(0.6, abs=1e-7)
    # equal ece: the smaller category id first
    same = Reliability(c["cat_bin_count"][0, :2], c["cat_bin_correct"][0, :2], c["cat_bin_conf_q32"][0, :2], c["cat_bin_conf_min"][0, :2],
                       c["cat_bin_conf_max"][0, :2])
    val2 = Validation(list("abcd"), None, None, None, None, None, np.array([[1, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 1]]),
                      np.zeros(4), 4, 2, 0, 0, 0)
    two = GroupedValidation(val2, CoverStats(t["cover"], 1), None, main, np.array([2, 0, 0, 2]), np.zeros(4, np.int64),
                            np.array([t["score_q32"][3], 0, 0, t["score_q32"][3]]), np.array([1, -1, -1, 0]), {1: same, 0: same})
    assert [r["category"] for r in two.category_calibration(min_samples=1)] == [0, 1]
    with pytest.raises(ValueError, match="the bins hold 2 rows, the per-class sums 4"):
        gv({0: same, 1: same}).category_calibration(min_samples=1)
    with pytest.raises(ValueError, match="no category tables"):
        GroupedValidation(val, CoverStats(t["cover"], 1), None, main, t["support"], t["nll_q32"], t["score_q32"]).category_calibration()
    with pytest.raises(ValueError, match="go together"):
        GroupedValidation(val, CoverStats(t["cover"], 1), None, main, t["support"], t["nll_q32"], t["score_q32"], cat, None)


def test_category_argument_errors_come_before_the_device():
    from mermaid_classifier_amd import grouped_validate
    from test_validation_host import _predictor
    pred = _predictor()
    X = np.zeros((6, 8), np.float32)
    y = ["c0", "c1", "c3", "c0", "c2", "c1"]
    with pytest.raises(ValueError, match="category_of_class must be 4 integers"):
        grouped_validate(pred, (X, y), [3, 3], category_of_class=[0, 1, 0])
    with pytest.raises(ValueError, match="category_of_class must be 4 integers"):
        grouped_validate(pred, (X, y), [3, 3], category_of_class=[0.0, 1.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="category_of_class must be 4 integers"):
        grouped_validate(pred, (X, y), [3, 3], category_of_class=[[0, 1, 0, 1]])
    with pytest.raises(ValueError, match="category ids must lie below 64; got 64"):
        grouped_validate(pred, (X, y), [3, 3], category_of_class=[0, 1, 64, 1])
    with pytest.raises(ValueError, match="names no category"):
        grouped_validate(pred, (X, y), [3, 3], category_of_class=[-1, -1, -2, -1])
    with pytest.raises(ValueError, match="image_sizes add up to 5"):               # the grouped checks still come first
        grouped_validate(pred, (X, y), [2, 3], category_of_class=[0, 1, 0, 1])
