"""CPU tests of grouped validation (``mmc_head_evaluate_grouped*``, ``metrics.grouped_validate``): the ABI surface, the argument
checks that fire before a device is touched, and the derivations of ``CoverStats`` / ``SourceStats`` / ``Reliability`` /
``by_class`` against what the reference's own ``compute_cover``, ``compute_per_source`` and ``_adaptive_ece`` returned on the seeded
data of tests/golden/metrics_fixture.npz (tests/golden/make_metrics_golden.py).  The raw tables come from ``restate`` below, a numpy
restatement of the device pass; the GPU tests (test_gpu_metrics.py) compare the kernels with the same function.

Bounds.  Cover percentages and R^2: |d| <= 1e-9 (the fp64 reordering error over 300 images is below 1e-13: margin, not slack).
Per-source columns: equal after the reference's rounding to 4 decimals (the generator keeps every value 1e-9 away from a rounding
boundary).  ECE and bin means: |d| <= 1e-12 (conf_q32 is exact for scores >= 2^-9 and pairwise fp64 summation errs below 1e-14).
count, conf_min, conf_max: equal."""

import numpy as np
import pytest

from conftest import GOLDEN

COVER_J = ("sum t", "sum p", "sum (p-t)", "sum (p-t)^2", "sum |p-t|", "min t", "max t", "sum (t-tbar)^2")


def restate(g, est, score, p_true, image_sizes, source_of_image, n_sources, K, n_bins):
    """The tables of mmc_head_evaluate_grouped from per-row values.  ``g`` is the true class of a scored row and -1 otherwise;
    ``score`` / ``p_true`` are float32.  -> dict; ``cover_abs`` holds, per cover sum, the sum of the absolute terms (the scale of its
    rounding error)."""
    g, est = np.asarray(g, np.int64), np.asarray(est, np.int64)
    score, p_true = np.asarray(score, np.float32), np.asarray(p_true, np.float32)
    sizes = np.asarray(image_sizes, np.int64)
    n_images = len(sizes)
    ok = g >= 0
    image = np.repeat(np.arange(n_images), sizes)[ok]
    gs, es, ss, ps = g[ok], est[ok], score[ok], p_true[ok]
    nll = np.rint(-np.log(np.clip(ps.astype(np.float64), 1e-15, 1.0)) * 2.0 ** 32).astype(np.int64)
    sq = np.rint(ss.astype(np.float64) * 2.0 ** 32).astype(np.int64)
    out = dict(support=np.bincount(gs, minlength=K).astype(np.int64))
    out["nll_q32"] = np.array([nll[gs == c].sum() for c in range(K)], np.int64)
    out["score_q32"] = np.array([sq[gs == c].sum() for c in range(K)], np.int64)
    if n_sources:
        src = np.asarray(source_of_image, np.int64)[image]
        out["source_confusion"] = np.bincount((src * K + gs) * K + es, minlength=n_sources * K * K).reshape(n_sources, K, K).astype(np.int64)
    # cover
    true_cnt = np.bincount(image * K + gs, minlength=n_images * K).reshape(n_images, K)
    pred_cnt = np.bincount(image * K + es, minlength=n_images * K).reshape(n_images, K)
    points = np.bincount(image, minlength=n_images)
    used = points > 0
    cover, cover_abs = np.zeros((K, 8)), np.zeros((K, 8))
    if used.any():
        t = true_cnt[used] / points[used, None].astype(np.float64)
        p = pred_cnt[used] / points[used, None].astype(np.float64)
        d = p - t
        dev = t - t.sum(0) / used.sum()
        cover = np.stack([t.sum(0), p.sum(0), d.sum(0), (d * d).sum(0), np.abs(d).sum(0), t.min(0), t.max(0), (dev * dev).sum(0)], 1)
        cover_abs = np.stack([t.sum(0), p.sum(0), np.abs(d).sum(0), (d * d).sum(0), np.abs(d).sum(0), t.min(0) * 0, t.max(0) * 0,
                              (dev * dev).sum(0)], 1)
    out.update(cover=cover, cover_abs=cover_abs, n_images_used=int(used.sum()))
    # reliability: (score, correct) order, bins over the sorted positions b n / n_bins
    correct = es == gs
    order = np.lexsort((correct, ss))
    ss, correct, sq = ss[order], correct[order], sq[order]
    n = len(ss)
    edges = np.arange(n_bins + 1) * n // n_bins
    cnt, cor, cq = np.zeros(n_bins, np.int64), np.zeros(n_bins, np.int64), np.zeros(n_bins, np.int64)
    cmin, cmax = np.zeros(n_bins, np.float32), np.zeros(n_bins, np.float32)
    for b in range(n_bins):
        lo, hi = edges[b], edges[b + 1]
        if hi > lo:
            cnt[b], cor[b], cq[b], cmin[b], cmax[b] = hi - lo, correct[lo:hi].sum(), sq[lo:hi].sum(), ss[lo], ss[hi - 1]
    out.update(bin_count=cnt, bin_correct=cor, bin_conf_q32=cq, bin_conf_min=cmin, bin_conf_max=cmax)
    return out


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN / "metrics_fixture.npz"))


@pytest.fixture(scope="module")
def tables(fx):
    K = len(fx["classes"])
    p_true = np.where(fx["est"] == fx["gt"], fx["scores"], np.float32(0.05)).astype(np.float32)
    return {nb: restate(fx["gt"], fx["est"], fx["scores"], p_true, fx["image_sizes"], fx["source_of_image"], 4, K, nb) for nb in (20, 7)}


# ---- the ABI surface ----

def test_library_and_package_export_the_grouped_entry_points():
    import re
    from conftest import ROOT
    from mermaid_classifier_amd import _lib
    import ctypes as C
    lib = _lib.lib()
    header = (ROOT / "include" / "mmc.h").read_text()
    kinds = {"mmc_head*": C.c_void_p, "mmc_featureset*": C.c_void_p, "void*": C.c_void_p, "int64_t": C.c_int64, "int": C.c_int,
             "unsigned": C.c_uint}
    for sym in ("mmc_head_evaluate_grouped", "mmc_head_evaluate_grouped_set"):
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
    tot = np.full(_lib.MMC_EVAL_TOTALS, 9, np.int64)
    grouped = [None, 1, None, 0, 20] + [None] * 11
    assert lib.mmc_head_evaluate_grouped(None, None, None, 1, None, 0, None, None, None, None, tot.ctypes.data, None, None, *grouped, 0,
                                         None) == _lib.MMC_ERR_ARG
    assert b"head handle is NULL" in lib.mmc_last_error() and not tot.any()
    tot[:] = 9
    assert lib.mmc_head_evaluate_grouped_set(None, None, 0, 1, None, 0, None, None, None, None, tot.ctypes.data, None, None, *grouped,
                                             None) == _lib.MMC_ERR_ARG
    assert b"head handle is NULL" in lib.mmc_last_error() and not tot.any()
    assert (_lib.MMC_GROUPED_MAX_BINS, _lib.MMC_COVER_SUMS) == (64, 8)
    for name, value in (("MMC_GROUPED_MAX_BINS", 64), ("MMC_GROUPED_MAX_SOURCE_CELLS", 1 << 26), ("MMC_GROUPED_MAX_COVER_CELLS", 1 << 28),
                        ("MMC_COVER_SUMS", 8)):
        assert int(re.search(r"#define " + name + r" (\d+)", header).group(1)) == value == getattr(_lib, name)
    import mermaid_classifier_amd as m
    for name in ("grouped_validate", "GroupedValidation", "CoverStats", "SourceStats", "Reliability"):
        assert name in m.__all__ and getattr(m, name) is not None, name
    from mermaid_classifier_amd import build
    assert "metrics.hip" in build.SOURCES and all((build.CSRC / d).is_file() for d in build.SOURCES["metrics.hip"])


# ---- argument checks ----

def test_grouped_validate_argument_errors_come_before_the_device():
    from mermaid_classifier_amd import FeatureSet, grouped_validate
    from test_validation_host import _predictor
    pred = _predictor()
    X = np.zeros((6, 8), np.float32)
    y = ["c0", "c1", "c3", "c0", "c2", "c1"]
    with pytest.raises(ValueError, match="image_sizes add up to 5, the data has 6 rows"):
        grouped_validate(pred, (X, y), [2, 3])
    with pytest.raises(ValueError, match=r"image_sizes\[1\] = 0: every image holds at least one point"):
        grouped_validate(pred, (X, y), [3, 0, 3])
    with pytest.raises(ValueError, match="every image holds at least one point"):
        grouped_validate(pred, (X, y), [7, -1])
    with pytest.raises(ValueError, match="non-empty 1-D sequence of integers"):
        grouped_validate(pred, (X, y), [])
    with pytest.raises(ValueError, match="non-empty 1-D sequence of integers"):
        grouped_validate(pred, (X, y), [3.0, 3.0])
    with pytest.raises(ValueError, match=r"source_of_image has shape \(3,\), expected \(2,\)"):
        grouped_validate(pred, (X, y), [3, 3], source_of_image=[0, 1, 0])
    with pytest.raises(ValueError, match="source_of_image must hold integers >= 0"):
        grouped_validate(pred, (X, y), [3, 3], source_of_image=[0, -1])
    for bad in (0, 65, 2.5, True, -3):
        with pytest.raises(ValueError, match="n_bins must be an integer in"):
            grouped_validate(pred, (X, y), [3, 3], n_bins=bad)
    with pytest.raises(ValueError, match="rows must be True or False"):
        grouped_validate(pred, (X, y), [3, 3], rows=1)
    with pytest.raises(ValueError, match="X has 9 features, expected 8"):
        grouped_validate(pred, (np.zeros((6, 9), np.float32), y), [3, 3])
    with pytest.raises(ValueError, match=r"Labels \['zz'\] are not in the model's classes"):
        grouped_validate(pred, (X, ["c0", "zz", "c1", "c0", "c0", "c0"]), [3, 3])
    with pytest.raises(ValueError, match="no rows"):
        grouped_validate(pred, (np.zeros((0, 8), np.float32), []), [1])
    with pytest.raises(ValueError, match="FeatureSet or one"):
        grouped_validate(pred, [(X, y), (X, y)][:1] * 3, [3, 3])
    with pytest.raises(ValueError, match="must be a CalibratedMLP or a Predictor"):
        grouped_validate(object(), (X, y), [3, 3])
    with pytest.raises(ValueError, match="the feature set has 9 features, expected 8"):
        grouped_validate(pred, FeatureSet(9, ["c0", "c1"]), [1])
    with pytest.raises(ValueError, match="no rows"):
        grouped_validate(pred, FeatureSet(8, ["c0", "c1"]), [1])
    with pytest.raises(ValueError, match=r"4 sources x 4 x 4|per-source cells"):
        grouped_validate(pred, (X, y), [3, 3], source_of_image=[0, (1 << 26) // 16])


def test_one_grouped_call_covers_at_most_a_whole_split(monkeypatch):
    from mermaid_classifier_amd import grouped_validate, metrics
    from test_validation_host import _predictor
    monkeypatch.setattr(metrics, "MAX_ROWS_PER_CALL", 5)
    with pytest.raises(ValueError, match="6 rows: one grouped call covers a whole split of at most 5 rows"):
        grouped_validate(_predictor(), (np.zeros((6, 8), np.float32), ["c0"] * 6), [6])


# ---- the derivations against the reference's outputs ----

def test_cover_table_and_scalars_match_compute_cover(fx, tables):
    from mermaid_classifier_amd import CoverStats
    t = tables[20]
    assert t["n_images_used"] == len(fx["image_sizes"]) == 300
    cs = CoverStats(t["cover"], t["n_images_used"])
    tab = cs.table()
    assert np.array_equal(tab["class"], fx["cover_class"])                       # classes in gt or est, by mean true cover
    assert 8 not in tab["class"] and 7 in tab["class"] and len(tab["class"]) == 8
    for k in ("mean_true_cover_pct", "bias_pct", "rmse_pct", "mae_pct", "r_squared"):
        want = fx[f"cover_{k}"]
        assert np.array_equal(np.isnan(tab[k]), np.isnan(want)), k
        gap = np.nanmax(np.abs(tab[k] - want))
        print(f"cover {k}: max |d| = {gap:.3g} (allowed 1e-9)")
        assert gap <= 1e-9, k
    assert np.isnan(tab["r_squared"][tab["class"] == 7]).all()                   # never in gt: constant true cover
    sc = cs.scalars()
    for name in ("cover_mean_abs_bias_pct", "cover_mean_rmse_pct", "cover_mean_mae_pct", "cover_median_r_squared"):
        assert abs(sc[name] - float(fx[f"scalar_{name}"])) <= 1e-9, name


def test_cover_branches():
    from mermaid_classifier_amd import CoverStats
    names = ("cover_mean_abs_bias_pct", "cover_mean_rmse_pct", "cover_mean_mae_pct", "cover_median_r_squared")
    # no image with a scored row: an empty table and the all-zero scalars
    cs = CoverStats(np.zeros((4, 8)), 0)
    assert all(len(v) == 0 for v in cs.table().values()) and cs.scalars() == dict.fromkeys(names, 0.0)
    # no class above 0.5 % mean true cover: the all-zero fallback (cover.py:112-120)
    K, n_images = 400, 3
    g = np.arange(1200) % K
    r = restate(g, (g + 1) % K, np.full(1200, 0.5, np.float32), np.full(1200, 0.1, np.float32), [400] * n_images, None, 0, K, 1)
    cs = CoverStats(r["cover"], r["n_images_used"])
    assert len(cs.table()["class"]) == K and cs.table()["mean_true_cover_pct"].max() == pytest.approx(0.25)
    assert cs.scalars() == dict.fromkeys(names, 0.0)
    # significant classes whose true cover is constant: the NaN-dropping median has nothing left
    r = restate([0, 0, 1, 1, 0, 0, 1, 1], [0, 1, 1, 1, 0, 0, 0, 1], np.full(8, 0.5, np.float32), np.full(8, 0.5, np.float32), [4, 4], None, 0, 3, 1)
    cs = CoverStats(r["cover"], 2)
    tab, sc = cs.table(), cs.scalars()
    assert tab["class"].tolist() == [0, 1] and np.isnan(tab["r_squared"]).all() and np.isnan(sc["cover_median_r_squared"])
    assert sc["cover_mean_abs_bias_pct"] == pytest.approx(0.0) and sc["cover_mean_mae_pct"] == pytest.approx(25.0)
    # one class varies: its R^2 is the median
    r = restate([0, 0, 1, 1, 0, 1, 1, 1], [0, 0, 1, 1, 0, 0, 1, 1], np.full(8, 0.5, np.float32), np.full(8, 0.5, np.float32), [4, 4], None, 0, 2, 1)
    cs = CoverStats(r["cover"], 2)
    t0, p0 = np.array([0.5, 0.25]), np.array([0.5, 0.5])
    want = 1 - ((t0 - p0) ** 2).sum() / ((t0 - t0.mean()) ** 2).sum()
    assert cs.scalars()["cover_median_r_squared"] == pytest.approx(want, abs=1e-12)
    with pytest.raises(ValueError, match="expected"):
        CoverStats(np.zeros((4, 7)), 1)


def test_source_table_and_scalars_match_compute_per_source(fx, tables):
    from mermaid_classifier_amd import SourceStats
    st = SourceStats(tables[20]["source_confusion"])
    images = np.bincount(fx["source_of_image"], minlength=4)
    tab = st.table(fx["source_keys"].tolist(), images, top_of_class=fx["top_of_class"])
    assert tab["source_key"] == [fx["source_keys"][i] for i in fx["source_index"]]
    assert tab["num_val_images"] == fx["source_num_val_images"].tolist()
    assert tab["num_val_annotations"] == fx["source_num_val_annotations"].tolist() == sorted(tab["num_val_annotations"], reverse=True)
    for k in ("accuracy", "balanced_accuracy", "f1_macro", "precision_macro", "recall_macro", "cross_branch_error_rate"):
        assert tab[k] == fx[f"source_{k}"].tolist(), k
    sc = st.scalars()
    assert sc["per_source/n_sources"] == float(fx["scalar_per_source_n_sources"]) == 4.0
    assert sc["per_source/min_accuracy"] == pytest.approx(float(fx["scalar_per_source_min_accuracy"]), abs=1e-15)
    assert sc["per_source/max_accuracy"] == pytest.approx(float(fx["scalar_per_source_max_accuracy"]), abs=1e-15)
    assert "cross_branch_error_rate" not in st.table(fx["source_keys"].tolist(), images)


def test_source_branches():
    from mermaid_classifier_amd import SourceStats
    conf = np.zeros((3, 4, 4), np.int64)
    conf[0, 2, 2] = 9                      # a single class, all right: balanced accuracy = accuracy
    conf[2, 1, 1], conf[2, 1, 3], conf[2, 0, 1] = 2, 1, 1   # source 1 holds nothing and is left out
    st = SourceStats(conf)
    tab = st.table(["a:1", "b:2", "c:3"], [3, 0, 2], top_of_class=[0, 0, 1, 1])
    assert tab["source_key"] == ["a:1", "c:3"] and tab["num_val_annotations"] == [9, 4] and tab["num_val_images"] == [3, 2]
    assert tab["accuracy"] == [1.0, 0.5] and tab["balanced_accuracy"] == [1.0, round((0 + 2 / 3) / 2, 4)]
    assert tab["precision_macro"] == [1.0, round((0 + 2 / 3 + 0) / 3, 4)] and tab["recall_macro"] == [1.0, round((0 + 2 / 3 + 0) / 3, 4)]
    assert tab["f1_macro"] == [1.0, round((0 + 2 * 2 / (3 + 3) + 0) / 3, 4)]
    assert tab["cross_branch_error_rate"] == [0.0, 0.5]                          # no error at all; 1 -> 3 crosses, 0 -> 1 does not
    assert st.scalars() == {"per_source/n_sources": 2.0, "per_source/min_accuracy": 0.5, "per_source/max_accuracy": 1.0}
    assert SourceStats(np.zeros((2, 3, 3))).scalars() == {} and SourceStats(np.zeros((2, 3, 3))).table(["a", "b"], [0, 0])["source_key"] == []
    with pytest.raises(ValueError, match="top_of_class must be 4 integers"):
        st.table(["a", "b", "c"], [1, 1, 1], top_of_class=[0, 1])
    with pytest.raises(ValueError, match="must have 3 entries"):
        st.table(["a"], [1])


@pytest.mark.parametrize("n_bins", [20, 7])
def test_reliability_matches_adaptive_ece(fx, tables, n_bins):
    from mermaid_classifier_amd import Reliability
    t = tables[n_bins]
    rel = Reliability(t["bin_count"], t["bin_correct"], t["bin_conf_q32"], t["bin_conf_min"], t["bin_conf_max"])
    bins = rel.bins
    assert len(bins) == n_bins == len(fx[f"bins{n_bins}_count"])
    assert [b["count"] for b in bins] == fx[f"bins{n_bins}_count"].tolist()
    assert [b["conf_min"] for b in bins] == fx[f"bins{n_bins}_conf_min"].tolist()
    assert [b["conf_max"] for b in bins] == fx[f"bins{n_bins}_conf_max"].tolist()
    for k in ("avg_confidence", "avg_accuracy"):
        gap = np.abs(np.array([b[k] for b in bins]) - fx[f"bins{n_bins}_{k}"]).max()
        print(f"n_bins {n_bins} {k}: max |d| = {gap:.3g} (allowed 1e-12)")
        assert gap <= 1e-12, k
    assert all(b["gap"] == b["avg_confidence"] - b["avg_accuracy"] for b in bins)
    print(f"n_bins {n_bins}: |ece - reference| = {abs(rel.ece - float(fx[f'ece{n_bins}'])):.3g} (allowed 1e-12)")
    assert abs(rel.ece - float(fx[f"ece{n_bins}"])) <= 1e-12


def test_reliability_with_fewer_rows_than_bins():
    from mermaid_classifier_amd import Reliability
    score = np.array([0.9, 0.3, 0.5, 0.7, 0.5, 1.0, 0.25], np.float32)
    g, est = np.array([0, 1, 2, 0, 1, 2, 0]), np.array([0, 1, 0, 0, 1, 2, 1])
    r = restate(g, est, score, score, [7], None, 0, 3, 20)
    assert r["bin_count"].sum() == 7 and (r["bin_count"] == 0).sum() == 13
    rel = Reliability(r["bin_count"], r["bin_correct"], r["bin_conf_q32"], r["bin_conf_min"], r["bin_conf_max"])
    bins = rel.bins
    assert len(bins) == 7 and all(b["count"] == 1 and b["conf_min"] == b["conf_max"] == b["avg_confidence"] for b in bins)
    assert [b["conf_min"] for b in bins] == np.sort(score).tolist()
    # equal scores 0.5: the wrong row comes first
    assert [b["avg_accuracy"] for b in bins] == [0.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0]
    order = np.argsort(score, kind="stable")
    want = np.abs((est == g)[order].astype(float) - score[order].astype(np.float64)).sum() / 7
    assert rel.ece == pytest.approx(want, abs=1e-15)
    with pytest.raises(ValueError, match="equally long"):
        Reliability([1, 2], [1], [1, 2], [0, 0], [0, 0])


def test_by_class_groups_the_integer_sums(fx, tables):
    from mermaid_classifier_amd import CoverStats, GroupedValidation, Reliability, Validation
    t = tables[20]
    K = len(fx["classes"])
    gt, est, scores = fx["gt"], fx["est"], fx["scores"]
    p_true = np.where(est == gt, scores, np.float32(0.05)).astype(np.float32)
    conf = np.bincount(gt * K + est, minlength=K * K).reshape(K, K)
    val = Validation(fx["classes"].tolist(), None, None, None, None, None, conf, np.zeros(K), len(gt), int((gt == est).sum()), 0, 0,
                     int(t["nll_q32"].sum()))
    gv = GroupedValidation(val, CoverStats(t["cover"], t["n_images_used"]), None,
                           Reliability(t["bin_count"], t["bin_correct"], t["bin_conf_q32"], t["bin_conf_min"], t["bin_conf_max"]),
                           t["support"], t["nll_q32"], t["score_q32"])
    cat = np.array([0, 0, 0, 1, 1, 1, 2, -1, 2])
    got = gv.by_class(cat, min_samples=30)
    assert sorted(got) == [0, 1, 2]
    for c in (0, 1, 2):
        m = np.isin(gt, np.flatnonzero(cat == c))
        assert got[c]["n_samples"] == int(m.sum())
        assert got[c]["accuracy"] == (est[m] == gt[m]).mean()
        assert got[c]["avg_confidence"] == pytest.approx(float(scores[m].astype(np.float64).mean()), abs=1e-12)
        assert got[c]["log_loss"] == pytest.approx(float(-np.log(p_true[m].astype(np.float64)).mean()), abs=1e-9)
    assert sorted(gv.by_class(cat, min_samples=int((gt >= 3).sum()))) == [0]     # small categories are left out
    with pytest.raises(ValueError, match="must be 9 integers"):
        gv.by_class([0, 1])
