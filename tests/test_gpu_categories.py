"""-m gpu: per-category reliability bins on the device (metrics.hip behind mmc_head_evaluate_categories / _set,
metrics.grouped_validate(..., category_of_class=...)).

The checker is ``restate_categories`` of test_taxonomy_host.py applied to the per-row outputs (est, score) of the same call: every
category table -- rows, bin counts, count / n_correct / conf_q32 per bin and the bits of conf_min / conf_max -- must be EQUAL, and
everything the grouped call returns must come back with the bits of mmc_head_evaluate_grouped on the same input (the cover doubles
included: the two calls make the same launches for them).
Shapes: K = 5 with an empty category, a category of a single row (2 bins, one empty) and a class without a category; K = 108 with
12 categories; rows above two 65 536-row chunks with every category on both sides of both chunk edges, from host rows and from a
feature set with first > 0; equal keys across bin edges inside a category; unscored rows; the argument checks."""

import numpy as np
import pytest

from test_gpu_metrics import EVAL_TABLES, PER_ROW, _load, _ptr, _rows_of, _set_of, _sizes, c_grouped, same_bits
from test_taxonomy_host import restate_categories

pytestmark = pytest.mark.gpu

GROUP_OUT = ("support", "nll_q32", "score_q32", "source_confusion", "cover", "n_images_used", "bin_count", "bin_correct", "bin_conf_q32",
             "bin_conf_min", "bin_conf_max")
CAT_OUT = ("cat_rows", "cat_n_bins", "cat_bin_count", "cat_bin_correct", "cat_bin_conf_q32", "cat_bin_conf_min", "cat_bin_conf_max")


def c_categories(head, X, y, sizes, cat, n_categories, source=None, n_sources=0, n_bins=20, lmap=None, fs=None, first=0, expect=0,
                 offsets=None):
    """mmc_head_evaluate_categories on host rows, or _set on rows [first, first + len(y)) of ``fs``; every output starts from -7.
    -> dict of outputs."""
    from mermaid_classifier_amd import _lib
    K, n = head.n_classes, len(y)
    y = np.ascontiguousarray(y, np.int32)
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum(sizes)])
    offsets = np.ascontiguousarray(offsets, np.int64)
    src = None if source is None else np.ascontiguousarray(source, np.int32)
    cat = None if cat is None else np.ascontiguousarray(cat, np.int32)
    nb = n_bins if 1 <= n_bins <= 64 else 64
    nc = n_categories if 1 <= n_categories <= 64 else 64
    o = dict(est=np.full(n, -7, np.int32), score=np.full(n, -7, np.float32), rank=np.full(n, -7, np.int32), p_true=np.full(n, -7, np.float32),
             totals=np.full(5, -7, np.int64), confusion=np.full((K, K), -7, np.int64), rank_hist=np.full(K, -7, np.int64),
             support=np.full(K, -7, np.int64), nll_q32=np.full(K, -7, np.int64), score_q32=np.full(K, -7, np.int64),
             source_confusion=np.full((n_sources if n_sources > 0 else 1, K, K), -7, np.int64), cover=np.full((K, 8), -7.0),
             n_images_used=np.full(1, -7, np.int64),
             bin_count=np.full(nb, -7, np.int64), bin_correct=np.full(nb, -7, np.int64), bin_conf_q32=np.full(nb, -7, np.int64),
             bin_conf_min=np.full(nb, -7, np.float32), bin_conf_max=np.full(nb, -7, np.float32),
             cat_rows=np.full(nc, -7, np.int64), cat_n_bins=np.full(nc, -7, np.int32), cat_bin_count=np.full((nc, 20), -7, np.int64),
             cat_bin_correct=np.full((nc, 20), -7, np.int64), cat_bin_conf_q32=np.full((nc, 20), -7, np.int64),
             cat_bin_conf_min=np.full((nc, 20), -7, np.float32), cat_bin_conf_max=np.full((nc, 20), -7, np.float32))
    common = [_ptr(lmap), 0 if lmap is None else len(lmap)] + [o[k].ctypes.data for k in PER_ROW + EVAL_TABLES] + \
             [offsets.ctypes.data, len(offsets) - 1, _ptr(src), n_sources, n_bins] + [o[k].ctypes.data for k in GROUP_OUT] + \
             [_ptr(cat), n_categories] + [o[k].ctypes.data for k in CAT_OUT]
    lib = _lib.lib()
    if fs is not None:
        status = lib.mmc_head_evaluate_categories_set(head._h, fs._handle(), first, n, *common, None)
    else:
        X = np.ascontiguousarray(X, np.float32)
        status = lib.mmc_head_evaluate_categories(head._h, X.ctypes.data, y.ctypes.data, n, *common, _lib.MMC_IN_HOST, None)
    assert status == expect, lib.mmc_last_error()
    if not n_sources:
        del o["source_confusion"]
    o["n_images_used"] = int(o["n_images_used"][0])
    return o


def grouped_part(o):
    return {k: v for k, v in o.items() if k not in CAT_OUT}


def matches_restatement(o, g, cat, n_categories, what):
    """The call's category tables against the numpy restatement on its own per-row outputs; ``g``: true class of a scored row, else -1."""
    want = restate_categories(g, o["est"], o["score"], cat, n_categories)
    for k in CAT_OUT[:5]:
        assert o[k].dtype == want[k].dtype and np.array_equal(o[k], want[k]), f"{what}: {k}"
    for k in CAT_OUT[5:]:
        assert np.array_equal(o[k].view(np.uint32), want[k].view(np.uint32)), f"{what}: {k}"
    g = np.asarray(g)
    with_cat = (g >= 0) & (np.asarray(cat)[np.maximum(g, 0)] >= 0)
    assert int(o["cat_rows"].sum()) == int(with_cat.sum()) == int(o["cat_bin_count"].sum()), what
    for c, nb in enumerate(o["cat_n_bins"]):                                        # the bins at index nb_c and above are all zero
        for k in CAT_OUT[2:]:
            assert not o[k][c, nb:].any(), f"{what}: {k}[{c}]"
    print(f"{what}: {len(g)} rows, rows per category {o['cat_rows'].tolist()}, bins {o['cat_n_bins'].tolist()}: every table equal")
    return want


# ---- 1. / 2. the two heads, both routes ----

def _case(name, n, rng):
    head = _load(name)._head
    K = head.n_classes
    X = _rows_of(name, n)
    _, arg = head.predict(X)
    y = np.where(rng.random(n) < 0.6, arg, rng.integers(0, K, n)).astype(np.int32)
    return head, K, X, y


def test_category_tables_of_a_small_head_with_an_empty_and_a_one_row_category():
    rng = np.random.default_rng(21)
    head, K, X, y = _case("head_fixture", 700, rng)
    assert K == 5
    cat = np.array([0, 2, -1, 0, 3], np.int32)                                      # category 1 is empty, class 2 has no category
    y[y == 4] = 0
    y[123] = 4                                                                      # category 3 holds a single row
    sizes = _sizes(rng, 700, 23)
    source = rng.integers(0, 4, len(sizes))
    o = c_categories(head, X, y, sizes, cat, 4, source, 4)
    assert o["totals"][:4].tolist() == [700, int((o["est"] == y).sum()), 0, 0]
    matches_restatement(o, y, cat, 4, "head_fixture, 4 categories")
    assert o["cat_rows"][1] == 0 and o["cat_n_bins"][1] == 0 and o["cat_rows"][3] == 1 and o["cat_n_bins"][3] == 2
    assert o["cat_bin_count"][3, :2].tolist() == [0, 1] and o["cat_bin_conf_min"][3, 1] == o["score"][123] == o["cat_bin_conf_max"][3, 1]
    assert o["cat_rows"].sum() == 700 - (y == 2).sum() and (y == 2).any()
    same_bits(grouped_part(o), c_grouped(head, X, y, sizes, source, 4, 20))         # the grouped call's bits, cover doubles included
    fs = _set_of(head, X, y)
    same_bits(o, c_categories(head, None, y, sizes, cat, 4, source, 4, fs=fs))
    same_bits(o, c_categories(head, X, y, sizes, cat, 4, source, 4))                # a repeat call
    fs.close()


def test_category_tables_of_108_classes_in_12_categories():
    rng = np.random.default_rng(22)
    head, K, X, y = _case("head108", 2000, rng)
    assert K == 108
    cat = (rng.permutation(K) % 12).astype(np.int32)
    sizes = _sizes(rng, 2000, 40)
    o = c_categories(head, X, y, sizes, cat, 12, None, 0, 7)
    matches_restatement(o, y, cat, 12, "head108, 12 categories")
    assert (o["cat_rows"] > 0).all() and len(set(o["cat_n_bins"].tolist())) > 1
    same_bits(grouped_part(o), c_grouped(head, X, y, sizes, None, 0, 7))
    fs = _set_of(head, X, y)
    same_bits(o, c_categories(head, None, y, sizes, cat, 12, None, 0, 7, fs=fs))
    fs.close()


# ---- 3. above the chunk ----

def test_categories_above_the_65536_row_chunk():
    rng = np.random.default_rng(23)
    n, first = 2 * 65536 + 777, 13
    head = _load("head108")._head
    K = head.n_classes
    X0 = _rows_of("head108", 256)
    _, arg = head.predict(X0)
    rows = (np.arange(n + first) - first) % 256                                     # one buffer: the set's rows, and the call's from row 13 on
    Xall = np.ascontiguousarray(X0[rows])
    X = Xall[first:]
    y = np.where(rng.random(n) < 0.6, arg[rows[first:]], rng.integers(0, K, n)).astype(np.int32)
    cat = (np.arange(K) % 12).astype(np.int32)
    cat[5] = -1
    sizes = _sizes(rng, n, 400)
    for lo, hi in ((0, 65536), (65536, 131072), (131072, n)):                       # every category lies on both sides of both chunk edges
        assert len(set(cat[y[lo:hi]].tolist()) - {-1}) == 12
    o = c_categories(head, X, y, sizes, cat, 12)
    matches_restatement(o, y, cat, 12, "131849 rows")
    assert o["cat_n_bins"].tolist() == [20] * 12 and len(np.unique(o["score"])) <= 256   # (and so every bin edge lies among equal scores)
    fs = _set_of(head, Xall, np.concatenate([y[:first], y]))                        # the same rows, 13 rows into a resident set
    same_bits(o, c_categories(head, None, y, sizes, cat, 12, fs=fs, first=first))
    fs.close()


# ---- 4. ties ----

def test_equal_keys_across_bin_edges_inside_a_category():
    head = _load("head_fixture")._head
    K = head.n_classes
    X0 = _rows_of("head_fixture", 64)
    _, arg = head.predict(X0)
    i0 = 0
    i1 = int(np.flatnonzero(arg != arg[0])[0])
    e0, e1 = int(arg[i0]), int(arg[i1])
    a, b = [c for c in range(K) if c not in (e0, e1)][:2]
    cat = np.full(K, -1, np.int32)
    cat[[e0, a]], cat[[e1, b]] = 0, 1
    # category 0: 40 copies of one row, 20 wrong then 20 right: 4 bins, the edge at 20 lies between two keys that differ in the
    # correctness bit alone, the edges at 10 and 30 inside equal keys.  category 1: 15 wrong, 25 right: the edge at 10 inside the wrong
    # keys, the change of the bit inside bin 1
    y = np.array([a] * 20 + [e0] * 20 + [b] * 15 + [e1] * 25, np.int32)
    X = np.ascontiguousarray(np.concatenate([np.tile(X0[i0], (40, 1)), np.tile(X0[i1], (40, 1))]))
    perm = np.random.default_rng(24).permutation(80)
    X, y = np.ascontiguousarray(X[perm]), y[perm]
    sizes = np.full(8, 10)
    o = c_categories(head, X, y, sizes, cat, 2)
    assert len(np.unique(o["score"])) == 2 and o["cat_rows"].tolist() == [40, 40] and o["cat_n_bins"].tolist() == [4, 4]
    assert o["cat_bin_count"][:, :4].tolist() == [[10] * 4] * 2
    assert o["cat_bin_correct"][:, :4].tolist() == [[0, 0, 10, 10], [0, 5, 10, 10]]
    assert (o["cat_bin_conf_min"][:, :4] == o["cat_bin_conf_max"][:, :4]).all()
    matches_restatement(o, y, cat, 2, "two distinct rows, 4 bins per category")
    # four distinct rows, each with every label: in both categories groups of equal score and mixed correctness straddle bin edges
    n = 400
    X = np.ascontiguousarray(X0[np.arange(n) % 4])
    y = ((np.arange(n) // 4) % K).astype(np.int32)
    cat = np.array([0, 1, 0, 1, 0], np.int32)
    o = c_categories(head, X, y, np.full(40, 10), cat, 2, None, 0, 7)
    for c in (0, 1):
        m = cat[y] == c
        s, k = o["score"][m], (o["est"] == y)[m]
        order = np.lexsort((k, s))
        s, k, nb = s[order], k[order], int(o["cat_n_bins"][c])
        edges = np.arange(1, nb) * len(s) // nb
        assert any(s[e - 1] == s[e] and k[e - 1] == k[e] for e in edges), f"category {c}: no bin edge inside equal keys"
        assert any(s[e - 1] == s[e] and len(set(k[s == s[e]].tolist())) == 2 for e in edges), f"category {c}: no mixed tie group at an edge"
    matches_restatement(o, y, cat, 2, "four distinct rows")
    same_bits(grouped_part(o), c_grouped(head, X, y, np.full(40, 10), None, 0, 7))


# ---- 5. exclusions ----

def test_unscored_rows_enter_no_category_table():
    """A one-layer head, so that a NaN feature reaches the probabilities (a hidden ReLU would turn it into 0)."""
    from mermaid_classifier_amd.inference import DeviceHead, HeadParams
    rng = np.random.default_rng(13)
    K = 5
    head = DeviceHead(HeadParams([rng.normal(0, 0.7, (K, 8)).astype(np.float32)], [rng.normal(0, 0.1, K).astype(np.float32)],
                                 rng.uniform(-12, -4, K).astype(np.float32), rng.uniform(0.5, 2, K).astype(np.float32)))
    n = 300
    X = _rows_of("head_fixture", n).copy()
    sizes = np.array([10] * 30)
    lmap = np.array([0, 1, 2, 3, 4, -1], np.int32)                                 # label 5: a class the head lacks
    cat = np.array([1, 0, 1, -1, 2], np.int32)                                     # categories are of the head's classes
    y = rng.integers(0, K, n).astype(np.int32)
    y[[3, 57, 140]] = 5
    y[200:210] = 5
    X[205] = np.nan
    X[77, 2] = np.nan
    assert np.isnan(head.predict(X[77:78])[0]).any() and y[77] != 5
    o = c_categories(head, X, y, sizes, cat, 3, lmap=lmap)
    g = lmap[y].copy()
    g[77] = -1
    assert o["totals"].tolist()[:4] == [n, int((o["est"] == g).sum()), 13, 1]
    matches_restatement(o, g, cat, 3, "13 unknown rows, 1 NaN row")
    assert o["cat_rows"].sum() == ((g >= 0) & (cat[np.maximum(g, 0)] >= 0)).sum() < (g >= 0).sum()
    same_bits(grouped_part(o), c_grouped(head, X, y, sizes, None, 0, 20, lmap=lmap))
    fs = _set_of(head, X, y, classes=list(range(6)))
    same_bits(o, c_categories(head, None, y, sizes, cat, 3, lmap=lmap, fs=fs))
    fs.close()
    y[:] = 5                                                                       # nothing scored at all
    o = c_categories(head, X, y, sizes, cat, 3, lmap=lmap)
    assert not any(o[k].any() for k in CAT_OUT)
    head.close()


# ---- 6. the C ABI's argument checks ----

def test_malformed_category_arguments_are_rejected_before_any_launch():
    from mermaid_classifier_amd import _lib
    head = _load("head_fixture")._head
    K = head.n_classes
    X = _rows_of("head_fixture", 20)
    y = (np.arange(20) % K).astype(np.int32)
    sizes, source, cat = np.array([5, 5, 10]), [0, 1, 1], [0, 1, -1, 2, 0]
    good = c_categories(head, X, y, sizes, cat, 3, source, 2, 4)
    E = _lib.MMC_ERR_ARG

    def rejected(what, **kw):
        args = dict(sizes=sizes, cat=cat, n_categories=3, source=source, n_sources=2, n_bins=4)
        args.update(kw)
        o = c_categories(head, X, y, expect=E, **args)
        assert what.encode() in _lib.lib().mmc_last_error(), (what, _lib.lib().mmc_last_error())
        for k, v in o.items():
            if k in PER_ROW:
                continue                                                           # (per-row outputs are not tables)
            if k.startswith("bin_") and not 1 <= args["n_bins"] <= 64:
                continue                                                           # (their length is n_bins)
            if k.startswith("cat_") and not 1 <= args["n_categories"] <= 64:
                assert (np.asarray(v) == -7).all(), (what, k)                      # (their length is n_categories: left alone)
                continue
            assert not np.asarray(v).any(), (what, k)

    rejected("category_of_class is NULL", cat=None)
    rejected("category_of_class[2] = -2 outside [-1, 3)", cat=[0, 1, -2, 2, 0])
    rejected("category_of_class[3] = 3 outside [-1, 3)", cat=[0, 1, -1, 3, 0])
    rejected("n_categories = 0 outside [1, 64]", n_categories=0)
    rejected("n_categories = 65 outside [1, 64]", n_categories=65)
    rejected("n_categories = -1 outside [1, 64]", n_categories=-1)
    rejected("n_bins = 0 outside [1, 64]", n_bins=0)                               # the grouped checks hold as well
    rejected("offsets increase strictly", offsets=[0, 5, 5, 20])
    rejected("source_of_image[2] = 2 outside [0, 2)", source=[0, 1, 2])
    same_bits(good, c_categories(head, X, y, sizes, cat, 3, source, 2, 4))         # a good call after the rejected ones
    # n == 0 is MMC_OK with zeroed outputs; every category output NULL: the rest still comes back
    lib = _lib.lib()
    tot, rows_out = np.full(5, -7, np.int64), np.full(3, -7, np.int64)
    catp = np.array(cat, np.int32)
    offs = np.zeros(1, np.int64)
    args = [None, 0, None, None, None, None, tot.ctypes.data, None, None, offs.ctypes.data, 0, None, 0, 4] + [None] * 11 + \
           [catp.ctypes.data, 3, rows_out.ctypes.data] + [None] * 6
    assert lib.mmc_head_evaluate_categories(head._h, X.ctypes.data, y.ctypes.data, 0, *args, _lib.MMC_IN_HOST, None) == _lib.MMC_OK
    assert not tot.any() and not rows_out.any()
    offs = np.array([0, 5, 10, 20], np.int64)
    args[9], args[10] = offs.ctypes.data, 3
    args[27] = None
    tot[:] = -7
    assert lib.mmc_head_evaluate_categories(head._h, X.ctypes.data, y.ctypes.data, 20, *args, _lib.MMC_IN_HOST, None) == _lib.MMC_OK
    assert np.array_equal(tot, good["totals"])
    # 64 categories: the largest count
    wide = c_categories(head, X, y, sizes, [63, 0, -1, 2, 63], 64)
    matches_restatement(wide, y, [63, 0, -1, 2, 63], 64, "64 categories")


# ---- 7. one handle's scratch ----

def test_interleaved_validation_passes_on_one_handle_match_fresh_handles():
    """validate, grouped, ranked and categories share one handle's device scratch, and each call lays out what it needs: a larger
    category call after a smaller grouped one, and back, every output bit for bit the same call's on a head that has done nothing else."""
    from mermaid_classifier_amd.inference import DeviceHead
    from test_gpu_ranking import _levels, c_ranked
    from test_gpu_validation import c_evaluate
    params = _load("head_fixture")._head.params
    X = _rows_of("head_fixture", 512)
    rng = np.random.default_rng(5)
    y = rng.integers(0, 5, 512).astype(np.int32)
    sizes = _sizes(rng, 512, 30)
    small = _sizes(rng, 100, 30)
    source = rng.integers(0, 3, len(sizes))
    levels = _levels(rng, 5, 3)
    cat = [0, 1, 1, -1, 2]
    calls = [lambda h: c_grouped(h, X[:100], y[:100], small, None, 0, 7),
             lambda h: c_categories(h, X, y, sizes, cat, 3, source, 3),
             lambda h: c_evaluate(h, X, y),
             lambda h: c_ranked(h, X[:300], y[:300], levels, 3, 3),
             lambda h: c_categories(h, X[:100], y[:100], small, [0, 0, 0, 0, 0], 1),
             lambda h: c_grouped(h, X, y, sizes, source, 3),
             lambda h: c_categories(h, X, y, sizes, cat, 3, source, 3)]
    one = DeviceHead(params)
    for i, call in enumerate(calls):
        got, want = call(one), call(DeviceHead(params))
        assert got.keys() == want.keys(), f"call {i}"
        for k in got:
            va, vb = np.asarray(got[k]), np.asarray(want[k])
            assert va.dtype == vb.dtype and va.tobytes() == vb.tobytes(), f"call {i}: {k}"


# ---- 8. the Python layer ----

def test_grouped_validate_with_categories_agrees_with_the_c_tables():
    from mermaid_classifier_amd import FeatureSet, grouped_validate
    pred = _load("head108")
    K = len(pred.classes)
    n = 1000
    rng = np.random.default_rng(14)
    X = _rows_of("head108", n)
    _, arg = pred._head.predict(X)
    yi = np.where(rng.random(n) < 0.5, arg, rng.integers(0, K, n)).astype(np.int32)
    labels = np.asarray(pred.classes)[yi]
    sizes = _sizes(rng, n, 30)
    cat = (np.arange(K) % 7).astype(np.int64)
    cat[cat == 6] = -3                                                             # negative: the class is left out
    c = c_categories(pred._head, X, yi, sizes, np.where(cat < 0, -1, cat), 6)
    gv = grouped_validate(pred, (X, labels), sizes, category_of_class=cat, rows=True)
    assert sorted(gv.category_reliability) == np.flatnonzero(c["cat_rows"]).tolist() == list(range(6))
    for i, rel in gv.category_reliability.items():
        nb = int(c["cat_n_bins"][i])
        for name, col in (("count", "cat_bin_count"), ("n_correct", "cat_bin_correct"), ("conf_q32", "cat_bin_conf_q32"),
                          ("conf_min", "cat_bin_conf_min"), ("conf_max", "cat_bin_conf_max")):
            assert getattr(rel, name).tobytes() == c[col][i, :nb].tobytes(), (i, name)
    assert np.array_equal(gv.category_of_class, np.where(cat < 0, -1, cat)) and gv.category_of_class.dtype == np.int32
    rows = gv.category_calibration(min_samples=30)
    assert [r["ece"] for r in rows] == sorted((r["ece"] for r in rows), reverse=True) and len(rows) == 6
    for r in rows:
        m = cat[yi] == r["category"]
        assert r["n_samples"] == int(m.sum()) and r["accuracy"] == (gv.validation.est[m] == yi[m]).mean()
        assert r["avg_confidence"] == pytest.approx(float(gv.validation.scores[m].astype(np.float64).mean()), abs=1e-12)
    plain = grouped_validate(pred, (X, labels), sizes, rows=True)
    assert plain.category_reliability is None and plain.category_of_class is None
    for name in ("count", "n_correct", "conf_q32", "conf_min", "conf_max"):
        assert getattr(plain.reliability, name).tobytes() == getattr(gv.reliability, name).tobytes(), name
    assert plain.cover.sums.tobytes() == gv.cover.sums.tobytes() and np.array_equal(plain.validation.confusion, gv.validation.confusion)
    with pytest.raises(ValueError, match="no category tables"):
        plain.category_calibration()
    fs = FeatureSet(pred.input_dim, list(pred.classes)).append(X, labels)           # the same through a resident set
    gs = grouped_validate(pred, fs, sizes, category_of_class=cat)
    assert [r for r in gs.category_calibration()] == rows
    fs.close()
