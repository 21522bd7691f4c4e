"""-m gpu: grouped validation on the device (metrics.hip behind mmc_head_evaluate_grouped / _set, metrics.grouped_validate).

The checker is ``restate`` of test_metrics_host.py applied to the per-row outputs (est, score, p_true) of the same call.  Every
integer table -- per-class sums, per-source confusion, the bins' count / n_correct / conf_q32 and the bits of conf_min / conf_max,
n_images_used -- must be EQUAL; a cover sum must lie within 1e-12 of the checker's relative to the sum of its absolute terms (fp64
sums of at most a few thousand terms in another order err below 1e-13 of that), min t / max t equal.  The per-class loss sums use the
device's log where the checker uses the host's, a difference the rounding to 2^-32 units absorbs unless a row's loss lies within
about 2^-16 units of a half; the rows here are few distinct ones, and the sum over classes is also checked against totals[4].
Shapes: K = 5 and 108 (more classes than lanes, no multiple of 64), rows above two 65 536-row chunks with images across the chunk
boundaries and one image of 70 000 rows, equal keys across bin edges, all rows equal, unscored rows and an image of only such rows,
fewer rows than bins, one bin."""

import numpy as np
import pytest

from conftest import GOLDEN
from test_metrics_host import restate

pytestmark = pytest.mark.gpu

PER_ROW = ("est", "score", "rank", "p_true")
EVAL_TABLES = ("totals", "confusion", "rank_hist")
INT_TABLES = ("support", "nll_q32", "score_q32", "n_images_used", "bin_count", "bin_correct", "bin_conf_q32")


def _load(name):
    from mermaid_classifier_amd import load_predictor
    return load_predictor(GOLDEN / name / "model.pt", GOLDEN / name / "model.json")


def _ptr(a):
    return None if a is None else a.ctypes.data


def _rows_of(name, n):
    X0 = np.load(GOLDEN / f"{name}_io.npz")["X"]
    return np.ascontiguousarray(np.tile(X0, (-(-n // len(X0)), 1))[:n])


def _sizes(rng, n, hi=40):
    out = []
    while sum(out) < n:
        out.append(int(min(rng.integers(1, hi + 1), n - sum(out))))
    return np.array(out, np.int64)


def c_grouped(head, X, y, sizes, source=None, n_sources=0, n_bins=20, lmap=None, fs=None, offsets=None, expect=0, first=0):
    """mmc_head_evaluate_grouped on host rows, or _set on rows [first, first + len(y)) of ``fs``; every output starts from -7.
    -> dict of outputs."""
    from mermaid_classifier_amd import _lib
    K, n = head.n_classes, len(y)
    y = np.ascontiguousarray(y, np.int32)
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum(sizes)])
    offsets = np.ascontiguousarray(offsets, np.int64)
    src = None if source is None else np.ascontiguousarray(source, np.int32)
    nb = n_bins if 1 <= n_bins <= 64 else 64
    o = dict(est=np.full(n, -7, np.int32), score=np.full(n, -7, np.float32), rank=np.full(n, -7, np.int32), p_true=np.full(n, -7, np.float32),
             totals=np.full(5, -7, np.int64), confusion=np.full((K, K), -7, np.int64), rank_hist=np.full(K, -7, np.int64),
             support=np.full(K, -7, np.int64), nll_q32=np.full(K, -7, np.int64), score_q32=np.full(K, -7, np.int64),
             source_confusion=np.full((n_sources if 0 < n_sources * K * K <= 1 << 26 else 1, K, K), -7, np.int64), cover=np.full((K, 8), -7.0), n_images_used=np.full(1, -7, np.int64),
             bin_count=np.full(nb, -7, np.int64), bin_correct=np.full(nb, -7, np.int64), bin_conf_q32=np.full(nb, -7, np.int64),
             bin_conf_min=np.full(nb, -7, np.float32), bin_conf_max=np.full(nb, -7, np.float32))
    common = [_ptr(lmap), 0 if lmap is None else len(lmap)] + [o[k].ctypes.data for k in PER_ROW + EVAL_TABLES] + \
             [offsets.ctypes.data, len(offsets) - 1, _ptr(src), n_sources, n_bins] + \
             [o[k].ctypes.data for k in ("support", "nll_q32", "score_q32", "source_confusion", "cover", "n_images_used", "bin_count",
                                         "bin_correct", "bin_conf_q32", "bin_conf_min", "bin_conf_max")]
    lib = _lib.lib()
    if fs is not None:
        status = lib.mmc_head_evaluate_grouped_set(head._h, fs._handle(), first, n, *common, None)
    else:
        X = np.ascontiguousarray(X, np.float32)
        status = lib.mmc_head_evaluate_grouped(head._h, X.ctypes.data, y.ctypes.data, n, *common, _lib.MMC_IN_HOST, None)
    assert status == expect, lib.mmc_last_error()
    if not n_sources:
        del o["source_confusion"]
    o["n_images_used"] = int(o["n_images_used"][0])
    return o


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        va, vb = np.asarray(a[k]), np.asarray(b[k])
        assert va.dtype == vb.dtype and va.tobytes() == vb.tobytes(), k


def matches_restatement(o, g, sizes, source, n_sources, K, n_bins, what):
    """The call's tables against the numpy restatement on its own per-row outputs; ``g``: true class of a scored row, else -1."""
    want = restate(g, o["est"], o["score"], o["p_true"], sizes, source, n_sources, K, n_bins)
    for k in INT_TABLES + (("source_confusion",) if n_sources else ()):
        assert np.array_equal(o[k], want[k]), f"{what}: {k}"
    for k in ("bin_conf_min", "bin_conf_max"):
        assert np.array_equal(o[k].view(np.uint32), want[k].view(np.uint32)), f"{what}: {k}"
    assert int(o["nll_q32"].sum()) == int(o["totals"][4]) and int(o["support"].sum()) == int((np.asarray(g) >= 0).sum()), what
    assert np.array_equal(o["cover"][:, 5:7], want["cover"][:, 5:7]), f"{what}: min t / max t"
    rel = 0.0
    for j in (0, 1, 2, 3, 4, 7):
        gap = np.abs(o["cover"][:, j] - want["cover"][:, j])
        scale = want["cover_abs"][:, j]
        assert np.all(gap[scale == 0] == 0), f"{what}: cover column {j}"
        if (scale > 0).any():
            rel = max(rel, float((gap[scale > 0] / scale[scale > 0]).max()))
    print(f"{what}: {len(o['est'])} rows, {len(sizes)} images ({o['n_images_used']} used); cover sums within {rel:.3g} of the checker "
          f"relative to the sum of absolute terms (allowed 1e-12); every integer table equal")
    assert rel <= 1e-12, what
    return want


def _set_of(head, X, y, classes=None):
    from mermaid_classifier_amd import FeatureSet
    return FeatureSet(head.input_dim, list(range(head.n_classes)) if classes is None else classes).append(X, y)


# ---- 1. / 2. the two heads, both routes, twice ----

@pytest.mark.parametrize("name,n,n_images_hi,n_sources", [("head_fixture", 700, 23, 4), ("head108", 2000, 40, 3)])
def test_grouped_tables_match_the_restatement(name, n, n_images_hi, n_sources):
    head = _load(name)._head
    K = head.n_classes
    rng = np.random.default_rng(11)
    X = _rows_of(name, n)
    proba, arg = head.predict(X)
    y = np.where(rng.random(n) < 0.6, arg, rng.integers(0, K, n)).astype(np.int32)
    sizes = _sizes(rng, n, n_images_hi)
    if name == "head_fixture":                                                     # 60 images: 59 of 1-11 rows and a large one
        sizes = rng.integers(1, 12, 59)
        sizes = np.concatenate([sizes, [n - sizes.sum()]])
        assert len(sizes) == 60 and sizes.min() >= 1 and sizes.sum() == n
    source = rng.integers(0, n_sources, len(sizes))
    host = c_grouped(head, X, y, sizes, source, n_sources, 20)
    assert K == (5 if name == "head_fixture" else 108) and host["totals"][:4].tolist() == [n, int((host["est"] == y).sum()), 0, 0]
    matches_restatement(host, y, sizes, source, n_sources, K, 20, f"{name} host rows")
    fs = _set_of(head, X, y)
    same_bits(host, c_grouped(head, None, y, sizes, source, n_sources, 20, fs=fs))
    same_bits(host, c_grouped(head, X, y, sizes, source, n_sources, 20))          # a repeat call: the same bits, doubles included
    # the evaluation part has the bits of mmc_head_evaluate
    from test_gpu_validation import c_evaluate
    plain = c_evaluate(head, X, y)
    for k in PER_ROW + EVAL_TABLES:
        assert plain[k].tobytes() == host[k].tobytes(), k
    other = c_grouped(head, X, y, sizes, None, 0, 7)                                # no sources, other bins: the rest keeps its bits
    matches_restatement(other, y, sizes, None, 0, K, 7, f"{name} 7 bins, no sources")
    for k in ("support", "nll_q32", "score_q32", "cover"):
        assert other[k].tobytes() == host[k].tobytes(), k
    fs.close()


# ---- 3. above the chunk ----

def test_grouped_above_the_65536_row_chunk():
    head = _load("head_fixture")._head
    n, K = 2 * 65536 + 777, head.n_classes
    rng = np.random.default_rng(12)
    X = _rows_of("head_fixture", n)
    y = ((7 * np.arange(n)) % K).astype(np.int32)
    a = _sizes(rng, 30000)
    b = _sizes(rng, 131000 - 100000)
    c = _sizes(rng, n - 131200)
    sizes = np.concatenate([a, [70000], b, [200], c])
    offs = np.concatenate([[0], np.cumsum(sizes)])
    assert offs[-1] == n and sizes.max() == 70000
    for edge in (65536, 131072):                                                   # an image straddles each chunk boundary
        i = np.searchsorted(offs, edge, side="right") - 1
        assert offs[i] < edge < offs[i + 1]
    source = rng.integers(0, 4, len(sizes))
    o = c_grouped(head, X, y, sizes, source, 4, 20)
    matches_restatement(o, y, sizes, source, 4, K, 20, "131849 rows")
    fs = _set_of(head, X, y)
    same_bits(o, c_grouped(head, None, y, sizes, source, 4, 20, fs=fs))
    fs.close()


# ---- 4. ties ----

def test_equal_keys_across_bin_edges():
    head = _load("head_fixture")._head
    K = head.n_classes
    X0 = _rows_of("head_fixture", 4)
    n = 400
    X = np.ascontiguousarray(X0[np.arange(n) % 4])                                 # four distinct rows, each with every label
    y = ((np.arange(n) // 4) % K).astype(np.int32)
    sizes = np.full(40, 10)
    o = c_grouped(head, X, y, sizes, None, 0, 7)
    assert len(np.unique(o["score"])) <= 4
    order = np.lexsort((o["est"] == y, o["score"]))
    s, c = o["score"][order], (o["est"] == y)[order]
    mixed = [e for e in (np.arange(1, 7) * n // 7) if s[e - 1] == s[e] and len(set(c[s == s[e]].tolist())) == 2]
    assert mixed, "no equal-score group of mixed correctness straddles a bin edge: the case does not test what it is meant to"
    matches_restatement(o, y, sizes, None, 0, K, 7, "4 distinct rows, 7 bins")
    # all rows identical: one key or two, every bin edge inside a tie group
    X1 = np.ascontiguousarray(np.tile(X0[:1], (n, 1)))
    o = c_grouped(head, X1, y, sizes, None, 0, 20)
    assert len(np.unique(o["score"])) == 1 and o["bin_count"].tolist() == [20] * 20
    assert np.all(o["bin_conf_min"] == o["score"][0]) and np.all(o["bin_conf_max"] == o["score"][0])
    matches_restatement(o, y, sizes, None, 0, K, 20, "identical rows, 20 bins")
    y1 = np.full(n, o["est"][0], np.int32)                                         # ... and all right: a single key
    o = c_grouped(head, X1, y1, sizes, None, 0, 20)
    assert o["bin_correct"].tolist() == [20] * 20
    matches_restatement(o, y1, sizes, None, 0, K, 20, "identical rows, one key")


# ---- 5. exclusions ----

def test_unscored_rows_enter_no_table():
    """A one-layer head, so that a NaN feature reaches the probabilities (a hidden ReLU would turn it into 0)."""
    from mermaid_classifier_amd.inference import DeviceHead, HeadParams
    rng = np.random.default_rng(13)
    K = 5
    head = DeviceHead(HeadParams([rng.normal(0, 0.7, (K, 8)).astype(np.float32)], [rng.normal(0, 0.1, K).astype(np.float32)],
                                 rng.uniform(-12, -4, K).astype(np.float32), rng.uniform(0.5, 2, K).astype(np.float32)))
    n = 300
    X = _rows_of("head_fixture", n).copy()
    sizes = np.array([10] * 30)
    source = np.arange(30) % 3
    lmap = np.array([0, 1, 2, 3, 4, -1], np.int32)                                 # label 5: a class the head lacks
    y = rng.integers(0, K, n).astype(np.int32)
    clean = c_grouped(head, X, y, sizes, source, 3, 20, lmap=lmap)
    y[[3, 57, 140]] = 5
    y[200:210] = 5                                                                 # image 20 holds only unknown rows ...
    X[205] = np.nan
    X[77, 2] = np.nan                                                              # ... and row 77 is not finite
    assert np.isnan(head.predict(X[77:78])[0]).any()
    o = c_grouped(head, X, y, sizes, source, 3, 20, lmap=lmap)
    g = lmap[y].copy()
    g[77] = -1
    assert o["totals"].tolist()[:4] == [n, int((o["est"] == g).sum()), 13, 1]
    assert o["n_images_used"] == 29
    matches_restatement(o, g, sizes, source, 3, K, 20, "13 unknown rows, 1 NaN row")
    keep = np.ones(n, bool)
    keep[[3, 57, 140, 77]] = False
    keep[200:210] = False
    for k in PER_ROW:                                                              # the neighbours are unaffected
        assert o[k][keep].tobytes() == clean[k][keep].tobytes(), k
    assert o["rank"][3] == 0 and o["p_true"][3] == 0
    fs = _set_of(head, X, y, classes=list(range(6)))                               # the same through a resident set
    same_bits(o, c_grouped(head, None, y, sizes, source, 3, 20, lmap=lmap, fs=fs))
    fs.close()
    # nothing scored at all
    y[:] = 5
    o = c_grouped(head, X, y, sizes, source, 3, 20, lmap=lmap)
    assert o["n_images_used"] == 0 and not o["cover"].any() and not o["bin_count"].any() and not o["support"].any()
    assert not o["source_confusion"].any() and not o["bin_conf_max"].any()
    head.close()


# ---- 6. fewer rows than bins ----

def test_fewer_rows_than_bins_and_one_bin():
    head = _load("head_fixture")._head
    K = head.n_classes
    X = _rows_of("head_fixture", 7)
    y = np.array([0, 1, 2, 3, 4, 0, 1], np.int32)
    sizes = np.array([3, 4])
    o = c_grouped(head, X, y, sizes, [0, 0], 1, 20)
    assert o["bin_count"].sum() == 7 and (o["bin_count"] == 0).sum() == 13
    empty = o["bin_count"] == 0
    assert not o["bin_correct"][empty].any() and not o["bin_conf_q32"][empty].any() and not o["bin_conf_min"][empty].any()
    matches_restatement(o, y, sizes, [0, 0], 1, K, 20, "7 rows, 20 bins")
    o = c_grouped(head, X, y, sizes, None, 0, 1)
    assert o["bin_count"].tolist() == [7] and o["bin_conf_min"][0] == o["score"].min() and o["bin_conf_max"][0] == o["score"].max()
    matches_restatement(o, y, sizes, None, 0, K, 1, "7 rows, 1 bin")
    o = c_grouped(head, X, y, sizes, None, 0, 64)
    matches_restatement(o, y, sizes, None, 0, K, 64, "7 rows, 64 bins")


# ---- 7. the C ABI's argument checks ----

def test_malformed_group_arguments_are_rejected_before_any_launch():
    from mermaid_classifier_amd import _lib
    head = _load("head_fixture")._head
    K = head.n_classes
    X = _rows_of("head_fixture", 20)
    y = (np.arange(20) % K).astype(np.int32)
    sizes, source = np.array([5, 5, 10]), [0, 1, 1]
    good = c_grouped(head, X, y, sizes, source, 2, 4)
    E = _lib.MMC_ERR_ARG

    def rejected(what, **kw):
        args = dict(sizes=sizes, source=source, n_sources=2, n_bins=4)
        args.update(kw)
        o = c_grouped(head, X, args.pop("y", y), expect=E, **args)
        assert what.encode() in _lib.lib().mmc_last_error(), (what, _lib.lib().mmc_last_error())
        nb = args["n_bins"]
        for k, v in o.items():
            if k in PER_ROW:
                continue                                                           # (per-row outputs are not tables)
            if k.startswith("bin_") and not 1 <= nb <= 64:
                continue                                                           # (their length is n_bins)
            if k == "source_confusion" and not 0 < args["n_sources"] * K * K <= (1 << 26):
                continue                                                           # (its size is n_sources * K * K)
            assert not np.asarray(v).any(), (what, k)

    rejected("image_offsets[0] = 1: must be 0", offsets=[1, 5, 10, 20])
    rejected("offsets increase strictly", offsets=[0, 5, 5, 20])
    rejected("offsets increase strictly", offsets=[0, 12, 10, 20])
    rejected("must be n = 20", offsets=[0, 5, 10, 19])
    rejected("must be n = 20", offsets=[0, 5, 10, 21])
    rejected("every image owns at least one row", offsets=np.arange(22), source=[0] * 21)
    rejected("source_of_image[2] = 2 outside [0, 2)", source=[0, 1, 2])
    rejected("source_of_image[0] = -1 outside [0, 2)", source=[-1, 1, 1])
    rejected("n_sources = -1 is negative", n_sources=-1)
    rejected("n_bins = 0 outside [1, 64]", n_bins=0)
    rejected("n_bins = 65 outside [1, 64]", n_bins=65)
    rejected("cells of per-source confusion", n_sources=(1 << 26) // (K * K) + 1)
    rejected("label index y[0] = 5 outside [0, 5)", y=np.where(np.arange(20) == 0, 5, y).astype(np.int32))
    lib = _lib.lib()
    tot = np.full(5, -7, np.int64)
    offs = np.array([0, 5, 10, 20], np.int64)
    args = [None, 0, None, None, None, None, tot.ctypes.data, None, None, None, 3, None, 0, 4] + [None] * 11
    assert lib.mmc_head_evaluate_grouped(head._h, X.ctypes.data, y.ctypes.data, 20, *args, _lib.MMC_IN_HOST, None) == E
    assert b"image_offsets is NULL" in lib.mmc_last_error() and not tot.any()
    args[9] = offs.ctypes.data
    args[6] = None
    assert lib.mmc_head_evaluate_grouped(head._h, X.ctypes.data, y.ctypes.data, 20, *args, _lib.MMC_IN_HOST, None) == E
    assert b"totals is NULL" in lib.mmc_last_error()
    args[6] = tot.ctypes.data                                                      # every group output NULL: the totals still come back
    assert lib.mmc_head_evaluate_grouped(head._h, X.ctypes.data, y.ctypes.data, 20, *args, _lib.MMC_IN_HOST, None) == _lib.MMC_OK
    assert np.array_equal(tot, good["totals"])
    # the image-count cap, through a head of many classes
    from mermaid_classifier_amd.inference import DeviceHead, HeadParams
    rng = np.random.default_rng(5)
    KW = 2500
    wide = DeviceHead(HeadParams([rng.normal(0, 0.5, (KW, 8)).astype(np.float32)], [np.zeros(KW, np.float32)],
                                 np.full(KW, -10, np.float32), np.full(KW, 2, np.float32)))
    m = (1 << 28) // KW + 1
    tot[:] = -7
    offs = np.arange(m + 1, dtype=np.int64)
    args = [None, 0, None, None, None, None, tot.ctypes.data, None, None, offs.ctypes.data, m, None, 0, 4] + [None] * 11
    Xw, yw = np.zeros((m, 8), np.float32), np.zeros(m, np.int32)
    assert lib.mmc_head_evaluate_grouped(wide._h, Xw.ctypes.data, yw.ctypes.data, m, *args, _lib.MMC_IN_HOST, None) == E
    assert b"cells of per-image counts" in lib.mmc_last_error() and not tot.any()
    wide.close()
    same_bits(good, c_grouped(head, X, y, sizes, source, 2, 4))                    # a good call after the rejected ones


# ---- 8. the Python layer ----

def test_grouped_validate_agrees_with_validate_and_the_restatement():
    from mermaid_classifier_amd import FeatureSet, grouped_validate, validate
    pred = _load("head108")
    K = len(pred.classes)
    n = 1000
    rng = np.random.default_rng(14)
    X = _rows_of("head108", n)
    _, arg = pred._head.predict(X)
    yi = np.where(rng.random(n) < 0.5, arg, rng.integers(0, K, n))
    labels = np.asarray(pred.classes)[yi]
    sizes = _sizes(rng, n, 30)
    source = rng.integers(0, 5, len(sizes))
    plain = validate(pred, (X, labels))
    gv = grouped_validate(pred, (X, labels), sizes, source_of_image=source, n_bins=20, rows=True)
    for name in ("gt", "est", "scores", "ranks", "p_true", "confusion", "rank_hist"):
        assert np.array_equal(getattr(gv.validation, name), getattr(plain, name)), name
    for name in ("classes", "n", "n_correct", "n_unknown", "n_nonfinite", "nll_q32", "accuracy", "log_loss", "mrr"):
        assert getattr(gv.validation, name) == getattr(plain, name), name
    want = restate(plain.gt, plain.est, plain.scores.astype(np.float32), plain.p_true, sizes, source, 5, K, 20)
    assert np.array_equal(gv.sources.confusion, want["source_confusion"]) and gv.cover.n_images_used == len(sizes)
    for k in ("support", "nll_q32", "score_q32"):
        assert np.array_equal(getattr(gv, k), want[k]), k
    for k, col in (("count", "bin_count"), ("n_correct", "bin_correct"), ("conf_q32", "bin_conf_q32")):
        assert np.array_equal(getattr(gv.reliability, k), want[col]), k
    assert gv.sources.confusion.sum(0).tolist() == plain.confusion.tolist()
    assert 0.0 <= gv.reliability.ece <= 1.0 and len(gv.reliability.bins) == 20 and len(gv.cover.table()["class"]) >= 1
    assert sum(v["n_samples"] for v in gv.by_class(np.arange(K) % 3, min_samples=1).values()) == n
    # a resident set with one class more than the model goes through a label map; totals only
    fs = FeatureSet(pred.input_dim, list(pred.classes) + ["zz::extra"]).append(X, labels)
    gs = grouped_validate(pred, fs, sizes, source_of_image=source)
    assert not gs.validation.has_rows and gs.validation.nll_q32 == plain.nll_q32
    assert np.array_equal(gs.validation.confusion, plain.confusion) and np.array_equal(gs.sources.confusion, gv.sources.confusion)
    assert gs.cover.sums.tobytes() == gv.cover.sums.tobytes() and gs.reliability.ece == gv.reliability.ece
    fs.close()


# ---- the host paths every entry point shares: one handle's growing buffers, the padded input, a set slice ----

def test_interleaved_entry_points_on_one_handle_match_fresh_handles():
    """predict, evaluate, top-k and grouped evaluate share one handle's device buffers, and each call grows the ones it needs:
    8 rows, 512, 300, 512, 512, 8 on one head, every output bit for bit the same call's on a head that has done nothing else."""
    from mermaid_classifier_amd.inference import DeviceHead
    from test_gpu_validation import c_evaluate, same_outputs
    params = _load("head_fixture")._head.params
    X = np.load(GOLDEN / "head_fixture_io.npz")["X"]
    assert X.shape == (512, 8)
    rng = np.random.default_rng(5)
    y = rng.integers(0, 5, 512).astype(np.int32)
    sizes = _sizes(rng, 512, 30)
    source = rng.integers(0, 3, len(sizes))
    calls = [lambda h: h.predict(X[:8]),
             lambda h: c_evaluate(h, X, y),
             lambda h: h.topk(X[:300], 3),
             lambda h: c_grouped(h, X, y, sizes, source, 3),
             lambda h: h.predict(X),
             lambda h: h.topk(X[:8], 3)]
    one = DeviceHead(params)
    for i, call in enumerate(calls):
        got, want = call(one), call(DeviceHead(params))
        if isinstance(got, dict) and "support" in got:
            same_bits(got, want)
        elif isinstance(got, dict):
            same_outputs(got, want)
        else:
            for a, b in zip(got, want):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"call {i}"


def test_input_width_that_is_no_multiple_of_4_matches_the_zero_padded_twin():
    """A 6 -> 16 -> 5 head pads its rows to 8 columns on the device (memset + strided copy, for host rows, device rows and a feature
    set alike); its twin 8 -> 16 -> 5 with two zero weight columns, fed the rows with two zero columns, computes on the same
    padded data.  predict, top-k and evaluate of the narrow head must give the twin's bits on every route; 37 rows: the last
    workgroup is ragged."""
    import torch
    from mermaid_classifier_amd import FeatureSet
    from mermaid_classifier_amd.inference import DeviceHead, HeadParams
    from test_gpu_validation import c_evaluate, c_evaluate_set, same_outputs
    rng = np.random.default_rng(6)
    W1, b1 = rng.normal(0, 0.5, (16, 6)).astype(np.float32), rng.normal(0, 0.2, 16).astype(np.float32)
    W2, b2 = rng.normal(0, 0.5, (5, 16)).astype(np.float32), rng.normal(0, 0.2, 5).astype(np.float32)
    a, b = rng.uniform(-9, -4, 5).astype(np.float32), rng.uniform(0.5, 3, 5).astype(np.float32)
    narrow = DeviceHead(HeadParams([W1, W2], [b1, b2], a, b))
    twin = DeviceHead(HeadParams([np.concatenate([W1, np.zeros((16, 2), np.float32)], 1), W2], [b1, b2], a, b))
    assert (narrow.input_dim, twin.input_dim) == (6, 8)
    X6 = rng.normal(0.3, 0.6, (37, 6)).astype(np.float32)
    X8 = np.concatenate([X6, np.zeros((37, 2), np.float32)], 1)
    y = rng.integers(0, 5, 37).astype(np.int32)

    def bits(got, want, what):
        for g, w in zip(got, want):
            g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), what

    want_predict, want_topk, want_eval = twin.predict(X8), twin.topk(X8, 3, want_proba=True), c_evaluate(twin, X8, y)
    assert len(np.unique(want_predict[1])) > 1
    xd = torch.from_numpy(X6).cuda()
    bits(narrow.predict(X6), want_predict, "predict, host rows")
    bits(narrow.predict(xd), want_predict, "predict, device rows")
    bits(narrow.topk(X6, 3, want_proba=True), want_topk, "topk, host rows")
    bits(narrow.topk(xd, 3, want_proba=True), want_topk, "topk, device rows")
    same_outputs(c_evaluate(narrow, X6, y), want_eval)
    same_outputs(c_evaluate(narrow, X6, y, device=True), want_eval)
    same_outputs(c_evaluate_set(narrow, FeatureSet(6, list(range(5))).append(X6, y), 0, 37), want_eval)


def test_grouped_set_from_a_later_first_row_matches_the_host_slice():
    """mmc_head_evaluate_grouped_set on rows [11, 512) of a set (the image offsets cover those rows) == mmc_head_evaluate_grouped on
    the host slice, in every table and every bit."""
    head = _load("head_fixture")._head
    X = np.load(GOLDEN / "head_fixture_io.npz")["X"]
    rng = np.random.default_rng(8)
    _, arg = head.predict(X)
    y = np.where(rng.random(512) < 0.6, arg, rng.integers(0, 5, 512)).astype(np.int32)
    sizes = _sizes(rng, 512 - 11, 30)
    source = rng.integers(0, 3, len(sizes))
    host = c_grouped(head, X[11:], y[11:], sizes, source, 3)
    sliced = c_grouped(head, None, y[11:], sizes, source, 3, fs=_set_of(head, X, y), first=11)
    same_bits(host, sliced)
    assert host["totals"][0] == 501 and host["support"].sum() == 501 and (host["est"] >= 0).all()
