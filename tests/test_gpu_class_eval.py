"""Class-wise evaluation on the device -- ``mmc_trainer_evaluate_classes`` / ``_set`` (csrc/calib.hip, ``eval_rows_kernel<CONF>``),
``calibration.evaluate_classes`` -- and the balancing sweep end to end (``sampling``, ``train_sweep(class_scores=True)``,
``rank_sweep``).

The classifiers are built from explicit parameters (seeded numpy draws, one hidden layer of 16) through
``TorchMLPClassifier.__setstate__``, so the expected table comes from float64 numpy logits of the same parameters.  Rows are drawn
until every kept one has a float64 top-2 logit gap of at least 1e-3 (asserted below): the device's fp32 forward over at most 16
terms of magnitude ~1 errs by ~1e-6, so it cannot move an argmax, and the tables compare with ``==``.  The totals compare with
``==`` against ``mmc_trainer_evaluate(_set)_q32`` on the same rows: the per-row arithmetic is the same instantiation's.

Shapes: K = 3, 65 (the first K past the 64 lanes) and 108 (production); n = 1, 4, 5 (four rows per workgroup); 16 384 + 3 rows
(two chunks: accumulation, scratch reuse); 6 columns (rows that are not 16-byte sized).  In every case class 0 is absent from y
and class K - 1 is never predicted (its output bias is -30)."""

import ctypes as C
import functools

import numpy as np
import pytest

GAP = 1e-3


def _build(ws, bs, K):
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    proto = TorchMLPClassifier(hidden_layer_sizes=tuple(int(w.shape[0]) for w in ws[:-1]))
    clf = TorchMLPClassifier.__new__(TorchMLPClassifier)
    state = {k: v for k, v in proto.__dict__.items() if k != "_h"}
    state.update(classes_=np.arange(K), n_features_in_=int(ws[0].shape[1]), n_iter_=1, loss_curve_=[0.0], _class_weight_vector=None,
                 _module_state=([np.ascontiguousarray(w, dtype=np.float32) for w in ws],
                                [np.ascontiguousarray(b, dtype=np.float32) for b in bs]))
    clf.__setstate__(state)
    return clf


def _logits64(ws, bs, X):
    h = X.astype(np.float64)
    for i, (w, b) in enumerate(zip(ws, bs)):
        h = h @ w.astype(np.float64).T + b.astype(np.float64)
        if i < len(ws) - 1:
            h = np.maximum(h, 0.0)
    return h


@functools.lru_cache(maxsize=None)
def _case(K, dim, n, seed):
    """-> (ws, bs, X, y, est): parameters, n rows whose float64 top-2 logit gap is >= GAP, labels without class 0, and the float64
    argmax.  Computed once per shape and left unchanged."""
    rng = np.random.default_rng(seed)
    ws = [rng.normal(0, 0.6, (16, dim)).astype(np.float32), rng.normal(0, 0.8, (K, 16)).astype(np.float32)]
    bs = [rng.normal(0, 0.3, 16).astype(np.float32), rng.normal(0, 0.3, K).astype(np.float32)]
    bs[1][K - 1] = -30.0                                                    # never the argmax
    cand = rng.normal(0, 1, (n + n // 4 + 64, dim)).astype(np.float32)
    top2 = np.sort(_logits64(ws, bs, cand), axis=1)[:, -2:]
    X = np.ascontiguousarray(cand[(top2[:, 1] - top2[:, 0]) >= GAP][:n])
    assert X.shape == (n, dim)
    z = _logits64(ws, bs, X)
    est = z.argmax(1)
    y = np.where(rng.random(n) < 0.6, est, rng.integers(1, K, n))
    y = np.where(y == 0, K - 1, y).astype(np.int32)                          # class 0 is absent from y
    if n >= 4:
        y[n - 1] = K - 1                                                    # the never-predicted class has support
    for a in (X, y, est):
        a.setflags(write=False)
    return ws, bs, X, y, est


def _want_table(K, y, est):
    t = np.zeros((K, K), np.int64)
    np.add.at(t, (y, est), 1)
    return t


def _classes_host(clf, X, y, K, fill=7):
    from mermaid_classifier_amd import _lib
    nc, q = C.c_int64(fill), C.c_int64(fill)
    table = np.full((K, K), fill, np.int64)
    X, y = np.ascontiguousarray(X), np.ascontiguousarray(y)
    status = _lib.lib().mmc_trainer_evaluate_classes(clf._h, X.ctypes.data, y.ctypes.data, len(y), C.byref(nc), C.byref(q),
                                                     table.ctypes.data, None)
    return status, int(nc.value), int(q.value), table


def _classes_set(clf, fs, first, n, K, fill=7):
    from mermaid_classifier_amd import _lib
    nc, q = C.c_int64(fill), C.c_int64(fill)
    table = np.full((K, K), fill, np.int64)
    status = _lib.lib().mmc_trainer_evaluate_classes_set(clf._h, fs._handle(), first, n, C.byref(nc), C.byref(q), table.ctypes.data, None)
    return status, int(nc.value), int(q.value), table


def _plain_host(clf, X, y):
    from mermaid_classifier_amd import _lib
    nc, q = C.c_int64(0), C.c_int64(0)
    X, y = np.ascontiguousarray(X), np.ascontiguousarray(y)
    _lib.check(_lib.lib().mmc_trainer_evaluate_q32(clf._h, X.ctypes.data, y.ctypes.data, len(y), C.byref(nc), C.byref(q), None))
    return int(nc.value), int(q.value)


def _plain_set(clf, fs, first, n):
    from mermaid_classifier_amd import _lib
    nc, q = C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.lib().mmc_trainer_evaluate_set_q32(clf._h, fs._handle(), first, n, C.byref(nc), C.byref(q), None))
    return int(nc.value), int(q.value)


def test_c_abi_argument_errors_without_device():
    """A NULL trainer is rejected before anything is looked at; the two totals are zeroed."""
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    assert {"mmc_trainer_evaluate_classes", "mmc_trainer_evaluate_classes_set"} <= set(_lib.SYMBOLS)
    table = np.full((3, 3), 7, np.int64)
    for call in (lambda nc, q: lib.mmc_trainer_evaluate_classes(None, None, None, 1, C.byref(nc), C.byref(q), table.ctypes.data, None),
                 lambda nc, q: lib.mmc_trainer_evaluate_classes_set(None, None, 0, 1, C.byref(nc), C.byref(q), table.ctypes.data, None)):
        nc, q = C.c_int64(7), C.c_int64(7)
        assert call(nc, q) == _lib.MMC_ERR_ARG and b"trainer handle is NULL" in lib.mmc_last_error()
        assert nc.value == 0 and q.value == 0
    assert (table == 7).all()                                               # K is unknown without a trainer: the table is not touched


SHAPES = [(3, 8, 1), (3, 8, 4), (3, 8, 5), (65, 8, 203), (108, 8, 16384 + 3), (108, 6, 333), (65, 6, 5)]


def _check_preconditions(K, dim, n):
    ws, bs, X, y, est = _case(K, dim, n, 1000 + K + n)
    top2 = np.sort(_logits64(ws, bs, X), axis=1)[:, -2:]
    gap = float((top2[:, 1] - top2[:, 0]).min())
    print(f"K {K} dim {dim} n {n}: smallest float64 top-2 logit gap {gap:.3e}")
    assert gap >= GAP                                                       # fp32 rounding cannot move an argmax
    assert 0 not in set(y.tolist()) and K - 1 not in set(est.tolist()) and (n < 4 or K - 1 in set(y.tolist()))
    # why GAP is enough: an a-priori bound on the fp32 forward's logit error (u = 2^-24 per operation, d + 2 and 16 + 2 operations per
    # dot product and bias, the hidden layer's error carried through |W2|) stays below GAP / 2 on every row
    u = 2.0 ** -24
    a1 = np.abs(X).astype(np.float64) @ np.abs(ws[0]).astype(np.float64).T + np.abs(bs[0])
    w2 = np.abs(ws[1]).astype(np.float64)
    err = (16 + 2) * u * (a1 @ w2.T + np.abs(bs[1])) + ((dim + 2) * u * a1) @ w2.T
    print(f"  a-priori fp32 logit error bound {err.max():.3e}")
    assert 2 * err.max() < GAP


@pytest.mark.parametrize("K,dim,n", SHAPES)
def test_the_cases_meet_their_preconditions(K, dim, n):
    """Host only: the seeds were picked so that the generator's conditions hold for every shape."""
    _check_preconditions(K, dim, n)


@pytest.mark.gpu
@pytest.mark.parametrize("K,dim,n", SHAPES)
def test_class_table_and_totals(K, dim, n):
    from mermaid_classifier_amd import FeatureSet, _lib
    ws, bs, X, y, est = _case(K, dim, n, 1000 + K + n)
    _check_preconditions(K, dim, n)
    want = _want_table(K, y, est)
    clf = _build(ws, bs, K)
    fs = FeatureSet(dim, np.arange(K), reserve=n).append(X, y)

    # the totals carry the bits of the plain calls; the table is numpy's; both forms agree
    plain_h, plain_s = _plain_host(clf, X, y), _plain_set(clf, fs, 0, n)
    st_h, nc_h, q_h, tab_h = _classes_host(clf, X, y, K)
    st_s, nc_s, q_s, tab_s = _classes_set(clf, fs, 0, n, K)
    assert st_h == st_s == _lib.MMC_OK
    print(f"  n_correct {nc_h} sum_q32 {q_h}; plain host {plain_h} set {plain_s}; table cells differing from numpy "
          f"{int((tab_h != want).sum())} / {int((tab_s != want).sum())}")
    assert (nc_h, q_h) == plain_h == plain_s == (nc_s, q_s)
    assert np.array_equal(tab_h, want) and np.array_equal(tab_s, want)
    assert int(np.trace(tab_h)) == nc_h == int((y == est).sum())
    assert np.array_equal(tab_h.sum(1), np.bincount(y, minlength=K))
    assert tab_h[0].sum() == 0 and tab_h[:, K - 1].sum() == 0                # the absent class and the never-predicted class

    # the plain calls after the class-wise ones still give their totals (the scratch is shared, with another layout)
    assert _plain_host(clf, X, y) == plain_h and _plain_set(clf, fs, 0, n) == plain_s
    # a repeated call returns the same table: the device table is zeroed per call
    assert np.array_equal(_classes_set(clf, fs, 0, n, K)[3], want) and np.array_equal(_classes_host(clf, X, y, K)[3], want)

    # two calls on a split of the rows add up (n = 1: one row and none)
    cut = n // 2 + 1 if n > 1 else 1
    for parts in ([_classes_set(clf, fs, 0, cut, K), _classes_set(clf, fs, cut, n - cut, K)],
                  [_classes_host(clf, X[:cut], y[:cut], K), _classes_host(clf, X[cut:], y[cut:], K)]):
        assert all(p[0] == _lib.MMC_OK for p in parts)
        assert parts[0][1] + parts[1][1] == nc_h and parts[0][2] + parts[1][2] == q_h
        assert np.array_equal(parts[0][3] + parts[1][3], want)
        assert np.array_equal(parts[0][3], _want_table(K, y[:cut], est[:cut]))
    fs.close()


@pytest.mark.gpu
def test_evaluate_classes_equals_evaluate():
    """The Python entry: a resident set through ``_set``, batches through the host-fed call with the tables added."""
    from mermaid_classifier_amd import ClassScores, FeatureSet, evaluate, evaluate_classes
    K, dim, n = 65, 8, 203
    ws, bs, X, y, est = _case(K, dim, n, 1000 + K + n)
    clf = _build(ws, bs, K)
    fs = FeatureSet(dim, np.arange(K)).append(X, y)
    want = _want_table(K, y, est)
    batches = [(X[:50], y[:50]), (X[50:51], y[50:51]), (X[51:], y[51:])]
    for data in (fs, (X, y), batches):
        acc, loss, cs = evaluate_classes(clf, data)
        assert (acc, loss) == evaluate(clf, data)
        assert isinstance(cs, ClassScores) and np.array_equal(cs.confusion, want) and cs.classes == list(range(K))
        assert cs.accuracy == acc
    with pytest.raises(ValueError, match="no rows"):
        evaluate_classes(clf, [])
    fs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [65, 108])
def test_ties_land_in_the_first_class(K):
    """An all-zero last layer makes every logit exactly equal: the argmax is the first index, on both sides of the 64 lanes."""
    from mermaid_classifier_amd import FeatureSet, _lib
    ws, bs, X, y, _ = _case(K, 8, 203, 1000 + K + 203) if K == 65 else _case(K, 6, 333, 1000 + K + 333)
    ws, bs = [ws[0], np.zeros_like(ws[1])], [bs[0], np.zeros_like(bs[1])]
    clf = _build(ws, bs, K)
    fs = FeatureSet(X.shape[1], np.arange(K)).append(X, y)
    want = _want_table(K, y, np.zeros(len(y), np.int64))
    for status, nc, q, table in (_classes_host(clf, X, y, K), _classes_set(clf, fs, 0, len(y), K)):
        assert status == _lib.MMC_OK and nc == 0 and np.array_equal(table, want)      # y never holds class 0
        assert (nc, q) == _plain_host(clf, X, y)
    fs.close()


@pytest.mark.gpu
def test_rejected_calls_zero_the_outputs_and_leave_the_trainer_usable():
    from mermaid_classifier_amd import FeatureSet, _lib
    lib = _lib.lib()
    K, dim, n = 65, 8, 203
    ws, bs, X, y, est = _case(K, dim, n, 1000 + K + n)
    clf = _build(ws, bs, K)
    fs = FeatureSet(dim, np.arange(K)).append(X, y)
    other = FeatureSet(6, np.arange(K)).append(X[:, :6], y)                  # a set of another width
    want = _want_table(K, y, est)
    good = _classes_set(clf, fs, 0, n, K)
    assert good[0] == _lib.MMC_OK and np.array_equal(good[3], want)

    def follow_up():
        for got in (_classes_host(clf, X, y, K), _classes_set(clf, fs, 0, n, K)):
            assert got[0] == _lib.MMC_OK and got[1:3] == good[1:3] and np.array_equal(got[3], want)

    # NULL confusion: MMC_ERR_ARG, the two totals zeroed
    Xc, yc = np.ascontiguousarray(X), np.ascontiguousarray(y)
    for call in (lambda nc, q: lib.mmc_trainer_evaluate_classes(clf._h, Xc.ctypes.data, yc.ctypes.data, n, C.byref(nc), C.byref(q), None, None),
                 lambda nc, q: lib.mmc_trainer_evaluate_classes_set(clf._h, fs._handle(), 0, n, C.byref(nc), C.byref(q), None, None)):
        nc, q = C.c_int64(7), C.c_int64(7)
        assert call(nc, q) == _lib.MMC_ERR_ARG and b"confusion is NULL" in lib.mmc_last_error()
        assert nc.value == 0 and q.value == 0
    follow_up()
    # a label equal to K
    bad = y.copy()
    bad[n - 1] = K
    status, nc, q, table = _classes_host(clf, X, bad, K)
    assert status == _lib.MMC_ERR_ARG and b"outside [0, 65)" in lib.mmc_last_error()
    assert nc == 0 and q == 0 and not table.any()
    follow_up()
    # a set of another width; rows outside the set
    status, nc, q, table = _classes_set(clf, other, 0, n, K)
    assert status == _lib.MMC_ERR_ARG and b"feature set has 6 columns" in lib.mmc_last_error()
    assert nc == 0 and q == 0 and not table.any()
    status, nc, q, table = _classes_set(clf, fs, n - 3, 4, K)
    assert status == _lib.MMC_ERR_ARG and b"outside the set's" in lib.mmc_last_error() and nc == 0 and q == 0 and not table.any()
    follow_up()
    fs.close()
    other.close()


def _clusters(rng, sizes):
    """Three overlapping clusters in 8 dimensions, the rows of the classes interleaved at random."""
    centres = rng.normal(0, 1.0, (3, 8))
    y = rng.permutation(np.repeat(np.arange(3), sizes))
    return (centres[y] + rng.normal(0, 1.2, (len(y), 8))).astype(np.float32), y


@pytest.mark.gpu
def test_balancing_sweep_end_to_end():
    """Arms A and C of the balancing study in miniature: unweighted, effective-number weights, a balanced subsample -- one resident
    train set, one sweep.  ``class_scores=True`` changes nothing that is returned, and ``rank_sweep`` is ``validate`` per model."""
    from mermaid_classifier_amd import (FeatureSet, SweepConfig, class_counts, effective_number_weights, evaluate_classes, grouped_validate,
                                        rank_sweep, row_batches, subsample_rows, subsample_targets, train_sweep, validate)
    rng = np.random.default_rng(11)
    (Xt, yt), (Xr, yr), (Xv, yv) = _clusters(rng, [300, 80, 20]), _clusters(rng, [60, 40, 20]), _clusters(rng, [60, 40, 20])
    sets = [FeatureSet(8, np.arange(3)).append(X, y) for X, y in ((Xt, yt), (Xr, yr), (Xv, yv))]
    counts = class_counts(sets[0])
    assert counts.tolist() == [300, 80, 20]
    weights = effective_number_weights({k: int(c) for k, c in enumerate(counts)}, beta=0.99)
    targets = subsample_targets({k: int(c) for k, c in enumerate(counts)}, "balanced", 150, min_per_class=10)
    assert targets == {0: 50, 1: 50, 2: 20}
    rows = subsample_rows(sets[0], targets)
    assert np.bincount(yt[rows]).tolist() == [50, 50, 20]
    base = dict(hidden_layer_sizes=(16,), learning_rate_init=1e-2, random_state=0, batch_size=40)
    configs = [SweepConfig(**base), SweepConfig(**base, class_weight=weights), SweepConfig(**base, batches=row_batches(rows, 60))]
    runs = {}
    for flag in (False, True):
        seen = []
        runs[flag] = (train_sweep(*sets, configs, 2, batch_size=200, on_epoch_end=seen.append, class_scores=flag), seen)
    for (cal, info, accs), (cal0, info0, accs0) in zip(runs[True][0], runs[False][0]):
        assert info == info0 and accs == accs0
        for u, v in zip(cal.weights + cal.biases, cal0.weights + cal0.biases):
            assert np.array_equal(u, v)
        assert np.array_equal(cal.a_, cal0.a_) and np.array_equal(cal.b_, cal0.b_)
    extra = {"val_balanced_accuracy", "val_f1_macro"}
    strip = lambda ms: [{k: v for k, v in m.items() if k not in extra | {"cumulative_seconds"}} for m in ms]
    assert strip(runs[True][1]) == strip(runs[False][1]) and len(runs[True][1]) == 6
    assert all(extra <= set(m) for m in runs[True][1]) and not any(extra & set(m) for m in runs[False][1])

    results = runs[True][0]
    ranked = rank_sweep(results, sets[2])
    want = []
    for i, (cal, info, _) in enumerate(results):
        v = validate(cal, sets[2], rows=False)
        cs = v.class_scores()
        want.append({"config": i, "balanced_accuracy": cs.balanced_accuracy, "f1_macro": cs.f1_macro, "accuracy": v.accuracy,
                     "mcc": cs.mcc, "log_loss": v.log_loss, "best_val_epoch": info["best_val_epoch"], "final_epoch": info["final_epoch"]})
        # the table behind the scores is the one the labels give
        est = cal.predict(Xv)
        table = np.zeros((3, 3), np.int64)
        np.add.at(table, (yv, est), 1)
        assert np.array_equal(cs.confusion, table)
    want.sort(key=lambda r: (-r["balanced_accuracy"], -r["f1_macro"], r["config"]))
    print("ranking:", [(r["config"], round(r["balanced_accuracy"], 4), round(r["f1_macro"], 4)) for r in ranked])
    assert ranked == want and sorted(r["config"] for r in ranked) == [0, 1, 2]
    sizes = np.full(12, 10)
    with_cover = rank_sweep(results, sets[2], image_sizes=sizes, n_bins=5)
    assert [r["config"] for r in with_cover] == [r["config"] for r in ranked]
    for r, plain in zip(with_cover, ranked):
        g = grouped_validate(results[r["config"]][0], sets[2], sizes, n_bins=5)
        assert {k: v for k, v in r.items() if k not in ("cover_median_r_squared", "ece")} == plain
        assert r["ece"] == g.reliability.ece
        a, b = r["cover_median_r_squared"], g.cover.scalars()["cover_median_r_squared"]
        assert a == b or (np.isnan(a) and np.isnan(b))
    # the last epoch's callback entries are the class-wise evaluation of the returned (uncalibrated) parameters: without early
    # stopping the returned model is the last epoch's
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier   # noqa: F401
    last = [m for m in runs[True][1] if m["epoch"] == 1]
    for m in last:
        cal = results[m["config"]][0]
        clf = _build(cal.weights, cal.biases, 3)
        acc, loss, cs = evaluate_classes(clf, sets[2])
        assert (acc, loss) == (m["val_accuracy"], m["val_loss"])
        assert (cs.balanced_accuracy, cs.f1_macro) == (m["val_balanced_accuracy"], m["val_f1_macro"])
    for s in sets:
        s.close()
