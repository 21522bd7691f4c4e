"""Feature transforms on the MI355X (csrc/features.hip, mermaid_classifier_amd/feature_transform.py) against the float64 checker
of tests/feature_transform_checker.py, per element, at the smallest shapes that reach every edge: empty and single-row classes,
ranges that start inside a set, below / exactly / just above one 256-row chunk, every chunk range holding two chunks, one partial
tile, a full plus a ragged tile, an off-diagonal tile pair, and one production-width case.  The bounds are derived in the checker's
header; every gate is 1 x."""

import ctypes as C
import json

import numpy as np
import pytest

import feature_transform_checker as ck
from conftest import check_labels

pytestmark = pytest.mark.gpu

K = 5                    # class 3 is empty, class 4 has a single row
FIRST, TAIL = 13, 5      # rows of the set before and after the range under test

# max |p - float64 evaluation of the same parameters| over the 120 validation rows of the end-to-end case, measured on an MI355X
# (profiles/feature_transform.txt): 1.75e-7 on the transformed route, 8.11e-7 on the folded route.  The seeds are fixed; the gate is
# 4 x the larger, the margin being for how expf is scheduled from one box to the next.
DP_MEASURED = (1.75e-7, 8.11e-7)
DP_GATE = 4 * max(DP_MEASURED)


def _rows(n, dim, seed):
    """FIRST + n + TAIL rows; the range under test has labels in {0, 1, 2} plus one row of class 4, the rows around it are far off
    and carry every class, so a range error shows."""
    X, yi = ck.reef_like(FIRST + n + TAIL, dim, 3, seed=seed)
    yi[FIRST + n // 2] = 4
    outside = np.r_[0:FIRST, FIRST + n:FIRST + n + TAIL]
    X[outside] = X[outside] * 3 + 50
    yi[outside] = np.arange(len(outside)) % K
    return X, yi


def _set(X, yi, dim):
    from mermaid_classifier_amd import FeatureSet
    return FeatureSet(dim, np.arange(K)).append(X, yi)


@pytest.mark.parametrize("dim", [8, 72])
@pytest.mark.parametrize("n", [1, 77, 257, 1031])
def test_moments(dim, n):
    from mermaid_classifier_amd.feature_transform import moments
    X, yi = _rows(n, dim, seed=100 + n + dim)
    fs = _set(X, yi, dim)
    counts, mean, m2 = moments(fs, FIRST, n)
    again = moments(fs, FIRST, n)
    fs.close()
    sl = slice(FIRST, FIRST + n)
    r_counts, r_mean, r_m2, b_mean, b_m2 = ck.moments(X[sl], yi[sl], K)
    assert np.array_equal(counts, r_counts) and counts[3] == 0 and counts[4] == 1
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(m2))
    assert not mean[3].any() and not m2[3].any() and not m2[4].any()               # empty: zeros; a single row: no deviation
    assert np.array_equal(mean[4], X[FIRST + n // 2].astype(np.float64))
    e_mean = np.abs(mean.astype(np.longdouble) - r_mean).astype(np.float64)
    e_m2 = np.abs(m2.astype(np.longdouble) - r_m2).astype(np.float64)
    ratio = lambda e, b: float(np.where(b > 0, e / np.where(b > 0, b, 1), np.where(e > 0, np.inf, 0)).max())
    print(f"moments dim {dim} n {n}: worst |mean err| / bound {ratio(e_mean, b_mean):.3g}, |m2 err| / bound {ratio(e_m2, b_m2):.3g}")
    assert np.all(e_mean <= b_mean) and np.all(e_m2 <= b_m2)
    for a, b in zip((counts, mean, m2), again):
        assert np.array_equal(a, b)                                                 # a repeated call: identical bits


def _check_scatter(fs, X, yi, n, what):
    """total and by-label scatter of rows [FIRST, FIRST + n) about the device's own fp32 centres -> the worst ratios"""
    from mermaid_classifier_amd.feature_transform import moments, scatter_matrix
    sl = slice(FIRST, FIRST + n)
    counts, mean, m2 = moments(fs, FIRST, n)
    _, _, _, _, b_m2 = ck.moments(X[sl], yi[sl], K)
    worst = {}
    for name, centres, labels in (("G=1", mean[K].astype(np.float32), None), ("G=K", mean[:K].astype(np.float32), yi[sl])):
        S = scatter_matrix(fs, centres, FIRST, n)
        Xc = ck.centred(X[sl], centres, labels)
        ref, bound = ck.scatter(Xc)
        err = np.abs(S - ref)
        worst[name] = float(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)).max())
        assert np.all(err <= bound), f"{what} {name}: {int((err > bound).sum())} elements over, worst {worst[name]:.3g}"
        assert np.array_equal(S, S.T)                                               # symmetric, bit for bit
        assert np.array_equal(S, scatter_matrix(fs, centres, FIRST, n))             # a repeated call: identical bits
        if labels is not None:
            # diag(S) is sum_c m2_c up to the two bounds -- and up to what separates the two definitions: the operands of S are
            # fl32(x - c32), each within 2^-24 of x - c32 (so a square within 2^-23 (1 + 2^-25)), and about c32 instead of the
            # class mean mu_c a class's sum of squares is larger by exactly n_c (c32 - mu_c)^2
            operand = 2.0 ** -23 * (1 + 2.0 ** -25) * np.diag(ref)
            cast = (counts[:, None] * (centres.astype(np.float64) - mean[:K]) ** 2).sum(axis=0)
            gap = np.abs(np.diag(S) - m2[:K].sum(axis=0))
            assert np.all(gap <= np.diag(bound) + b_m2[:K].sum(axis=0) + operand + cast)
    print(f"scatter {what}: worst |err| / bound {worst}")
    return worst


@pytest.mark.parametrize("dim", [8, 72, 200])
@pytest.mark.parametrize("n", [1, 77, 256, 259, 16 * 256 * 2 + 5])
def test_scatter(dim, n):
    X, yi = _rows(n, dim, seed=200 + n % 1000 + dim)
    fs = _set(X, yi, dim)
    try:
        _check_scatter(fs, X, yi, n, f"dim {dim} n {n}")
    finally:
        fs.close()


def test_scatter_production_width():
    n, dim = 3000, 1280
    X, yi = _rows(n, dim, seed=77)
    fs = _set(X, yi, dim)
    try:
        _check_scatter(fs, X, yi, n, f"dim {dim} n {n}")
    finally:
        fs.close()


def test_scatter_odd_width_takes_the_scalar_staging():
    """dim = 10 is no multiple of 4: the staging loads element by element."""
    X, yi = _rows(300, 10, seed=31)
    fs = _set(X, yi, 10)
    try:
        _check_scatter(fs, X, yi, 300, "dim 10 n 300")
    finally:
        fs.close()


def _transform(src, first, n, centre, T, dst):
    from mermaid_classifier_amd import _lib
    _lib.check(_lib.lib().mmc_featureset_transform(src._handle(), first, n, centre.ctypes.data, T.ctypes.data, T.shape[0],
                                                   dst._handle(), _lib.MMC_IN_HOST, None))


@pytest.mark.parametrize("dim", [72, 1280])
@pytest.mark.parametrize("n", [1, 259])
@pytest.mark.parametrize("m_kind", ["1", "64", "dim"])
def test_transform(dim, n, m_kind):
    from mermaid_classifier_amd import FeatureSet
    m = dim if m_kind == "dim" else int(m_kind)
    X, yi = _rows(n, dim, seed=300 + n + dim)
    rng = np.random.default_rng(m + n)
    centre = X[FIRST:FIRST + max(n, 2)].mean(axis=0).astype(np.float32)
    T = np.ascontiguousarray(rng.normal(0, 1.0 / np.sqrt(dim), (m, dim)).astype(np.float32))
    src = _set(X, yi, dim)
    head = rng.normal(0, 1, (3, m)).astype(np.float32)
    dst = FeatureSet(m, np.arange(K)).append(head, [4, 0, 2])       # no reserve: the append below has to grow the set
    _transform(src, FIRST, n, centre, T, dst)
    assert len(dst) == 3 + n and len(src) == FIRST + n + TAIL
    Y, labels = dst.read()
    assert np.array_equal(Y[:3], head) and np.array_equal(labels[:3], [4, 0, 2])   # the rows already there are untouched
    assert np.array_equal(labels[3:], yi[FIRST:FIRST + n])
    ref, bound = ck.transform(ck.centred(X[FIRST:FIRST + n], centre), T)
    err = np.abs(Y[3:].astype(np.float64) - ref)
    print(f"transform dim {dim} n {n} m {m}: worst |err| / bound {float((err / bound).max()):.3g}")
    assert np.all(err <= bound)
    src.close()
    dst.close()


def test_rejected_calls_change_nothing():
    from mermaid_classifier_amd import FeatureSet
    from mermaid_classifier_amd.feature_transform import moments, scatter_matrix
    dim = 12
    X, yi = _rows(40, dim, seed=4)
    src = _set(X, yi, dim)
    centre = np.zeros(dim, np.float32)
    T = np.ascontiguousarray(np.eye(7, dim, dtype=np.float32))
    head = np.arange(14, dtype=np.float32).reshape(2, 7)
    dst = FeatureSet(7, np.arange(K)).append(head, [1, 2])
    wrong_width = FeatureSet(8, np.arange(K)).append(np.zeros((1, 8), np.float32), [0])
    other_classes = FeatureSet(7, np.arange(K + 1)).append(np.zeros((1, 7), np.float32), [0])
    total = len(src)
    for args, target, match in (((0, 10), wrong_width, "has width 8"),
                                ((0, 10), other_classes, "classes"),
                                ((total - 3, 4), dst, "outside the set's"),
                                ((-1, 2), dst, "outside the set's")):
        with pytest.raises(ValueError, match=match):
            _transform(src, args[0], args[1], centre, T, target)
    with pytest.raises(ValueError, match="dst is src"):
        _transform(src, 0, 10, centre, np.ascontiguousarray(np.eye(dim, dtype=np.float32)), src)
    assert len(dst) == 2 and len(wrong_width) == 1 and len(other_classes) == 1 and len(src) == total
    Y, labels = dst.read()
    assert np.array_equal(Y, head) and np.array_equal(labels, [1, 2])
    Xs, ys = src.read()
    assert np.array_equal(Xs, X) and np.array_equal(ys, yi)
    with pytest.raises(ValueError, match="outside the set's"):
        moments(src, total - 1, 2)
    with pytest.raises(ValueError, match="outside the set's"):
        scatter_matrix(src, centre, 5, total)
    with pytest.raises(ValueError, match="centres must be"):
        scatter_matrix(src, np.zeros((2, dim), np.float32))
    # n = 0: zeros, nothing appended
    counts, mean, m2 = moments(src, 3, 0)
    assert not counts.any() and not mean.any() and not m2.any() and not scatter_matrix(src, centre, 3, 0).any()
    _transform(src, 3, 0, centre, T, dst)
    assert len(dst) == 2
    wide = FeatureSet(2052, np.arange(K)).append(np.zeros((2, 2052), np.float32), [0, 1])
    with pytest.raises(ValueError, match="MMC_SCATTER_MAX_DIM"):
        scatter_matrix(wide, np.zeros(2052, np.float32))
    for fs in (src, dst, wrong_width, other_classes, wide):
        fs.close()


def test_fit_and_apply_on_the_device():
    """FeatureTransform.fit from a resident set is from_statistics of the device's moments and scatter; apply's rows whiten."""
    from mermaid_classifier_amd import FeatureTransform
    from mermaid_classifier_amd.feature_transform import moments, scatter_matrix
    n, dim = 900, 72
    X, yi = ck.reef_like(n, dim, K, seed=8)
    fs = _set(X, yi, dim)
    counts, mean, m2 = moments(fs)
    for scatter in ("total", "within"):
        centres = (mean[K] if scatter == "total" else mean[:K]).astype(np.float32)
        S = scatter_matrix(fs, centres)
        for kind in ("standardize", "pca", "whiten"):
            ft = FeatureTransform.fit(fs, kind, scatter=scatter, n_components=None if kind == "standardize" else 20)
            want = FeatureTransform.from_statistics(kind, counts, mean, m2, S, scatter=scatter,
                                                    n_components=None if kind == "standardize" else 20)
            assert np.array_equal(ft.components_, want.components_) and np.array_equal(ft.mean_, want.mean_)
            assert np.array_equal(ft.counts_, counts) and np.array_equal(ft.class_means_, mean[:K])
    part = FeatureTransform.fit(fs, "whiten", rows=(100, 500))
    sub = FeatureTransform.from_statistics("whiten", *moments(fs, 100, 500),
                                           scatter_matrix(fs, moments(fs, 100, 500)[1][K].astype(np.float32), 100, 500))
    assert np.array_equal(part.components_, sub.components_) and part.n_rows_ == 500
    ft = FeatureTransform.fit(fs, "whiten", eps=1e-6)
    out = ft.apply(fs)
    Y, labels = out.read()
    assert Y.shape == (n, dim) and np.array_equal(labels, yi) and np.array_equal(out.classes, fs.classes)
    centre, T = ft.device_operands()
    ref, bound = ck.transform(ck.centred(X, centre), T)
    assert np.all(np.abs(Y - ref) <= bound)
    cov = Y.astype(np.float64).T @ Y.astype(np.float64) / n
    print("whitened rows: max |cov - I|", np.abs(cov - np.eye(dim)).max())
    assert np.abs(cov - np.eye(dim)).max() <= 1e-3                                  # eps = 1e-6 and fp32 rows
    fs.close()
    out.close()


# ---- end to end: 16 -> 24 -> 12 -> 7 head, 230 + 120 + 120 rows, 3 epochs ---------------------------------------------------------
E2E_K, E2E_DIM = 7, 16


def _clf():
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    return TorchMLPClassifier(hidden_layer_sizes=(24, 12), learning_rate_init=3e-3, random_state=0, batch_size=50)


def _same_model(a, b):
    assert len(a.weights) == len(b.weights)
    for x, y in zip(a.weights + a.biases, b.weights + b.biases):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert np.array_equal(a.a_, b.a_) and np.array_equal(a.b_, b.b_) and np.array_equal(a.classes_, b.classes_)


@pytest.fixture(scope="module")
def e2e():
    from mermaid_classifier_amd import FeatureSet, FeatureTransform, train_classifier
    X, yi = ck.reef_like(470, E2E_DIM, E2E_K, seed=21, rank=6)
    classes = np.arange(E2E_K)
    cuts = (slice(0, 230), slice(230, 350), slice(350, 470))
    sets = [FeatureSet(E2E_DIM, classes).append(X[s], yi[s]) for s in cuts]
    ft = FeatureTransform.fit(sets[0], "whiten", eps=1e-3)
    folded = train_classifier(*sets, 3, batch_size=100, clf=_clf(), transform={"kind": "whiten", "eps": 1e-3})
    moved = [ft.apply(s) for s in sets]
    unfolded = train_classifier(*moved, 3, batch_size=100, clf=_clf())
    val_t = moved[2].read()[0]
    for s in moved:
        s.close()
    yield dict(X=X, yi=yi, cuts=cuts, sets=sets, ft=ft, folded=folded, unfolded=unfolded, val_raw=X[cuts[2]], val_t=val_t)
    for s in sets:
        s.close()


def test_train_classifier_with_a_transform_returns_the_folded_model(e2e):
    from mermaid_classifier_amd import train_classifier
    ft, (folded, info, accs), (unfolded, info_u, accs_u) = e2e["ft"], e2e["folded"], e2e["unfolded"]
    assert folded.n_features_in_ == E2E_DIM and unfolded.n_features_in_ == E2E_DIM and folded.weights[0].shape == (24, E2E_DIM)
    assert np.array_equal(folded.transform_.components_, ft.components_) and np.array_equal(folded.transform_.mean_, ft.mean_)
    _same_model(folded, unfolded.folded(ft))                        # trained on the transformed sets, then folded: nothing else
    assert info == info_u and accs == accs_u and len(accs) == 3
    with pytest.raises(RuntimeError, match="to_sklearn needs the classifier"):
        folded.to_sklearn()
    # a fitted transform passed in is the dict fitted on train
    again = train_classifier(*e2e["sets"], 3, batch_size=100, clf=_clf(), transform=ft)
    _same_model(again[0], folded)
    assert again[1:] == (info, accs)
    assert all(len(s) == n for s, n in zip(e2e["sets"], (230, 120, 120)))       # the raw splits are as they were

    p_folded = folded.predict_proba(e2e["val_raw"])
    p_unfolded = unfolded.predict_proba(e2e["val_t"])
    r_folded = ck.head_f64(e2e["val_raw"], folded.weights, folded.biases, folded.a_, folded.b_)
    r_unfolded = ck.head_f64(e2e["val_t"], unfolded.weights, unfolded.biases, unfolded.a_, unfolded.b_)
    dp_t, dp_f = float(np.abs(p_unfolded - r_unfolded).max()), float(np.abs(p_folded - r_folded).max())
    print(f"end to end: max|dp| vs float64 of the same parameters: transformed route {dp_t:.3g}, folded route {dp_f:.3g}; "
          f"gate {DP_GATE:.3g}; folded vs transformed route {float(np.abs(p_folded - p_unfolded).max()):.3g}; "
          f"val accuracy {float((p_folded.argmax(1) == e2e['yi'][e2e['cuts'][2]]).mean()):.3f}")
    check_labels(p_unfolded, r_unfolded, dp_bound=DP_GATE, max_flips=1, what="transformed route vs float64")
    check_labels(p_folded, r_folded, dp_bound=DP_GATE, max_flips=1, what="folded route vs float64")
    # the fold itself, in float64 and before its one rounding: the same function of the raw rows
    Wf = unfolded.weights[0].astype(np.float64) @ ft.components_
    bf = unfolded.biases[0].astype(np.float64) - Wf @ ft.mean_
    exact = ck.head_f64(e2e["val_raw"], [Wf] + unfolded.weights[1:], [bf] + unfolded.biases[1:], unfolded.a_, unfolded.b_)
    same = ck.head_f64(ft.transform_rows(e2e["val_raw"]), unfolded.weights, unfolded.biases, unfolded.a_, unfolded.b_)
    assert np.abs(exact - same).max() <= 1e-12 * same.max()


def test_transform_none_is_todays_path(e2e):
    from mermaid_classifier_amd import train_classifier
    plain = train_classifier(*e2e["sets"], 3, batch_size=100, clf=_clf())
    none = train_classifier(*e2e["sets"], 3, batch_size=100, clf=_clf(), transform=None)
    _same_model(plain[0], none[0])
    assert plain[1:] == none[1:]
    assert plain[0]._clf_state is not None and not hasattr(plain[0], "transform_")


def test_sweep_with_a_transform_equals_train_classifier_per_member(e2e):
    from mermaid_classifier_amd import SweepConfig, train_classifier, train_sweep
    configs = [SweepConfig(hidden_layer_sizes=(24, 12), learning_rate_init=3e-3, random_state=0, batch_size=50),
               SweepConfig(hidden_layer_sizes=(10,), learning_rate_init=1e-2, random_state=3, batch_size=64, label_smoothing=0.1)]
    spec = {"kind": "pca", "n_components": 9, "scatter": "within"}
    got = train_sweep(*e2e["sets"], configs, 3, batch_size=100, transform=spec)
    assert len(got) == 2
    for cfg, (cal, info, accs) in zip(configs, got):
        solo = train_classifier(*e2e["sets"], 3, batch_size=100, clf=cfg.classifier(e2e["sets"][1].device), transform=spec)
        _same_model(cal, solo[0])
        assert (info, accs) == solo[1:] and cal.n_features_in_ == E2E_DIM and cal.transform_.n_components == 9


def test_train_and_validate_scores_the_raw_val_split(e2e):
    from mermaid_classifier_amd import train_and_validate
    cal, val_results, msg = train_and_validate(*e2e["sets"], 3, batch_size=100, clf=_clf(), transform=e2e["ft"])
    _same_model(cal, e2e["folded"][0])
    want = float((e2e["folded"][0].predict(e2e["val_raw"]) == e2e["yi"][e2e["cuts"][2]]).mean())
    assert msg.acc == pytest.approx(want, abs=1e-12) and len(msg.ref_accs) == 3


def test_export_of_the_folded_model_takes_raw_features(e2e, tmp_path):
    from mermaid_classifier_amd import load_predictor
    from mermaid_classifier_amd.calibration import export_artifact
    folded = e2e["folded"][0]
    model_pt, manifest, gap = export_artifact(folded, tmp_path, e2e["val_raw"][:64])
    print("export parity of the folded model", gap)
    assert gap <= 1e-6 and manifest["input_dim"] == E2E_DIM
    assert json.loads((tmp_path / "model.json").read_text()) == manifest
    pred = load_predictor(model_pt, tmp_path / "model.json", device=0)
    assert np.abs(pred.predict_proba(e2e["val_raw"]) - folded.predict_proba(e2e["val_raw"])).max() <= 1e-6
