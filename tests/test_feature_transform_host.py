"""Feature transforms without a device: the derived bounds of tests/feature_transform_checker.py hold for an honest emulation of
csrc/features.hip's scatter and transform arithmetic and catch six wrong kernels where their bug is; FeatureTransform's host
algebra (fit from statistics, fold, argument errors, pickling)."""

import pickle

import numpy as np
import pytest

import feature_transform_checker as ck
from mermaid_classifier_amd.feature_transform import FeatureTransform, eigen_basis

K = 5


@pytest.fixture(scope="module")
def data():
    X, yi = ck.reef_like(4000, 200, K, seed=11)
    counts, mean, m2, _, _ = ck.moments(X, yi, K)
    return X, yi, counts, mean.astype(np.float64), m2.astype(np.float64)


@pytest.fixture(scope="module")
def small():
    """n = 4203 rows (17 chunks, the last ragged with a ragged last 16-row stage, in 16 ranges: the last range holds two chunks),
    dim = 136 (two tiles: an off-diagonal pair)."""
    X, yi = ck.reef_like(4203, 136, K, seed=5)
    assert ck.scatter_splits(4203, 136) == 16
    counts, mean, _, _, _ = ck.moments(X, yi, K)
    return X, yi, mean.astype(np.float64)


def test_features_look_like_pooled_activations(data):
    X, _, _, mean, m2 = data
    sd = np.sqrt(m2[K] / len(X))
    assert X.min() >= 0 and np.median(mean[K] / sd) > 3          # column means of several standard deviations
    corr = np.corrcoef(X[:, :40].T)
    assert np.abs(corr[np.triu_indices(40, 1)]).mean() > 0.1     # and strongly correlated


def test_scatter_emulation_within_bound(data):
    X, yi, _, mean, _ = data
    worst = {}
    for name, centres, labels in (("total", mean[K].astype(np.float32), None), ("within", mean[:K].astype(np.float32), yi)):
        ref, bound = ck.scatter(ck.centred(X, centres, labels))
        got = ck.emulate_scatter(X, centres, labels)
        worst[name] = float((np.abs(got - ref) / bound).max())
        assert np.array_equal(got, got.T)
    print("scatter emulation, worst |err| / bound:", worst)
    assert max(worst.values()) <= 1.0


def test_transform_emulation_within_bound(data):
    X, _, _, mean, _ = data
    rng = np.random.default_rng(3)
    T = rng.normal(0, 0.2, (37, 200)).astype(np.float32)
    Xc = ck.centred(X[:300], mean[K].astype(np.float32))
    ref, bound = ck.transform(Xc, T)
    ratio = float((np.abs(ck.emulate_transform(Xc, T) - ref) / bound).max())
    print("transform emulation, worst |err| / bound:", ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("bug", ["drop_last_chunk", "centre_after_pad", "neighbour_centre", "no_mirror", "split_twice", "no_clear"])
def test_wrong_scatter_kernels_exceed_the_bound(small, bug):
    X, yi, mean = small
    by_label = bug == "neighbour_centre"
    centres = (mean[:K] if by_label else mean[K]).astype(np.float32)
    labels = yi if by_label else None
    ref, bound = ck.scatter(ck.centred(X, centres, labels))
    honest = np.abs(ck.emulate_scatter(X, centres, labels) - ref) / bound
    wrong = np.abs(ck.emulate_scatter(X, centres, labels, bug=bug) - ref) / bound
    print(bug, "honest worst", float(honest.max()), "wrong worst", float(wrong.max()), "elements over", int((wrong > 1).sum()))
    assert honest.max() <= 1.0
    assert wrong.max() > 1.0
    if bug == "no_mirror":                                        # where the bug is: the lower off-diagonal block, nowhere else
        over = wrong > 1.0
        assert over[128:, :128].all() and not over[:128].any() and not over[128:, 128:].any()


def _whiten_inputs(data, scatter):
    X, yi, counts, mean, m2 = data
    centres = mean[K] if scatter == "total" else mean[:K]
    S, _ = ck.scatter(ck.centred(X, centres.astype(np.float32), None if scatter == "total" else yi))
    return counts, mean, m2, S


def test_whiten_makes_the_scatter_the_identity(data):
    counts, mean, m2, S = _whiten_inputs(data, "total")
    ft = FeatureTransform.from_statistics("whiten", counts, mean, m2, S, eps=1e-12)
    n = counts.sum()
    W = ft.components_ @ (S / n) @ ft.components_.T
    print("whiten: max |T S T^T / n - I|", np.abs(W - np.eye(200)).max())
    assert np.abs(W - np.eye(200)).max() <= 1e-9
    assert ft.kind == "whiten" and ft.dim == 200 and ft.n_components == 200 and ft.n_rows_ == n
    assert np.array_equal(ft.mean_, mean[K]) and np.array_equal(ft.class_means_, mean[:K]) and np.array_equal(ft.counts_, counts)


def test_sign_order_and_truncation(data):
    counts, mean, m2, S = _whiten_inputs(data, "total")
    full = FeatureTransform.from_statistics("pca", counts, mean, m2, S)
    lam = full.explained_variance_
    assert np.all(np.diff(lam) <= 0)                                                   # descending
    V = full.components_
    lead = np.abs(V).argmax(axis=1)
    assert np.all(V[np.arange(200), lead] > 0)                                         # the largest-magnitude component is positive
    assert np.abs(V @ V.T - np.eye(200)).max() <= 1e-12
    assert np.abs(V @ (S / counts.sum()) @ V.T - np.diag(lam)).max() <= 1e-9 * lam[0]
    cut = FeatureTransform.from_statistics("pca", counts, mean, m2, S, n_components=17)
    assert cut.n_components == 17 and np.array_equal(cut.components_, V[:17]) and np.array_equal(cut.explained_variance_, lam[:17])
    wh = FeatureTransform.from_statistics("whiten", counts, mean, m2, S, n_components=17, eps=1e-3)
    assert np.allclose(wh.components_, V[:17] / np.sqrt(lam[:17] + 1e-3 * lam.mean())[:, None], rtol=1e-14, atol=0)
    # ties go to the lowest index, and a flipped input comes back the same
    lam2, Vt = eigen_basis(np.diag([2.0, 2.0, 1.0]))
    assert np.array_equal(lam2, [2.0, 2.0, 1.0]) and np.all(Vt[np.arange(3), np.abs(Vt).argmax(axis=1)] > 0)
    tie = np.array([[0.5, -0.5], [-0.5, 0.5]])                                          # eigenvectors (1, -1)/sqrt2 and (1, 1)/sqrt2
    _, Vt = eigen_basis(tie)
    assert Vt[0, 0] > 0 and Vt[0, 1] < 0 and np.all(Vt[1] > 0)


def test_total_is_within_plus_between(data):
    X, yi, counts, mean, m2 = data
    _, _, _, S_total = _whiten_inputs(data, "total")
    _, _, _, S_within = _whiten_inputs(data, "within")
    # the operands are fl32(x - c): each carries a relative rounding of at most 2^-24, so a product of two is off by at most 2^-23 of
    # |xc_j||xc_k| and an element of either scatter by at most 2^-23 sqrt(S_jj S_kk) (Cauchy-Schwarz); two scatters: 2^-22
    diff = mean[:K] - mean[K]
    between = (counts[:, None, None] * diff[:, :, None] * diff[:, None, :]).sum(axis=0)
    scale = np.sqrt(np.outer(np.diag(S_total), np.diag(S_total)))
    print("total - within - between, worst / scale:", (np.abs(S_total - S_within - between) / scale).max())
    assert (np.abs(S_total - S_within - between) / scale).max() <= 2.0 ** -22
    assert np.abs(m2[K] - m2[:K].sum(axis=0) - np.diag(between)).max() <= 1e-9 * m2[K].max()
    within = FeatureTransform.from_statistics("whiten", counts, mean, m2, S_within, scatter="within")
    assert within.scatter == "within" and np.array_equal(within.mean_, mean[K])        # still centred on the global mean


def test_standardize(data):
    X, yi, counts, mean, m2 = data
    ft = FeatureTransform.from_statistics("standardize", counts, mean, m2, eps=1e-3)
    var = m2[K] / len(X)
    want = (X.astype(np.float64) - mean[K]) / np.sqrt(var + 1e-3 * var.mean())
    assert np.abs(ft.transform_rows(X) - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(ft.explained_variance_, var) and ft.n_components == 200
    pooled = FeatureTransform.from_statistics("standardize", counts, mean, m2, scatter="within")
    assert np.array_equal(pooled.explained_variance_, m2[:K].sum(axis=0) / len(X))


def test_fold_is_the_same_function_of_raw_features(data):
    X, yi, counts, mean, m2 = data
    _, _, _, S = _whiten_inputs(data, "total")
    ft = FeatureTransform.from_statistics("whiten", counts, mean, m2, S, n_components=24)
    rng = np.random.default_rng(9)
    dims = [24, 12, 9, K]
    weights = [rng.normal(0, 0.4, (o, i)) for i, o in zip(dims, dims[1:])]
    biases = [rng.normal(0, 0.2, o) for o in dims[1:]]
    a, b = rng.uniform(-9, -3, K), rng.uniform(0.5, 2.0, K)
    # float64 fold (the definition, before the one rounding to fp32)
    Wf = weights[0] @ ft.components_
    bf = biases[0] - Wf @ ft.mean_
    raw = X[:500].astype(np.float64)
    p_folded = ck.head_f64(raw, [Wf] + weights[1:], [bf] + biases[1:], a, b)
    p_unfolded = ck.head_f64(ft.transform_rows(raw), weights, biases, a, b)
    rel = np.abs(p_folded - p_unfolded).max() / p_unfolded.max()
    print("fold: max relative |dp|", rel)
    assert rel <= 1e-12
    w32, b32 = ft.fold([w.astype(np.float32) for w in weights], [v.astype(np.float32) for v in biases])
    assert w32[0].dtype == np.float32 and w32[0].shape == (12, 200) and b32[0].shape == (12,)
    W1 = weights[0].astype(np.float32).astype(np.float64) @ ft.components_
    assert np.array_equal(w32[0], W1.astype(np.float32))
    assert np.array_equal(b32[0], (biases[0].astype(np.float32).astype(np.float64) - W1 @ ft.mean_).astype(np.float32))
    for i in (1, 2):
        assert np.array_equal(w32[i], weights[i].astype(np.float32)) and np.array_equal(b32[i], biases[i].astype(np.float32))
    with pytest.raises(ValueError, match="first layer takes"):
        ft.fold([np.zeros((3, 25), np.float32)], [np.zeros(3, np.float32)])


def test_calibrated_mlp_folded(data):
    from mermaid_classifier_amd.calibration import CalibratedMLP
    X, yi, counts, mean, m2 = data
    ft = FeatureTransform.from_statistics("standardize", counts, mean, m2)
    rng = np.random.default_rng(2)
    weights = [rng.normal(0, 0.1, (7, 200)).astype(np.float32), rng.normal(0, 0.1, (K, 7)).astype(np.float32)]
    biases = [np.zeros(7, np.float32), np.zeros(K, np.float32)]
    cm = CalibratedMLP(weights, biases, np.arange(K), -np.ones(K), np.zeros(K), np.ones(K), clf_state={"x": 1})
    folded = cm.folded(ft)
    assert folded.n_features_in_ == 200 and folded.transform_ is ft and folded._clf_state is None
    assert np.array_equal(folded.a_, cm.a_) and np.array_equal(folded.b_, cm.b_) and np.array_equal(folded.classes_, cm.classes_)
    with pytest.raises(RuntimeError, match="to_sklearn needs the classifier"):
        folded.to_sklearn()
    cut = FeatureTransform(ft.kind, ft.mean_, ft.components_[:50], ft.explained_variance_[:50])
    with pytest.raises(ValueError, match="writes 50 features"):
        cm.folded(cut)


def test_argument_errors_need_no_device(data):
    from mermaid_classifier_amd import FeatureSet, train_classifier, train_sweep, SweepConfig
    X, yi, counts, mean, m2 = data
    fs = FeatureSet(8, np.arange(K))                              # no handle yet, and none is made below
    for kwargs, match in ((dict(kind="zca"), "kind must be one of"),
                          (dict(kind="pca", scatter="between"), "scatter must be one of"),
                          (dict(kind="whiten", eps=0.0), "eps must be a positive"),
                          (dict(kind="whiten", eps=-1e-3), "eps must be a positive"),
                          (dict(kind="whiten", eps=float("nan")), "eps must be a positive"),
                          (dict(kind="pca", n_components=0), r"n_components must be an integer in \[1, 8\]"),
                          (dict(kind="pca", n_components=9), r"n_components must be an integer in \[1, 8\]"),
                          (dict(kind="pca", n_components=2.5), r"n_components must be an integer in \[1, 8\]"),
                          (dict(kind="standardize", n_components=3), "keeps every feature"),
                          (dict(kind="pca"), "at least 2 rows"),
                          (dict(kind="pca", rows=(0, 5)), "outside the set's 0 rows")):
        with pytest.raises(ValueError, match=match):
            FeatureTransform.fit(fs, **kwargs)
        assert fs._h is None
    with pytest.raises(ValueError, match="must be a FeatureSet"):
        FeatureTransform.fit(X, "pca")
    with pytest.raises(ValueError, match="at least 2 rows"):
        one = np.zeros(K, np.int64)
        one[0] = 1
        FeatureTransform.from_statistics("standardize", one, mean, m2)
    ft = FeatureTransform.from_statistics("standardize", counts, mean, m2)
    with pytest.raises(ValueError, match="the transform takes 200"):
        ft.apply(fs)
    assert fs._h is None
    # the training entries check the splits first, as without a transform
    with pytest.raises(ValueError, match="empty"):
        train_classifier(fs, fs, fs, 1, batch_size=4, transform={"kind": "whiten"})
    with pytest.raises(ValueError, match="empty"):
        train_sweep(fs, fs, fs, [SweepConfig()], 1, batch_size=4, transform=ft)


def test_pickle_round_trip(data):
    X, yi, counts, mean, m2 = data
    _, _, _, S = _whiten_inputs(data, "within")
    ft = FeatureTransform.from_statistics("whiten", counts, mean, m2, S, n_components=31, eps=2e-3, scatter="within")
    back = pickle.loads(pickle.dumps(ft))
    for name in ("mean_", "components_", "explained_variance_", "counts_", "class_means_"):
        assert np.array_equal(getattr(back, name), getattr(ft, name))
    assert (back.kind, back.scatter, back.eps, back.n_rows_, back.dim, back.n_components) == ("whiten", "within", 2e-3, 4000, 200, 31)
    assert np.array_equal(back.transform_rows(X[:9]), ft.transform_rows(X[:9]))
    c32, t32 = back.device_operands()
    assert c32.dtype == np.float32 and t32.dtype == np.float32 and t32.shape == (31, 200) and t32.flags.c_contiguous
