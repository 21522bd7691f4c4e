"""Logit calibration on the device (csrc/logit_scaling.hip, csrc/logit_newton.h, logit_scaling.py) against
tests/logit_scaling_checker.py: every element of the sums inside its 1x bound, the bit-level promises of include/mmc.h, the fits of
all three modes, the two cases without a finite minimiser, and the route through train_classifier / train_sweep / export.

Lines that start with ``logit_scaling:`` carry the figures tools/logit_scaling_cost.py records (worst error / bound ratios, the
parameter gap to the checker's optimum); none of them is gated beyond what is asserted here.
"""

import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import logit_scaling_checker as ck  # noqa: E402

pytestmark = pytest.mark.gpu

B = ck.BLOCK_ROWS
ALL_K = (2, 3, 15, 16, 17, 108, 128)
ALL_N = (1, 3, 4, 5, B - 1, B, B + 1, 3 * B + 7)
# every K with the ragged N, every N with K = 17
SHAPES = [(K, 3 * B + 7) for K in ALL_K] + [(17, N) for N in ALL_N if N != 3 * B + 7]
VARIANTS = ("identity", "random", "absent", "large")


def _store(z, y, cuts=()):
    from mermaid_classifier_amd.logit_scaling import _LogitCalibrator
    cal = _LogitCalibrator(z.shape[1])
    edges = [0, *cuts, len(y)]
    for lo, hi in zip(edges[:-1], edges[1:]):
        cal.add_logits(z[lo:hi], y[lo:hi])
    assert len(cal) == len(y)
    return cal


@functools.lru_cache(maxsize=None)
def _case(K, N, variant):
    """-> (z, y, a, c) of one stats case; seeded by the shape."""
    rng = np.random.default_rng(1000 * K + N)
    z = (rng.standard_normal((N, K)) * 3.0).astype(np.float32)
    y = rng.integers(0, K, N).astype(np.int32)
    a, c = np.ones(K), np.zeros(K)
    if variant == "random":
        a = rng.uniform(0.2, 3.0, K)
        a[rng.integers(0, K)] = -rng.uniform(0.2, 3.0)
        c = rng.standard_normal(K)
    elif variant == "absent":
        # two classes without a row (K = 2 can only lose one: every row carries a label)
        gone = np.array([0, K - 1]) if K > 2 else np.array([1])
        keep = np.setdiff1d(np.arange(K), gone)
        y = keep[rng.integers(0, len(keep), N)].astype(np.int32)
        a = rng.uniform(0.2, 3.0, K)
        c = rng.standard_normal(K)
    elif variant == "large":
        z = rng.uniform(-3000.0, 3000.0, (N, K)).astype(np.float32)
        z[0, 0] = 3000.0
        z[-1, K - 1] = -3000.0
        a = np.full(K, 3.0)
    return z, y, a, c


@functools.lru_cache(maxsize=None)
def _reference(K, N, variant):
    z, y, a, c = _case(K, N, variant)
    st = ck.stats(z, y, a, c)
    return st, ck.bounds(st, N, K)


def _ratios(got, want, bound):
    """max |got - want| / bound over the elements; an element with a zero bound must match exactly."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    bound = np.asarray(bound, np.float64)
    exact = bound == 0.0
    assert (err[exact] == 0.0).all()
    return float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K,N", SHAPES)
def test_stats_match_the_checker_per_element(K, N, variant):
    z, y, a, c = _case(K, N, variant)
    st, (b_nll, b_grad, b_hess) = _reference(K, N, variant)
    cal = _store(z, y)
    nll, grad, H, counts = cal.stats(a, c)
    cal.close()
    assert np.isfinite(nll) and np.isfinite(grad).all() and np.isfinite(H).all()
    assert np.array_equal(counts, st["counts"])
    r_nll = abs(nll - st["nll"]) / b_nll
    r_grad = _ratios(grad, st["grad"], b_grad)
    r_hess = _ratios(H, st["hess"], b_hess)
    print(f"logit_scaling: stats K={K} N={N} {variant}: error/bound nll {r_nll:.3g} grad {r_grad:.3g} hess {r_hess:.3g}")
    assert r_nll <= 1.0 and r_grad <= 1.0 and r_hess <= 1.0
    assert np.array_equal(H, H.T)
    if variant == "absent":
        assert counts[K - 1] == 0 and (K == 2 or counts[0] == 0)   # (a short set leaves more classes without a row)


@pytest.mark.parametrize("K", (17, 128))
def test_large_logits_give_the_checkers_probabilities(K):
    """One row per store: g_c + onehot(y) IS the row's p.  |a z| up to 9000: finite, and p inside gamma_p of the checker's."""
    z, y, a, c = _case(K, 3 * B + 7, "large")
    worst = 0.0
    for n in (0, 1, 2, 3 * B + 6):
        zr, yr = z[n:n + 1], y[n:n + 1]
        st = ck.stats(zr, yr, a, c, hess=False)
        cal = _store(zr, yr)
        nll, grad, _, _ = cal.stats(a, c, hess=False)
        cal.close()
        assert np.isfinite(nll) and np.isfinite(grad).all()
        onehot = np.eye(K)[yr[0]]
        p = grad[K:] + onehot
        gamma_p = 8.0 * st["U"] + 4.0 * ck.ULP_EXP + K + 2.0 * ck.ULP_DIV
        bound = 2.0 * (gamma_p + 1.0) * ck.EPS * (st["p"][0] + onehot)
        worst = max(worst, _ratios(p, st["p"][0], bound))
        assert abs(p.sum() - 1.0) <= 1e-12
    print(f"logit_scaling: large-logit p K={K}: error/bound {worst:.3g}")
    assert worst <= 1.0


def _bits(*arrays):
    return [np.asarray(x, np.float64).tobytes() for x in arrays]


def test_bits_do_not_depend_on_the_split_the_repeat_or_the_hessian():
    K, N = 17, 3 * B + 7
    z, y, a, c = _case(K, N, "random")
    one = _store(z, y)
    first = one.stats(a, c)
    again = one.stats(a, c)
    assert _bits(*first[:3]) == _bits(*again[:3])
    light = one.stats(a, c, hess=False)
    assert light[2] is None and _bits(*light[:2]) == _bits(*first[:2])
    one.close()
    three = _store(z, y, cuts=(1, 1537))
    split = three.stats(a, c)
    three.close()
    assert _bits(*split[:3]) == _bits(*first[:3])
    assert np.array_equal(first[2], first[2].T)
    big = _case(128, N, "random")
    cal = _store(big[0], big[1])
    H = cal.stats(big[2], big[3])[2]
    cal.close()
    assert np.array_equal(H, H.T) and np.abs(H).max() > 0


def test_growth_with_rows_stored_gives_the_bits_of_one_call():
    """600 rows, then 600 more: the second add crosses the 1024-row capacity, so the store is reallocated and the stored rows
    move.  The statistics and every fit come out bit for bit as from a store that took the 1200 rows in one call."""
    z, y = ck.fixture(1200, 3)
    grown, whole = _store(z, y, cuts=(600,)), _store(z, y)
    try:
        a, c = np.array([1.5, 0.7, 1.1]), np.array([0.2, -0.1, -0.1])
        got, want = grown.stats(a, c), whole.stats(a, c)
        assert _bits(*got[:3]) == _bits(*want[:3]) and np.array_equal(got[3], want[3])
        for kind in ck.KINDS:
            r_g, r_w = grown.fit(kind, tol=1e-9, max_trials=100), whole.fit(kind, tol=1e-9, max_trials=100)
            assert r_g.converged and r_g.n_rows == 1200 and r_g.trials == r_w.trials
            assert _bits(r_g.a, r_g.c, r_g.nll_before, r_g.nll_after) == _bits(r_w.a, r_w.c, r_w.nll_before, r_w.nll_after), kind
    finally:
        grown.close()
        whole.close()


@pytest.fixture(scope="module")
def tiny():
    """dim 16 -> (8,) -> K = 5, trained for a few passes on about 600 rows per split."""
    from mermaid_classifier_amd import FeatureSet
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    rng = np.random.default_rng(11)
    K, D = 5, 16
    centers = rng.normal(0.0, 1.0, size=(K, D))
    classes = np.array([f"c{i}" for i in range(K)])

    def split(n):
        yi = rng.integers(0, K, n)
        return (centers[yi] + rng.normal(0.0, 1.6, size=(n, D))).astype(np.float32), classes[yi]
    train, ref, val = split(640), split(600), split(610)
    clf = TorchMLPClassifier(hidden_layer_sizes=(8,), learning_rate_init=5e-3, random_state=0)
    for _ in range(6):
        clf.partial_fit(*train, classes=classes.tolist())
    sets = [FeatureSet(D, classes).append(*s) for s in (train, ref, val)]
    yield {"clf": clf, "classes": classes, "train": train, "ref": ref, "val": val, "sets": sets}
    for fs in sets:
        fs.close()


def _logits(clf, X):
    from mermaid_classifier_amd import _lib
    X = np.ascontiguousarray(X, np.float32)
    out = np.empty((len(X), len(clf.classes_)), np.float32)
    _lib.check(_lib.lib().mmc_trainer_logits(clf._h, X.ctypes.data, len(X), out.ctypes.data, None))
    return out


def test_add_set_stores_the_trainers_logits(tiny):
    from mermaid_classifier_amd.logit_scaling import _LogitCalibrator
    clf, (Xr, yr), fs = tiny["clf"], tiny["ref"], tiny["sets"][1]
    yi = clf._labels_to_indices(yr).astype(np.int32)
    rng = np.random.default_rng(2)
    a, c = rng.uniform(0.5, 2.0, 5), rng.standard_normal(5)
    from_set = _LogitCalibrator(5)
    from_set.add_set(clf, fs)
    from_rows = _LogitCalibrator(5)
    from_rows.add_features(clf, Xr[:77], yi[:77])
    from_rows.add_features(clf, Xr[77:], yi[77:])
    from_logits = _store(_logits(clf, Xr), yi)
    want = from_logits.stats(a, c)
    for cal in (from_set, from_rows):
        got = cal.stats(a, c)
        assert _bits(*got[:3]) == _bits(*want[:3]) and np.array_equal(got[3], want[3])
        cal.close()
    from_logits.close()


def test_rejections_launch_nothing():
    from mermaid_classifier_amd import _lib
    from mermaid_classifier_amd.logit_scaling import _LogitCalibrator
    with pytest.raises(ValueError, match=r"\[2, 128\]"):
        _LogitCalibrator(129)
    with pytest.raises(ValueError, match=r"\[2, 128\]"):
        _LogitCalibrator(1)
    cal = _LogitCalibrator(4)
    lib = _lib.lib()
    a, c = np.ones(4), np.zeros(4)
    with pytest.raises(ValueError, match="no rows"):
        cal.stats(a, c)
    with pytest.raises(ValueError, match="no rows"):
        cal.fit("vector")
    z = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError, match="outside"):
        cal.add_logits(z, np.array([0, 4, 1]))
    bad = z.copy()
    bad[1, 2] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        cal.add_logits(bad, np.array([0, 1, 2]))
    assert len(cal) == 0
    cal.add_logits(z, np.array([0, 1, 2]))
    with pytest.raises(ValueError, match="not finite"):
        cal.stats(np.array([1.0, np.nan, 1.0, 1.0]), c)
    out = np.zeros(4)
    d, i = C.c_double(0.0), C.c_int32(0)

    def fit(mode, l2, tol, trials):
        return lib.mmc_logitcal_fit(cal._h, mode, l2, tol, trials, out.ctypes.data, out.ctypes.data, None, C.byref(d), C.byref(d),
                                    C.byref(i), C.byref(i), None)
    assert fit(3, 0.0, 1e-9, 100) == _lib.MMC_ERR_ARG and fit(-1, 0.0, 1e-9, 100) == _lib.MMC_ERR_ARG
    assert fit(0, -1e-3, 1e-9, 100) == _lib.MMC_ERR_ARG and fit(0, 0.0, 0.0, 100) == _lib.MMC_ERR_ARG
    assert fit(0, 0.0, 1e-9, 0) == _lib.MMC_ERR_ARG and fit(0, 0.0, 1e-9, 1001) == _lib.MMC_ERR_ARG
    assert lib.mmc_logitcal_stats(cal._h, a.ctypes.data, c.ctypes.data, None, out.ctypes.data, None, None, None) == _lib.MMC_ERR_ARG
    assert fit(0, 0.0, 1e-9, 100) == _lib.MMC_OK
    cal.close()


@functools.lru_cache(maxsize=None)
def _fit_fixture(N, K):
    return ck.fixture(N, K)


@functools.lru_cache(maxsize=None)
def _optimum(N, K, kind, l2=0.0):
    z, y = _fit_fixture(N, K)
    return ck.fit(z, y, kind, l2=l2, tol=1e-12, max_trials=400)


def _check_fit(z, y, kind, res, l2=0.0, tol=1e-9):
    N = len(y)
    assert res.converged and res.trials <= 100 and res.nll_after <= res.nll_before
    assert np.isfinite(res.a).all() and np.isfinite(res.c).all()
    g, bound = ck.active_gradient(z, y, res.a, res.c, kind, l2=l2, frozen=res.frozen)
    assert (np.abs(g) / N <= tol + bound / N).all(), (np.abs(g).max() / N, bound.max() / N)
    return g


@pytest.mark.parametrize("kind", ck.KINDS)
@pytest.mark.parametrize("N,K", [(700, 5), (4000, 108)])
def test_fit_reaches_the_checkers_optimum(N, K, kind):
    z, y = _fit_fixture(N, K)
    cal = _store(z, y)
    res = cal.fit(kind, tol=1e-9, max_trials=100)
    cal.close()
    assert res.kind == kind and res.n_rows == N and not res.frozen.any()
    g = _check_fit(z, y, kind, res)
    best = _optimum(N, K, kind)
    F_got, F_best = ck.objective(z, y, res.a, res.c), ck.objective(z, y, best["a"], best["c"])
    b_F = ck.bounds(ck.stats(z, y, res.a, res.c, hess=False), N, K)[0]
    if kind == "temperature":
        gap = np.array([res.a[0] - best["a"][0]])
    else:
        idx = ck.active_index(K, kind, res.frozen)
        gap = (np.concatenate([res.a, res.c]) - np.concatenate([best["a"], best["c"]]))[idx]
    # convexity: F(theta) - F(theta*) <= g(theta) . (theta - theta*)
    assert F_got - F_best <= np.abs(g) @ np.abs(gap) + b_F
    assert abs(res.c.mean()) <= 1e-9
    assert abs(res.nll_after - F_got / N) <= b_F / N and abs(res.nll_before - ck.stats(z, y, np.ones(K), np.zeros(K), hess=False)["nll"] / N) <= b_F / N
    if kind == "temperature":
        assert res.temperature == 1.0 / res.a[0] and (res.a == res.a[0]).all() and (res.c == 0).all()
    if kind == "bias":
        assert (res.a == 1.0).all()
    print(f"logit_scaling: fit N={N} K={K} {kind}: {res.trials} trials (checker {best['trials']}), nll {res.nll_before:.6f} -> "
          f"{res.nll_after:.6f}, max|g|/N {np.abs(g).max() / N:.3g}, parameter gap to the checker's optimum {np.abs(gap).max():.3g}")


@pytest.mark.parametrize("kind", ("bias", "vector"))
def test_absent_classes_come_back_frozen_at_the_identity(kind):
    z, y = _fit_fixture(700, 5)
    keep = ~np.isin(y, (1, 3))
    z, y = z[keep], y[keep]
    cal = _store(z, y)
    res = cal.fit(kind)
    cal.close()
    assert res.frozen.tolist() == [False, True, False, True, False]
    assert (res.a[[1, 3]] == 1.0).all() and (res.c[[1, 3]] == 0.0).all()
    _check_fit(z, y, kind, res)
    assert np.abs(res.c[[0, 2, 4]]).max() > 0


def test_absent_classes_do_not_freeze_the_temperature():
    z, y = _fit_fixture(700, 5)
    keep = ~np.isin(y, (1, 3))
    cal = _store(z[keep], y[keep])
    res = cal.fit("temperature")
    cal.close()
    assert not res.frozen.any()
    _check_fit(z[keep], y[keep], "temperature", res)


@pytest.mark.parametrize("kind", ck.KINDS)
def test_separable_rows_end_finite(kind):
    z, y = ck.separable()
    cal = _store(z, y)
    res = cal.fit(kind, l2=0.0)
    assert np.isfinite(res.a).all() and np.isfinite(res.c).all() and np.isfinite([res.nll_before, res.nll_after]).all()
    assert res.nll_after <= res.nll_before and res.trials <= 100
    ridge = cal.fit(kind, l2=1e-3)
    cal.close()
    _check_fit(z, y, kind, ridge, l2=1e-3)
    print(f"logit_scaling: separable {kind}: l2=0 {res.trials} trials converged={res.converged} a {res.a.round(4).tolist()}; "
          f"l2=1e-3 {ridge.trials} trials a {ridge.a.round(4).tolist()}")


def _host_head(weights, biases, a, b, X):
    """CalibratedHead in float64 on the host: MLP, softmax, one Platt sigmoid per class, renormalise, clip the overshoot."""
    h = np.asarray(X, np.float64)
    for i, (w, v) in enumerate(zip(weights, biases)):
        h = h @ np.asarray(w, np.float64).T + np.asarray(v, np.float64)
        if i < len(weights) - 1:
            h = np.maximum(h, 0.0)
    e = np.exp(h - h.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    q = 1.0 / (1.0 + np.exp(a[None, :] * p + b[None, :]))
    d = q.sum(axis=1, keepdims=True)
    q = np.divide(q, d, out=np.full_like(q, 1.0 / q.shape[1]), where=d != 0)
    q[(1.0 < q) & (q <= 1.0 + 1e-5)] = 1.0
    return q


def test_train_classifier_with_vector_scaling_end_to_end(tiny, tmp_path):
    from mermaid_classifier_amd import load_predictor, train_classifier, validate
    from mermaid_classifier_amd.calibration import export_artifact
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    train, ref, val = tiny["sets"]

    def make():
        return TorchMLPClassifier(hidden_layer_sizes=(8,), learning_rate_init=5e-3, random_state=0)
    plain, info0, accs0 = train_classifier(train, ref, val, 4, batch_size=320, clf=make())
    model, info, accs = train_classifier(train, ref, val, 4, batch_size=320, clf=make(), logit_scaling="vector")
    assert info == {**info0} and accs == accs0          # training and early stopping read raw logits
    sc = model.logit_scaling_
    assert plain.logit_scaling_ is None and sc.kind == "vector" and sc.converged and sc.nll_after <= sc.nll_before
    assert sc.n_rows == len(ref)
    fw, fb = sc.fold(plain.weights, plain.biases)
    assert all(np.array_equal(x, w) for x, w in zip(fw, model.weights)) and all(np.array_equal(x, w) for x, w in zip(fb, model.biases))
    X = tiny["val"][0]
    proba = model.predict_proba(X)
    want = _host_head(model.weights, model.biases, model.a_, model.b_, X)
    print("logit_scaling: end to end max |p - float64 head|", np.abs(proba - want).max())
    assert np.abs(proba - want).max() <= 1e-6
    scored = validate(model, val)
    assert 0.0 <= scored.accuracy <= 1.0 and np.isfinite(scored.log_loss)
    pt, manifest, gap = export_artifact(model, tmp_path, X[:256])
    assert gap <= 1e-6
    pred = load_predictor(pt, tmp_path / "model.json", device=0)
    assert np.abs(pred.predict_proba(X) - proba).max() <= 1e-6
    # a fitted scaling passed in is used as it is
    again, _, _ = train_classifier(train, ref, val, 4, batch_size=320, clf=make(), logit_scaling=sc)
    assert again.logit_scaling_ is sc and all(np.array_equal(x, w) for x, w in zip(again.weights, model.weights))
    assert np.array_equal(again.a_, model.a_) and np.array_equal(again.b_, model.b_)


def test_train_sweep_scales_only_the_member_that_asks(tiny):
    from mermaid_classifier_amd import SweepConfig, train_sweep
    train, ref, val = tiny["sets"]
    base = dict(hidden_layer_sizes=(8,), learning_rate_init=5e-3)
    without = train_sweep(train, ref, val, [SweepConfig(**base), SweepConfig(**base, random_state=1)], 3, batch_size=320)
    mixed = train_sweep(train, ref, val, [SweepConfig(**base), SweepConfig(**base, random_state=1, logit_scaling="temperature")], 3,
                        batch_size=320)
    plain, scaled = mixed[0][0], mixed[1][0]
    assert plain.logit_scaling_ is None
    for x, w in zip(plain.weights + plain.biases + [plain.a_, plain.b_], without[0][0].weights + without[0][0].biases + [without[0][0].a_, without[0][0].b_]):
        assert x.tobytes() == w.tobytes()
    sc = scaled.logit_scaling_
    assert sc.kind == "temperature" and sc.nll_after <= sc.nll_before
    raw = without[1][0]
    assert np.array_equal(scaled.weights[0], raw.weights[0]) and np.array_equal(scaled.weights[-1], sc.fold(raw.weights, raw.biases)[0][-1])
    # the sweep-wide value reaches a member without one; the member's own wins
    both = train_sweep(train, ref, val, [SweepConfig(**base), SweepConfig(**base, random_state=1, logit_scaling="temperature")], 3,
                       batch_size=320, logit_scaling="bias")
    assert both[0][0].logit_scaling_.kind == "bias" and both[1][0].logit_scaling_.kind == "temperature"


def test_folded_classifier_logits_against_a_z_plus_c(tiny):
    from mermaid_classifier_amd import fit_logit_scaling
    clf, (X, y) = tiny["clf"], tiny["ref"]
    sc = fit_logit_scaling(clf, (X, y), kind="vector")
    assert sc.n_rows == len(y)
    from_set = fit_logit_scaling(clf, tiny["sets"][1], kind="vector")
    assert from_set.a.tobytes() == sc.a.tobytes() and from_set.c.tobytes() == sc.c.tobytes()
    folded = sc.fold_classifier(clf)
    assert folded is not clf and np.array_equal(folded.classes_, clf.classes_)
    got = _logits(folded, X).astype(np.float64)
    want = sc.apply(_logits(clf, X))
    (W1, W2), (b1, b2) = clf.parameters()
    h = np.maximum(X.astype(np.float64) @ W1.astype(np.float64).T + b1, 0.0)
    A = np.abs(h) @ np.abs(sc.a[:, None] * W2).T + np.abs(sc.a * b2) + np.abs(sc.c)
    ratio = np.abs(got - want) / (ck.FOLD_GAMMA(W2.shape[1]) * 2.0 ** -24 * A)
    print(f"logit_scaling: folded logits error/bound {ratio.max():.3g}")
    assert ratio.max() <= 1.0
    adam = folded._adam_state()
    assert all(not m.any() for m in adam["exp_avg"][0]) and all(not m.any() for m in adam["exp_avg_sq"][1])
