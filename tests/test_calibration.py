"""Evaluation, Platt calibration and export of the trained MLP head (mermaid_classifier_amd/calibration.py, csrc/calib.hip).

CPU tests: a float64 restatement of the device's Newton scheme reproduces sklearn's Platt fits (tests/golden/
calibration_fixture.npz, made by make_calibration_golden.py with sklearn 1.7.2); the module's TorchScript head reproduces the
committed reference graph; argument errors that need no device.  GPU tests (-m gpu): the device fit, evaluate, calibrate and
export against the fixture and the host path.  No test needs sklearn except where it is imported live (importorskip)."""

import ctypes as C
import json

import numpy as np
import pytest

from conftest import GOLDEN, check_labels

FIX = GOLDEN / "calibration_fixture.npz"
SETS = ("main", "deg", "allpos")


# ---- float64 restatements ---------------------------------------------------------------------------------------------------
def _targets(pos):
    n1 = float(pos.sum())
    n0 = len(pos) - n1
    return np.where(pos, (n1 + 1.0) / (n1 + 2.0), 1.0 / (n0 + 2.0)), n0, n1


def platt_objective(F, pos, a, b):
    """_sigmoid_calibration's objective at (a, b) on the caller's scale of F: sum log1p(e^r) - T r, r = -(a F + b)."""
    T, _, _ = _targets(pos)
    r = -(a * np.asarray(F, np.float64) + b)
    return float(np.sum(np.logaddexp(0.0, r) - T * r))


def platt_newton(F, pos, max_iter=100):
    """The device's scheme (csrc/calib.hip) in float64 numpy: sklearn's objective and start point, damped Newton with a 1e-12
    ridge, Armijo backtracking, stop on |gradient| <= 1e-12 N or a negligible step.  -> (a, b, iterations)."""
    F = np.asarray(F, np.float64)
    N = len(F)
    T, n0, n1 = _targets(pos)
    mx = float(np.abs(F).max())
    scale = mx if mx >= 30.0 else 1.0
    Fs = F / scale
    max_f = mx / scale

    def ev(A, B):
        r = -(A * Fs + B)
        e = np.exp(-np.abs(r))
        inv = 1.0 / (1.0 + e)
        L = np.sum(np.maximum(r, 0.0) + np.log1p(e) - T * r)
        s = np.where(r >= 0.0, inv, e * inv)
        w = e * inv * inv
        d = s - T
        return L, (-np.sum(d * Fs), -np.sum(d)), (np.sum(w * Fs * Fs), np.sum(w * Fs), np.sum(w))

    A, B = 0.0, np.log((n0 + 1.0) / (n1 + 1.0))
    f, g, H = ev(A, B)
    it = 0
    while True:
        a11, a22, a12 = H[0] + 1e-12, H[2] + 1e-12, H[1]
        det = a11 * a22 - a12 * a12
        if det > 0:
            dA, dB = -(a22 * g[0] - a12 * g[1]) / det, -(a11 * g[1] - a12 * g[0]) / det
        else:
            dA, dB = 0.0, -g[1] / a22
        if max(abs(g[0]), abs(g[1])) <= 1e-12 * N or abs(dA) * max_f + abs(dB) <= 1e-13 * (1.0 + abs(B)) or it >= max_iter:
            break
        t = 1.0
        while True:
            it += 1
            Lt, gt, Ht = ev(A + t * dA, B + t * dB)
            if Lt <= f + 1e-4 * t * (g[0] * dA + g[1] * dB) + 64.0 * np.finfo(float).eps * abs(f):
                A, B, f, g, H = A + t * dA, B + t * dB, Lt, gt, Ht
                break
            t *= 0.5
            if t < 1e-6 or it >= max_iter:
                return A / scale, B, it
    return A / scale, B, it


def calibrated_proba(S, a, b):
    """_CalibratedClassifier.predict_proba from per-class a / b (multiclass)."""
    z = -(np.asarray(a)[None, :] * np.asarray(S, np.float64) + np.asarray(b)[None, :])
    c = 1.0 / (1.0 + np.exp(-z))
    d = c.sum(1, keepdims=True)
    p = np.divide(c, d, out=np.full_like(c, 1.0 / c.shape[1]), where=d != 0)
    p[(1.0 < p) & (p <= 1.0 + 1e-5)] = 1.0
    return p


def host_log_loss_terms(P, y):
    eps = np.finfo(np.float64).eps
    return -np.log(np.clip(P[np.arange(len(y)), y], eps, 1 - eps))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIX))


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_newton_restatement_reproduces_sklearn(fx, name):
    S, y, a_sk, b_sk = fx[f"{name}_S"], fx[f"{name}_y"], fx[f"{name}_a"], fx[f"{name}_b"]
    for k in range(S.shape[1]):
        pos = y == k
        a, b, it = platt_newton(S[:, k], pos)
        assert it <= 50
        sig = 1.0 / (1.0 + np.exp(a * S[:, k] + b))
        sig_sk = 1.0 / (1.0 + np.exp(a_sk[k] * S[:, k] + b_sk[k]))
        assert np.abs(sig - sig_sk).max() <= 1e-8, (name, k)
        f, f_sk = platt_objective(S[:, k], pos, a, b), platt_objective(S[:, k], pos, a_sk[k], b_sk[k])
        assert f <= f_sk + 1e-12 * abs(f_sk), (name, k, f, f_sk)


def test_log_loss_restatement_matches_sklearn(fx):
    P, y = fx["ll_P"], fx["ll_y"]
    assert float(np.mean(host_log_loss_terms(P, y))) == pytest.approx(float(fx["ll_log_loss"]), rel=1e-12)
    assert float(np.mean(P.argmax(1) == y)) == float(fx["ll_accuracy"])


def test_torchscript_head_matches_reference_graph():
    import torch
    from mermaid_classifier_amd.calibration import build_head_module
    from mermaid_classifier_amd.inference import params_from_torchscript
    io = np.load(GOLDEN / "head_fixture_io.npz")
    n = int(io["n_layers"])
    W = [io[f"W{i}"] for i in range(n)]
    B = [io[f"b{i}"] for i in range(n)]
    head = build_head_module(W, B, io["a"], io["b"])
    ref = torch.jit.load(str(GOLDEN / "head_fixture" / "model.pt"), map_location="cpu").eval()
    x = torch.from_numpy(io["X"])
    with torch.no_grad():
        got, want = head(x).numpy(), ref(x).numpy()
    assert np.abs(got - io["proba_head_f32"]).max() <= 1e-7
    assert np.abs(got - want).max() <= 1e-7
    p = params_from_torchscript(head)
    assert all(np.array_equal(u, v) for u, v in zip(p.weights, W)) and all(np.array_equal(u, v) for u, v in zip(p.biases, B))
    assert np.array_equal(p.a, io["a"]) and np.array_equal(p.b, io["b"])


def test_c_abi_argument_errors_without_device():
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p(1234)
    assert lib.mmc_calibrator_create(2, 0, C.byref(h)) == _lib.MMC_ERR_ARG and h.value is None
    assert b"multiclass" in lib.mmc_last_error()
    assert lib.mmc_calibrator_create(5, 0, None) == _lib.MMC_ERR_ARG
    a = np.zeros(4)
    assert lib.mmc_calibrator_fit(None, a.ctypes.data, a.ctypes.data, None, None) == _lib.MMC_ERR_ARG
    assert lib.mmc_calibrator_add_scores(None, a.ctypes.data, a.ctypes.data, 1, None) == _lib.MMC_ERR_ARG
    assert lib.mmc_calibrator_add_features(None, None, None, None, 1, None) == _lib.MMC_ERR_ARG
    nc, ll = C.c_int64(0), C.c_double(0.0)
    assert lib.mmc_trainer_evaluate(None, None, None, 1, C.byref(nc), C.byref(ll), None) == _lib.MMC_ERR_ARG
    q = C.c_int64(0)
    assert lib.mmc_trainer_evaluate_q32(None, None, None, 1, C.byref(nc), C.byref(q), None) == _lib.MMC_ERR_ARG
    lib.mmc_calibrator_destroy(None)
    assert all(hasattr(lib, s) for s in _lib.SYMBOLS)


def test_python_argument_errors_without_device():
    from mermaid_classifier_amd import calibration
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    with pytest.raises(RuntimeError, match="not fitted"):
        calibration.calibrate(TorchMLPClassifier(), (np.zeros((2, 4), np.float32), np.zeros(2)))
    with pytest.raises(RuntimeError, match="not fitted"):
        calibration.evaluate(TorchMLPClassifier(), (np.zeros((2, 4), np.float32), np.zeros(2)))

    class Binary(TorchMLPClassifier):
        def _fitted(self):
            return True
    clf = Binary()
    clf.classes_ = np.array(["a", "b"])
    with pytest.raises(ValueError, match="K >= 3"):
        calibration.calibrate(clf, (np.zeros((2, 4), np.float32), np.array(["a", "b"])))
    with pytest.raises(ValueError, match="K >= 3"):
        calibration.CalibratedMLP([np.zeros((2, 4), np.float32)], [np.zeros(2, np.float32)], ["a", "b"], [0, 0], [0, 0])


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _fit_scores(S, y, splits=None):
    from mermaid_classifier_amd.calibration import _Calibrator
    cal = _Calibrator(S.shape[1], 0)
    bounds = [0] + list(splits or []) + [len(y)]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        cal.add_scores(S[lo:hi], y[lo:hi])
    out = cal.fit()
    cal.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_device_fit_from_scores(fx, name):
    S, y, a_sk, b_sk = fx[f"{name}_S"], fx[f"{name}_y"], fx[f"{name}_a"], fx[f"{name}_b"]
    a, b, it = _fit_scores(S, y)
    print(name, "iterations", it.tolist())
    assert it.max() <= 50
    d = np.abs(calibrated_proba(S, a, b) - calibrated_proba(S, a_sk, b_sk)).max()
    print(name, "max|dp| vs sklearn", d)
    assert d <= 1e-6
    for k in range(S.shape[1]):
        f, f_sk = platt_objective(S[:, k], y == k, a[k], b[k]), platt_objective(S[:, k], y == k, a_sk[k], b_sk[k])
        assert f <= f_sk + 1e-9 * abs(f_sk), (name, k, f, f_sk)
    a2, b2, it2 = _fit_scores(S, y)
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(it, it2)
    a3, b3, _ = _fit_scores(S, y, splits=[len(y) // 7, len(y) // 7 + len(y) // 3 + 1])
    assert np.array_equal(a, a3) and np.array_equal(b, b3)


@pytest.mark.gpu
def test_growth_with_rows_stored_gives_the_bits_of_one_call():
    """600 rows of K = 3 scores, then 600 more: the second add crosses the 1024-row capacity, so the class-major store is
    reallocated and its columns move.  The fit comes out bit for bit as from a calibrator that took the 1200 rows in one call."""
    rng = np.random.default_rng(1200)
    y = rng.integers(0, 3, 1200)
    S = rng.dirichlet(np.ones(3), 1200) * 0.6 + 0.4 * np.eye(3)[y] * rng.uniform(0.0, 1.0, (1200, 1))
    a1, b1, it1 = _fit_scores(S, y, splits=[600])
    a2, b2, it2 = _fit_scores(S, y)
    assert np.isfinite(a1).all() and np.isfinite(b1).all() and it1.max() <= 50
    assert a1.tobytes() == a2.tobytes() and b1.tobytes() == b2.tobytes() and np.array_equal(it1, it2)


@pytest.mark.gpu
def test_device_argument_errors():
    from mermaid_classifier_amd.calibration import _Calibrator
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    cal = _Calibrator(4, 0)
    with pytest.raises(ValueError, match="no rows"):
        cal.fit()
    with pytest.raises(ValueError, match="outside"):
        cal.add_scores(np.full((3, 4), 0.25), np.array([0, 4, 1]))
    with pytest.raises(ValueError, match="not finite"):
        cal.add_scores(np.array([[0.25, 0.25, np.nan, 0.25]]), np.array([0]))
    with pytest.raises(ValueError, match="fp32 range"):
        cal.add_scores(np.array([[0.25, 0.25, 1e39, 0.25]]), np.array([0]))
    clf = TorchMLPClassifier(hidden_layer_sizes=(8,), random_state=0)
    clf.partial_fit(np.random.default_rng(0).normal(size=(12, 4)).astype(np.float32), np.arange(12) % 3)
    X = np.zeros((2, 4), np.float32)
    with pytest.raises(ValueError, match="classes"):
        cal.add_features(clf, X, np.zeros(2, np.int32))
    cal.close()


def _seeded_problem(rng, n, d, k, centers):
    y = rng.integers(0, k, size=n)
    X = centers[y] + rng.normal(0.0, 1.0, size=(n, d)).astype(np.float32)
    return X.astype(np.float32), y


@pytest.fixture(scope="module")
def trained():
    """TorchMLPClassifier at the production shape (1280 -> 500 -> 300 -> 100 -> 108), two seeded partial_fit passes."""
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    rng = np.random.default_rng(7)
    K, D = 108, 1280
    centers = rng.normal(0.0, 0.08, size=(K, D)).astype(np.float32)
    classes = np.array([f"ba{i}::gf{i % 7}" for i in range(K)])
    Xtr, ytr = _seeded_problem(rng, 6000, D, K, centers)
    clf = TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), random_state=0)
    for _ in range(2):
        clf.partial_fit(Xtr, classes[ytr], classes=classes.tolist())
    Xref, yref = _seeded_problem(rng, 20000, D, K, centers)
    return clf, classes, Xref, classes[yref]


def _host_platt(P, y_idx):
    try:
        from sklearn.calibration import _SigmoidCalibration
    except ImportError:
        fits = [platt_newton(P[:, k], y_idx == k)[:2] for k in range(P.shape[1])]
        return np.array([f[0] for f in fits]), np.array([f[1] for f in fits])
    a, b = np.empty(P.shape[1]), np.empty(P.shape[1])
    for k in range(P.shape[1]):
        cal = _SigmoidCalibration().fit(P[:, k], (y_idx == k).astype(np.int64))
        a[k], b[k] = cal.a_, cal.b_
    return a, b


@pytest.mark.gpu
def test_calibrate_from_features_matches_host_path(trained):
    from mermaid_classifier_amd.calibration import calibrate
    clf, classes, Xref, yref = trained
    batches = [(Xref[i:i + 3000], yref[i:i + 3000]) for i in range(0, len(yref), 3000)]
    cm = calibrate(clf, iter(batches))
    print("iterations", np.bincount(cm.iterations_))
    assert cm.iterations_.max() <= 50
    P = clf.predict_proba(Xref)
    y_idx = clf._labels_to_indices(yref)
    a_h, b_h = _host_platt(P, y_idx)
    want = calibrated_proba(P, a_h, b_h)
    got = cm.predict_proba(Xref)
    check_labels(got, want, dp_bound=1e-6, what="calibrate vs host Platt")
    assert np.array_equal(cm.predict(Xref[:64]), cm.classes_[got[:64].argmax(1)])


@pytest.mark.gpu
def test_evaluate_matches_host(trained):
    from mermaid_classifier_amd.calibration import evaluate
    clf, classes, Xref, yref = trained
    X, y = Xref[:9000], yref[:9000]
    acc, ll = evaluate(clf, (X, y))
    assert acc == float(np.mean(clf.predict(X) == y))
    host_ll = float(np.mean(host_log_loss_terms(clf.predict_proba(X), clf._labels_to_indices(y))))
    print("evaluate", acc, ll, "host log_loss", host_ll)
    assert abs(ll - host_ll) <= 1e-7 * abs(host_ll)
    acc3, ll3 = evaluate(clf, [(X[:1234], y[:1234]), (X[1234:5000], y[1234:5000]), (X[5000:], y[5000:])])
    assert acc3 == acc and ll3 == ll
    # the C ABI's sums: the fixed-point integers add up exactly however the rows are split, and the double form is that
    # integer times 2^-32
    from mermaid_classifier_amd import _lib
    yi = clf._labels_to_indices(y).astype(np.int32)

    def sums(lo, hi):
        nc, q, nc2, s = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        Xc = np.ascontiguousarray(X[lo:hi])
        yc = np.ascontiguousarray(yi[lo:hi])
        _lib.check(_lib.lib().mmc_trainer_evaluate_q32(clf._h, Xc.ctypes.data, yc.ctypes.data, hi - lo, C.byref(nc), C.byref(q), None))
        _lib.check(_lib.lib().mmc_trainer_evaluate(clf._h, Xc.ctypes.data, yc.ctypes.data, hi - lo, C.byref(nc2), C.byref(s), None))
        assert nc2.value == nc.value and s.value == q.value / 2**32
        return nc.value, q.value
    one = sums(0, 9000)
    parts = [sums(0, 17), sums(17, 6000), sums(6000, 9000)]
    assert one == (sum(p[0] for p in parts), sum(p[1] for p in parts))
    assert ll == one[1] / (9000 << 32)
    with pytest.raises(ValueError, match="not in classes_"):
        evaluate(clf, (X[:2], np.array(["nope", "nope"])))


@pytest.mark.gpu
def test_export_round_trip(trained, tmp_path):
    from mermaid_classifier_amd import SCHEMA_VERSION, TASK_NAME, load_predictor
    from mermaid_classifier_amd.calibration import ParityError, calibrate, export_artifact
    clf, classes, Xref, yref = trained
    cm = calibrate(clf, (Xref[:8000], yref[:8000]))
    model_pt, manifest, diff = export_artifact(cm, tmp_path, Xref[:512])
    print("export parity", diff)
    assert diff <= 1e-6
    on_disk = json.loads((tmp_path / "model.json").read_text())
    assert on_disk == manifest
    assert manifest["schema_version"] == SCHEMA_VERSION and manifest["task"] == TASK_NAME
    assert manifest["classes"] == clf.classes_.tolist() and manifest["input_dim"] == 1280
    assert manifest["config"] == {"patch_size": 224}
    assert set(manifest["trained_with"]) == {"torch", "sklearn", "pyspacer"}
    pred = load_predictor(model_pt, tmp_path / "model.json", device=0)
    X = Xref[8000:9000]
    want = cm.predict_proba(X)
    assert np.abs(pred.predict_proba(X) - want).max() <= 1e-6
    assert pred.classes == clf.classes_.tolist()
    assert np.abs(cm.predictor().predict_proba(X) - want).max() == 0.0
    with pytest.raises(ParityError):
        export_artifact(cm, tmp_path / "strict", Xref[:512], tol=-1.0)
    assert not (tmp_path / "strict").exists()                    # a failed gate writes nothing
    # the snapshot: later training of the classifier does not move the calibrated model
    before = cm.predict_proba(X[:32])
    clf.partial_fit(Xref[:2000], yref[:2000])
    assert np.array_equal(cm.predict_proba(X[:32]), before)
    pytest.importorskip("sklearn")
    sk = cm.to_sklearn()                                         # built from the snapshot, not the retrained classifier
    assert sk.cv == "prefit" and len(sk.calibrated_classifiers_) == 1
    assert np.abs(sk.predict_proba(X) - want).max() <= 1e-6


@pytest.mark.gpu
def test_device_fit_at_scale():
    rng = np.random.default_rng(11)
    N, K = 200_000, 108
    z = rng.normal(0.0, 2.0, size=(N, K))
    z -= z.max(1, keepdims=True)
    S = np.exp(z)
    S /= S.sum(1, keepdims=True)
    y = (np.argmax(z + rng.gumbel(size=(N, K)), 1)).astype(np.int32)
    a, b, it = _fit_scores(S, y)
    print("scale: iterations", np.bincount(it))
    assert it.max() <= 50
    S32 = S.astype(np.float32).astype(np.float64)   # the device stores fp32 scores: compare on the problem it solved
    worst = 0.0
    for k in range(K):
        pos = y == k
        ah, bh, _ = platt_newton(S32[:, k], pos)
        f, fh = platt_objective(S32[:, k], pos, a[k], b[k]), platt_objective(S32[:, k], pos, ah, bh)
        worst = max(worst, (f - fh) / abs(fh))
        assert f <= fh + 1e-9 * abs(fh), (k, f, fh)
    print("scale: worst relative objective excess", worst)
