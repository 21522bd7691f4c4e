"""Logit calibration without a device: the checker against autograd, the teeth of its bounds, the algebra of ``LogitScaling`` and
every argument error that must be raised before a device is touched."""

import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import logit_scaling_checker as ck  # noqa: E402


def _small(N=40, K=5, seed=3):
    z, y = ck.fixture(N, K, seed=seed)
    rng = np.random.default_rng(seed + 1)
    a = rng.uniform(0.2, 3.0, K)
    a[1] = -0.7
    c = rng.standard_normal(K)
    return z, y, a, c


@pytest.mark.parametrize("kind", ck.KINDS)
def test_checker_gradient_and_hessian_agree_with_autograd(kind):
    import torch
    z, y, a, c = _small()
    N, K = z.shape
    if kind == "temperature":
        a, c = np.full(K, 0.6), np.zeros(K)
    elif kind == "bias":
        a = np.ones(K)
    zt, yt = torch.from_numpy(z.astype(np.float64)), torch.from_numpy(y.astype(np.int64))

    def F(theta):
        if kind == "temperature":
            u = theta[0] * zt
        elif kind == "bias":
            u = zt + theta[None, :]
        else:
            u = theta[None, :K] * zt + theta[None, K:]
        return (torch.logsumexp(u, dim=1) - u[torch.arange(N), yt]).sum()

    theta0 = {"temperature": a[:1], "bias": c, "vector": np.concatenate([a, c])}[kind]
    theta = torch.tensor(theta0, dtype=torch.float64, requires_grad=True)
    g_ref = torch.autograd.grad(F(theta), theta)[0].numpy()
    H_ref = torch.autograd.functional.hessian(F, theta.detach()).numpy()
    st = ck.stats(z, y, a, c)
    assert abs(st["nll"] - float(F(theta).detach())) <= 1e-12 * abs(st["nll"])
    g, H = st["grad"], st["hess"]
    if kind == "temperature":
        g_got, H_got = np.array([g[:K].sum()]), np.array([[H[:K, :K].sum()]])
    elif kind == "bias":
        g_got, H_got = g[K:], H[K:, K:]
    else:
        g_got, H_got = g, H
    assert np.abs(g_got - g_ref).max() <= 1e-11 * max(1.0, np.abs(g_ref).max())
    assert np.abs(H_got - H_ref).max() <= 1e-11 * max(1.0, np.abs(H_ref).max())
    assert np.array_equal(H, H.T)
    assert np.array_equal(st["counts"], np.bincount(y, minlength=K))


def test_bounds_have_teeth_float32_sums_violate_them():
    """The same sums accumulated in float32 (terms in float64, rounded, added in row order) break the 1x gate somewhere."""
    z, y = ck.fixture(700, 5)
    N, K = z.shape
    a, c = np.ones(K), np.zeros(K)
    st = ck.stats(z, y, a, c)
    b_nll, b_grad, b_hess = ck.bounds(st, N, K)
    p = st["p"]
    onehot = np.zeros((N, K))
    onehot[np.arange(N), y] = 1.0
    r = p - onehot
    zd = z.astype(np.float64)
    g32 = np.concatenate([np.cumsum((zd * r).astype(np.float32), axis=0, dtype=np.float32)[-1],
                          np.cumsum(r.astype(np.float32), axis=0, dtype=np.float32)[-1]]).astype(np.float64)
    v = np.concatenate([zd * p, p], axis=1)
    S32 = np.zeros((2 * K, 2 * K), np.float32)
    for n in range(N):
        S32 += np.outer(v[n], v[n]).astype(np.float32)
    H32 = -S32.astype(np.float64)
    k = np.arange(K)
    H32[k, k] += (zd * zd * p).sum(axis=0)
    H32[K + k, K + k] += p.sum(axis=0)
    H32[k, K + k] += (zd * p).sum(axis=0)
    H32[K + k, k] += (zd * p).sum(axis=0)
    ratio_g = np.abs(g32 - st["grad"]) / b_grad
    ratio_h = np.abs(H32 - st["hess"]) / b_hess
    print("float32 accumulation: worst gradient ratio", ratio_g.max(), "worst Hessian ratio", ratio_h.max())
    assert ratio_g.max() > 1.0 and ratio_h.max() > 1.0
    # and float64 in another order (numpy's pairwise sums against a plain row-order chain) stays inside
    g64 = np.concatenate([np.cumsum(zd * r, axis=0)[-1], np.cumsum(r, axis=0)[-1]])
    assert (np.abs(g64 - st["grad"]) <= b_grad).all()
    assert b_nll > 0 and b_nll < 1e-9 * abs(st["nll"])


def test_reference_fit_meets_the_criterion_on_the_small_fixture():
    z, y = ck.fixture(700, 5)
    for kind in ck.KINDS:
        res = ck.fit(z, y, kind)
        g, bound = ck.active_gradient(z, y, res["a"], res["c"], kind)
        assert res["converged"] and res["trials"] <= 100 and res["nll_after"] <= res["nll_before"]
        assert (np.abs(g) / len(y) <= 1e-9 + bound / len(y)).all()
        assert abs(res["c"].mean()) <= 1e-9


def _scaling(K=6, seed=0, kind="vector"):
    from mermaid_classifier_amd import LogitScaling
    rng = np.random.default_rng(seed)
    return LogitScaling(kind, rng.uniform(0.3, 2.5, K), rng.standard_normal(K))


def test_fold_is_the_float32_rounding_of_the_float64_product_bit_for_bit():
    rng = np.random.default_rng(5)
    K, h, d = 6, 9, 11
    ws = [rng.standard_normal((h, d)).astype(np.float32), rng.standard_normal((K, h)).astype(np.float32)]
    bs = [rng.standard_normal(h).astype(np.float32), rng.standard_normal(K).astype(np.float32)]
    sc = _scaling(K)
    fw, fb = sc.fold(ws, bs)
    assert fw[1].dtype == np.float32 and fb[1].dtype == np.float32
    want_w = np.empty((K, h), np.float32)
    want_b = np.empty(K, np.float32)
    for k in range(K):
        for j in range(h):
            want_w[k, j] = np.float32(float(sc.a[k]) * float(ws[1][k, j]))
        want_b[k] = np.float32(float(sc.a[k]) * float(bs[1][k]) + float(sc.c[k]))
    assert fw[1].tobytes() == want_w.tobytes() and fb[1].tobytes() == want_b.tobytes()
    assert fw[0].tobytes() == ws[0].tobytes() and fb[0].tobytes() == bs[0].tobytes()
    assert fw[0] is not ws[0]
    with pytest.raises(ValueError, match="logits"):
        sc.fold([ws[0]], [bs[0]])


def test_apply_of_the_folded_float64_weights_is_a_z_plus_c():
    rng = np.random.default_rng(6)
    K, h = 6, 9
    W, b = rng.standard_normal((K, h)), rng.standard_normal(K)
    hid = rng.standard_normal((20, h))
    sc = _scaling(K)
    z = hid @ W.T + b
    folded = hid @ (sc.a[:, None] * W).T + (sc.a * b + sc.c)
    assert np.abs(folded - sc.apply(z)).max() <= 1e-13 * np.abs(folded).max()
    assert np.array_equal(sc.apply(z), sc.a[None, :] * z + sc.c[None, :])
    with pytest.raises(ValueError, match="logits must be"):
        sc.apply(np.zeros((3, K + 1)))


def test_fold_commutes_with_the_feature_transform_fold_on_a_head_with_no_hidden_layer():
    """One Linear layer is first and last at once: scaling first, then the transform, is the head a * (W T (x - mu) + b) + c."""
    from mermaid_classifier_amd import FeatureTransform
    rng = np.random.default_rng(7)
    K, m, dim = 6, 4, 7
    W, b = rng.standard_normal((K, m)).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    ft = FeatureTransform("pca", rng.standard_normal(dim), rng.standard_normal((m, dim)), np.ones(m))
    sc = _scaling(K)
    w1, b1 = sc.fold([W], [b])
    w2, b2 = ft.fold(w1, b1)
    x = rng.standard_normal((15, dim))
    want = sc.apply(ft.transform_rows(x) @ W.astype(np.float64).T + b.astype(np.float64))
    got = x @ w2[0].astype(np.float64).T + b2[0].astype(np.float64)
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 64 * 2.0 ** -24 * scale   # two float32 roundings of the weights, m + dim terms
    # the other order folds the same function too (both are exact in float64)
    w3, b3 = ft.fold([W], [b])
    w4, b4 = sc.fold(w3, b3)
    got2 = x @ w4[0].astype(np.float64).T + b4[0].astype(np.float64)
    assert np.abs(got2 - want).max() <= 64 * 2.0 ** -24 * scale


def test_python_argument_validation():
    from mermaid_classifier_amd import LogitScaling, calibration, fit_logit_scaling, logit_scaling
    from mermaid_classifier_amd.sweep import SweepConfig
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    with pytest.raises(ValueError, match="kind"):
        LogitScaling("matrix", np.ones(3), np.zeros(3))
    with pytest.raises(ValueError, match="K,"):
        LogitScaling("vector", np.ones(3), np.zeros(4))
    with pytest.raises(ValueError, match="finite"):
        LogitScaling("vector", [1.0, np.nan, 1.0], np.zeros(3))
    with pytest.raises(ValueError, match="frozen"):
        LogitScaling("vector", np.ones(3), np.zeros(3), frozen=[True])
    t = LogitScaling("temperature", np.full(4, 0.5), np.zeros(4))
    assert t.temperature == 2.0 and t.n_classes == 4
    with pytest.raises(AttributeError):
        LogitScaling("bias", np.ones(3), np.zeros(3)).temperature
    data = (np.zeros((2, 4), np.float32), np.zeros(2))
    for kwargs, match in (({"kind": "dirichlet"}, "kind"), ({"l2": -1.0}, "l2"), ({"tol": 0.0}, "tol"), ({"max_trials": 0}, "max_trials"),
                          ({"max_trials": 1001}, "max_trials"), ({"l2": float("nan")}, "l2")):
        with pytest.raises(ValueError, match=match):
            fit_logit_scaling(TorchMLPClassifier(), data, **kwargs)
    with pytest.raises(RuntimeError, match="not fitted"):
        fit_logit_scaling(TorchMLPClassifier(), data)
    with pytest.raises(RuntimeError, match="not fitted"):
        t.fold_classifier(TorchMLPClassifier())
    with pytest.raises(RuntimeError, match="not fitted"):
        calibration.calibrate(TorchMLPClassifier(), data, logit_scaling="vector")
    with pytest.raises(ValueError, match="logit_scaling"):
        logit_scaling.check_argument("platt")
    with pytest.raises(ValueError, match="logit_scaling"):
        logit_scaling.check_argument(3)
    logit_scaling.check_argument("bias")
    logit_scaling.check_argument(t)
    assert SweepConfig().logit_scaling is None and SweepConfig(logit_scaling="vector").logit_scaling == "vector"

    class Wide(TorchMLPClassifier):
        def _fitted(self):
            return True
    clf = Wide()
    clf.classes_ = np.arange(129)
    clf.n_features_in_ = 4
    with pytest.raises(ValueError, match="2 to 128 classes"):
        fit_logit_scaling(clf, data)


def test_c_abi_argument_errors_without_device():
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p(1234)
    assert lib.mmc_logitcal_create(129, 0, C.byref(h)) == _lib.MMC_ERR_ARG and h.value is None
    assert b"[2, 128]" in lib.mmc_last_error()
    h = C.c_void_p(1234)
    assert lib.mmc_logitcal_create(1, 0, C.byref(h)) == _lib.MMC_ERR_ARG and h.value is None
    assert lib.mmc_logitcal_create(5, 0, None) == _lib.MMC_ERR_ARG
    a = np.ones(8)
    z = np.zeros(8, np.float32)
    yy = np.zeros(2, np.int32)
    nll, before, after = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    trials, conv = C.c_int32(0), C.c_int32(0)
    assert lib.mmc_logitcal_stats(None, a.ctypes.data, a.ctypes.data, C.byref(nll), a.ctypes.data, None, None, None) == _lib.MMC_ERR_ARG
    assert lib.mmc_logitcal_fit(None, 0, 0.0, 1e-9, 100, a.ctypes.data, a.ctypes.data, None, C.byref(before), C.byref(after),
                                C.byref(trials), C.byref(conv), None) == _lib.MMC_ERR_ARG
    assert lib.mmc_logitcal_add_logits(None, z.ctypes.data, yy.ctypes.data, 2, None) == _lib.MMC_ERR_ARG
    assert lib.mmc_logitcal_add_features(None, None, None, None, 1, None) == _lib.MMC_ERR_ARG
    assert lib.mmc_logitcal_add_set(None, None, None, 0, 1, None) == _lib.MMC_ERR_ARG
    assert lib.mmc_logitcal_rows(None) == 0
    lib.mmc_logitcal_destroy(None)
    for name in ("mmc_logitcal_create", "mmc_logitcal_destroy", "mmc_logitcal_rows", "mmc_logitcal_add_features", "mmc_logitcal_add_set",
                 "mmc_logitcal_add_logits", "mmc_logitcal_stats", "mmc_logitcal_fit"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert (_lib.MMC_LOGITCAL_MAX_CLASSES, _lib.MMC_LOGITCAL_BLOCK_ROWS) == (ck.MAX_CLASSES, ck.BLOCK_ROWS)
    header = (Path(__file__).resolve().parents[1] / "include" / "mmc.h").read_text()
    assert f"#define MMC_LOGITCAL_BLOCK_ROWS {ck.BLOCK_ROWS}" in header and f"#define MMC_LOGITCAL_MAX_CLASSES {ck.MAX_CLASSES}" in header


def test_package_exports_the_new_names():
    import mermaid_classifier_amd as pkg
    from mermaid_classifier_amd import logit_scaling
    assert pkg.LogitScaling is logit_scaling.LogitScaling and pkg.fit_logit_scaling is logit_scaling.fit_logit_scaling
    assert "LogitScaling" in pkg.__all__ and "fit_logit_scaling" in pkg.__all__
    assert set(logit_scaling.KINDS) == set(ck.KINDS)
