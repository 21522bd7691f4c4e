"""Loss formulations of the MLP trainer (label smoothing, focal loss, logit prior), the part that needs no device.

Surface: constructor / ``SweepConfig`` defaults and errors, ``get_params`` / ``set_params``, pickles from before the options,
``sampling.logit_adjustment``, and the two C entry points rejecting bad arguments before they touch a device.

Checker and bound (tests/loss_checker.py): the fp64 autograd checker equals ``F.cross_entropy(weight=, label_smoothing=)`` at
gamma = 0 to 1e-12; a numpy fp32 emulation of the kernel's arithmetic stays within half of the per-element bounds that
tests/test_gpu_loss.py holds the device to, and three wrong kernels (focal term dropped, smoothing term dropped, prior not added)
exceed the ``dlogits`` bound at least 100 times."""

import ctypes as C
import itertools
import pickle

import numpy as np
import pytest

import loss_checker as lc

KS = (3, 5, 64, 65, 108, 130, 300)
EPS = (0.0, 0.1, 0.3)
GAMMAS = (0.0, 1.0, 2.0, 5.0, 8.0)
SCALES = (1.0, 4.0, 10.0)


# ---- surface ----------------------------------------------------------------------------------------------------------------
def test_classifier_and_sweep_config_loss_options():
    import mermaid_classifier_amd as pkg
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    clf = TorchMLPClassifier()
    assert (clf.label_smoothing, clf.focal_gamma, clf.logit_prior) == (0.0, 0.0, None)
    params = clf.get_params()
    assert params["label_smoothing"] == 0.0 and params["focal_gamma"] == 0.0 and params["logit_prior"] is None
    for bad in (-0.1, 1.0, 1.5, float("nan"), "0.1", None, True):
        with pytest.raises(ValueError, match="label_smoothing"):
            TorchMLPClassifier(label_smoothing=bad)
    for bad in (0.5, -1.0, 8.5, 0.999, float("nan"), float("inf"), "2", None):
        with pytest.raises(ValueError, match="focal_gamma"):
            TorchMLPClassifier(focal_gamma=bad)
    for eps, gamma in ((0.0, 1.0), (0.999, 8.0), (0.3, 2.5), (0, 0)):
        TorchMLPClassifier(label_smoothing=eps, focal_gamma=gamma)
    # positional callers are undisturbed: `device` is still the 15th argument and the options do not follow it positionally
    pos = TorchMLPClassifier((8,), "relu", "adam", 1e-4, "auto", 1e-3, 200, True, 0, 1e-4, 0.9, 0.999, 1e-8, None, "cuda:0")
    assert pos.device == "cuda:0" and pos.label_smoothing == 0.0
    prior = {"a": -0.5, "b": -1.0}
    clf = TorchMLPClassifier(label_smoothing=0.1, focal_gamma=2.0, logit_prior=prior)
    assert clf.get_params() == dict(TorchMLPClassifier().get_params(), label_smoothing=0.1, focal_gamma=2.0, logit_prior=prior)
    clf.set_params(label_smoothing=0.2, focal_gamma=1.0, logit_prior=None)
    assert (clf.label_smoothing, clf.focal_gamma, clf.logit_prior) == (0.2, 1.0, None)
    # the prior is resolved in classes_ order, like class_weight
    clf = TorchMLPClassifier(logit_prior={"b": -1.0, "a": -0.5, "c": 0.25})
    clf.classes_ = np.array(["a", "b", "c"])
    vec = clf._build_logit_prior_vector()
    assert vec.dtype == np.float32 and vec.tolist() == [-0.5, -1.0, 0.25]
    clf.logit_prior = {"a": 0.0, "c": 0.0}
    with pytest.raises(ValueError, match=r"logit_prior is missing offsets for \['b'\]"):
        clf._build_logit_prior_vector()
    for bad in (float("nan"), float("-inf"), 1e39):
        clf.logit_prior = {"a": 0.0, "b": bad, "c": 0.0}
        with pytest.raises(ValueError, match="not finite"):
            clf._build_logit_prior_vector()
    clf.logit_prior = None
    assert clf._build_logit_prior_vector() is None

    cfg = pkg.SweepConfig()
    assert (cfg.label_smoothing, cfg.focal_gamma, cfg.logit_prior) == (0.0, 0.0, None)
    assert cfg.classifier().get_params() == TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), learning_rate_init=1e-4,
                                                               random_state=0).get_params()
    # the three fields follow `batches`, so positional SweepConfig callers are undisturbed too
    names = list(pkg.SweepConfig.__dataclass_fields__)
    assert names[names.index("batches") + 1:] == ["label_smoothing", "focal_gamma", "logit_prior"]
    got = pkg.SweepConfig(hidden_layer_sizes=(8,), label_smoothing=0.1, focal_gamma=2.0, logit_prior=prior).classifier("cuda:0")
    assert (got.label_smoothing, got.focal_gamma, got.logit_prior, got.device) == (0.1, 2.0, prior, "cuda:0")
    with pytest.raises(ValueError, match="focal_gamma"):
        pkg.SweepConfig(focal_gamma=0.5).classifier()


def test_state_from_before_the_options_loads_as_plain():
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    clf = TorchMLPClassifier(hidden_layer_sizes=(8,), label_smoothing=0.1, focal_gamma=2.0, logit_prior={"a": 0.0})
    twin = pickle.loads(pickle.dumps(clf))
    assert twin.get_params() == clf.get_params() and not twin._fitted()
    old = {k: v for k, v in clf.__getstate__().items() if k not in ("label_smoothing", "focal_gamma", "logit_prior")}
    assert "class_weight" in old and "label_smoothing" not in old
    back = TorchMLPClassifier.__new__(TorchMLPClassifier)
    back.__setstate__(dict(old))
    assert (back.label_smoothing, back.focal_gamma, back.logit_prior) == (0.0, 0.0, None)
    assert back.get_params() == TorchMLPClassifier(hidden_layer_sizes=(8,)).get_params() and not back._fitted()


def test_logit_adjustment():
    import mermaid_classifier_amd as pkg
    from mermaid_classifier_amd import sampling
    assert pkg.logit_adjustment is sampling.logit_adjustment and "logit_adjustment" in pkg.__all__
    counts = {"a": 300, "b": 80, "c": 20}
    got = pkg.logit_adjustment(counts)
    assert list(got) == ["a", "b", "c"]
    for k, c in counts.items():
        assert got[k] == pytest.approx(np.log(c / 400.0), rel=1e-15, abs=0)
    half = pkg.logit_adjustment(counts, tau=0.5)
    assert all(half[k] == pytest.approx(0.5 * got[k], rel=1e-15) for k in counts)
    assert pkg.logit_adjustment({7: 5}) == {7: 0.0}
    assert pkg.logit_adjustment({k: np.int64(c) for k, c in counts.items()}) == got
    with pytest.raises(ValueError, match="empty"):
        pkg.logit_adjustment({})
    for bad in (0, -3):
        with pytest.raises(ValueError, match=">= 1"):
            pkg.logit_adjustment({"a": 10, "b": bad})


def test_loss_c_abi_argument_errors_without_device():
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    assert {"mmc_trainer_set_loss", "mmc_trainer_loss_gradient"} <= set(_lib.SYMBOLS)
    fake = C.c_void_p(1234)          # never dereferenced: the calls below fail before the trainer is looked at
    prior = (C.c_float * 3)(0.0, 0.0, 0.0)
    assert lib.mmc_trainer_set_loss(None, 0.1, 2.0, prior) == _lib.MMC_ERR_ARG
    assert b"NULL" in lib.mmc_last_error()
    for eps in (-0.1, 1.0, 2.0, float("nan"), float("inf")):
        assert lib.mmc_trainer_set_loss(fake, eps, 0.0, None) == _lib.MMC_ERR_ARG
        assert b"label_smoothing" in lib.mmc_last_error()
    for gamma in (-1.0, 0.5, 0.999, 8.001, float("nan"), float("inf")):
        assert lib.mmc_trainer_set_loss(fake, 0.0, gamma, None) == _lib.MMC_ERR_ARG
        assert b"focal_gamma" in lib.mmc_last_error()
    buf = (C.c_float * 6)()
    yb = (C.c_int32 * 2)(0, 1)
    assert lib.mmc_trainer_loss_gradient(None, buf, yb, 2, buf, buf, None) == _lib.MMC_ERR_ARG
    assert b"trainer handle is NULL" in lib.mmc_last_error()
    for args in ((None, yb, 2, buf, buf), (buf, None, 2, buf, buf), (buf, yb, 2, None, buf), (buf, yb, 2, buf, None)):
        assert lib.mmc_trainer_loss_gradient(fake, *args, None) == _lib.MMC_ERR_ARG
        assert b"NULL" in lib.mmc_last_error()
    for n in (0, -1, 16385, 1 << 40):
        assert lib.mmc_trainer_loss_gradient(fake, buf, yb, n, buf, buf, None) == _lib.MMC_ERR_ARG
        assert b"outside [1, 16384]" in lib.mmc_last_error()


# ---- the checker and the bound ------------------------------------------------------------------------------------------------
def _cases():
    """Every K x (eps, gamma) x logit scale, each without and with class weights + prior; 24 rows, the four special ones included."""
    for K, (eps, gamma), scale in itertools.product(KS, itertools.product(EPS, GAMMAS), SCALES):
        rng = np.random.default_rng([K, int(eps * 10), int(gamma), int(scale)])
        z, y = lc.logit_rows(rng, 24, K, scale)
        w, prior = lc.class_weights(rng, K), lc.dirichlet_prior(rng, K)
        yield dict(z=z, y=y, w=None, prior=None, eps=eps, gamma=gamma)
        yield dict(z=z, y=y, w=w, prior=prior, eps=eps, gamma=gamma)


def test_checker_is_torch_cross_entropy_at_gamma_zero():
    import torch
    import torch.nn.functional as F
    worst = 0.0
    for case in _cases():
        if case["gamma"] != 0.0:
            continue
        grad, rows, L, (u, yt, wt) = lc.checker(**case)
        u = u.clone().requires_grad_(True)
        want = F.cross_entropy(u, yt, weight=wt, label_smoothing=case["eps"])
        want.backward()
        worst = max(worst, abs(L - float(want)), float(np.abs(grad - u.grad.numpy()).max()))
        assert abs(rows.sum() - L) <= 1e-12
    print(f"checker vs F.cross_entropy, loss and gradient: {worst:.2e}")
    assert worst <= 1e-12


def _units(case, d, l):
    """-> (largest dlogits error, largest row_loss error) of ``d`` / ``l`` against the checker, as fractions of the bounds."""
    grad, rows, _, _ = lc.checker(**case)
    bd, bl = lc.bounds(case["y"], case["w"], rows)
    assert np.isfinite(d).all() and np.isfinite(l).all() and np.isfinite(grad).all() and np.isfinite(rows).all()
    return float(np.abs(d - grad).max() / bd), float((np.abs(l - rows) / bl).max())


def test_fp32_emulation_within_half_the_bounds_and_wrong_kernels_far_outside():
    peak_d = peak_l = 0.0
    wrong = {"drop_focal": 0.0, "drop_smoothing": 0.0, "drop_prior": 0.0}
    for case in _cases():
        fd, fl = _units(case, *lc.emulate(**case))
        peak_d, peak_l = max(peak_d, fd), max(peak_l, fl)
        active = {"drop_focal": case["gamma"] != 0.0, "drop_smoothing": case["eps"] != 0.0, "drop_prior": case["prior"] is not None}
        for flag, on in active.items():
            if on:
                wrong[flag] = max(wrong[flag], _units(case, *lc.emulate(**case, **{flag: True}))[0])
    print(f"emulation peaks: dlogits {peak_d * lc.DLOGITS_UNITS:.1f} of {lc.DLOGITS_UNITS:.0f} units, "
          f"row_loss {peak_l * lc.ROW_LOSS_UNITS:.1f} of {lc.ROW_LOSS_UNITS:.0f} units; wrong kernels (x the dlogits bound): {wrong}")
    assert peak_d <= 0.5 and peak_l <= 0.5
    assert all(v >= 100.0 for v in wrong.values())


def test_plain_emulation_is_within_the_bounds_too():
    """All defaults through the general arithmetic is the plain loss: the same bound holds (the device runs its plain kernel there)."""
    rng = np.random.default_rng(5)
    for K in KS:
        z, y = lc.logit_rows(rng, 24, K, 4.0)
        for w in (None, lc.class_weights(rng, K)):
            fd, fl = _units(dict(z=z, y=y, w=w, prior=None, eps=0.0, gamma=0.0), *lc.emulate(z, y, w))
            assert fd <= 0.5 and fl <= 0.5
