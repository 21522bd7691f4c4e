"""Device-resident feature sets (``mmc_featureset_*``, ``FeatureSet``), the passes that read them
(``partial_fit_rows``, ``evaluate`` / ``calibrate`` on a set) and the epoch loop (``epoch_loop``, ``train_classifier``).

CPU: C-ABI and Python argument errors that need no device; ``epoch_loop``'s bookkeeping with a fake classifier and
scripted validation losses.
GPU (-m gpu): every comparison is BITWISE against the host-fed route on the same rows (``partial_fit`` / ``evaluate`` /
``calibrate`` on host arrays) -- the resident routes launch the same step / forward kernels on the same values and sum the
evaluation in integers, so there is nothing to tolerate.  Data: tests/golden/trainer_fixture.npz (730 x 64, 7 classes,
hidden (48, 32); the weighted variant has one class of weight 0)."""

import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def fx():
    d = dict(np.load(GOLDEN / "trainer_fixture.npz"))
    d["y"] = d["classes"][d["y_idx"]]
    return d


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_featureset_c_abi_argument_errors_without_device():
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p(1234)
    assert lib.mmc_featureset_create(0, 3, 0, 0, C.byref(h)) == _lib.MMC_ERR_ARG and h.value is None
    assert b"dim" in lib.mmc_last_error()
    h = C.c_void_p(1234)
    assert lib.mmc_featureset_create(8, 0, 0, 0, C.byref(h)) == _lib.MMC_ERR_ARG and h.value is None
    assert b"n_classes" in lib.mmc_last_error()
    h = C.c_void_p(1234)
    assert lib.mmc_featureset_create(8, 3, 0, -1, C.byref(h)) == _lib.MMC_ERR_ARG and h.value is None
    assert lib.mmc_featureset_create(8, 3, 0, 0, None) == _lib.MMC_ERR_ARG
    if lib.mmc_device_count() == 0:   # valid arguments, no device: still an error, and *out is nulled
        h = C.c_void_p(1234)
        assert lib.mmc_featureset_create(8, 3, 0, 0, C.byref(h)) == _lib.MMC_ERR_HIP and h.value is None
    lib.mmc_featureset_destroy(None)
    assert lib.mmc_featureset_rows(None) == 0 and lib.mmc_featureset_dim(None) == 0
    x, y = np.zeros((1, 8), np.float32), np.zeros(1, np.int32)
    assert lib.mmc_featureset_append(None, x.ctypes.data, y.ctypes.data, 1, _lib.MMC_IN_HOST, None) == _lib.MMC_ERR_ARG
    assert lib.mmc_featureset_read(None, 0, 1, x.ctypes.data, y.ctypes.data, None) == _lib.MMC_ERR_ARG
    avg = C.c_double(0.0)
    assert lib.mmc_trainer_partial_fit_set(None, None, None, 1, 1, C.byref(avg), None) == _lib.MMC_ERR_ARG
    nc, q = C.c_int64(7), C.c_int64(7)
    assert lib.mmc_trainer_evaluate_set_q32(None, None, 0, 1, C.byref(nc), C.byref(q), None) == _lib.MMC_ERR_ARG
    assert lib.mmc_calibrator_add_set(None, None, None, 0, 1, None) == _lib.MMC_ERR_ARG


class _Fake:
    """A 'classifier' that counts its epochs."""

    def __init__(self):
        self.count = 0
        self.loss_curve_ = []


def _run_loop(losses, budget, patience):
    from mermaid_classifier_amd.training import epoch_loop
    calls, seen = [], []

    def train_epoch(clf, epoch):
        clf.count += 1
        clf.loss_curve_.append(10.0 - clf.count)

    def eval_val(clf):
        calls.append(clf.count)
        return 0.5 + 0.01 * clf.count, losses[len(calls) - 1]

    clf, info = epoch_loop(_Fake(), train_epoch, lambda clf: 0.25 * clf.count, eval_val, budget,
                           early_stopping_patience=patience, on_epoch_end=seen.append)
    return clf, info, seen, calls


def test_epoch_loop_stops_after_patience_and_restores_best():
    clf, info, seen, calls = _run_loop([.90, .80, .85, .80, .70], 10, 2)
    assert calls == [1, 2, 3, 4]                       # strict <: the tie at .80 does not reset; .70 is never evaluated
    assert clf.count == 2 and clf.loss_curve_ == [9.0, 8.0]   # the epoch-2 snapshot
    assert [m["epoch"] for m in seen] == [0, 1, 2, 3]
    for m in seen[:-1]:
        assert set(m) == {"epoch", "ref_accuracy", "val_accuracy", "val_loss", "training_loss", "cumulative_seconds"}
    last = seen[-1]
    assert last["final_epoch"] == 4 and last["early_stopped"] is True
    assert last["best_val_epoch"] == 2 and last["best_val_loss"] == .80
    assert last["ref_accuracy"] == 1.0 and last["val_accuracy"] == 0.5 + 0.01 * 4 and last["val_loss"] == .80 and last["training_loss"] == 6.0
    assert last["cumulative_seconds"] >= 0.0
    assert info == {"enabled": True, "patience": 2, "stop_reason": "early_stopping", "final_epoch": 4, "best_val_epoch": 2,
                    "best_val_loss": .80}


def test_epoch_loop_restores_best_after_a_used_up_budget():
    clf, info, seen, calls = _run_loop([.9, .7, .8, .75], 4, 3)
    assert calls == [1, 2, 3, 4] and clf.count == 2
    assert seen[-1]["final_epoch"] == 4 and seen[-1]["early_stopped"] is False
    assert seen[-1]["best_val_epoch"] == 2 and seen[-1]["best_val_loss"] == .7
    assert info["stop_reason"] == "budget_exhausted" and info["best_val_epoch"] == 2 and info["final_epoch"] == 4


def test_epoch_loop_nan_is_no_improvement_and_best_last_keeps_the_live_classifier():
    clf, info, _, calls = _run_loop([.9, float("nan"), .5], 3, 5)
    assert calls == [1, 2, 3] and clf.count == 3 and info["best_val_epoch"] == 3 and info["best_val_loss"] == .5
    clf, info, _, calls = _run_loop([float("nan"), float("nan"), .1], 5, 2)
    assert calls == [1, 2] and clf.count == 2           # no best epoch ever: nothing to restore
    assert info == {"enabled": True, "patience": 2, "stop_reason": "early_stopping", "final_epoch": 2, "best_val_epoch": None,
                    "best_val_loss": None}


def test_epoch_loop_without_patience_takes_no_snapshot(monkeypatch):
    from mermaid_classifier_amd import training

    def boom(obj):
        raise AssertionError("deepcopy called without early stopping")
    monkeypatch.setattr(training.copy, "deepcopy", boom)
    clf, info, seen, calls = _run_loop([.5, .9, .95], 3, None)
    assert calls == [1, 2, 3] and clf.count == 3
    assert seen[-1]["final_epoch"] == 3 and seen[-1]["early_stopped"] is False
    assert not any(k.startswith("best_val") for m in seen for k in m)
    assert info == {"enabled": False, "patience": None, "stop_reason": "budget_exhausted", "final_epoch": 3,
                    "best_val_epoch": None, "best_val_loss": None}


def test_epoch_loop_rejects_patience_below_one():
    from mermaid_classifier_amd.training import epoch_loop
    for bad in (0, -1):
        with pytest.raises(ValueError, match="early_stopping_patience"):
            epoch_loop(_Fake(), lambda c, e: None, lambda c: 0.0, lambda c: (0.0, 0.0), 3, early_stopping_patience=bad)


def test_python_argument_errors_without_device():
    import mermaid_classifier_amd as pkg
    from mermaid_classifier_amd import calibration
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    assert pkg.FeatureSet is not None and pkg.epoch_loop is not None and pkg.train_classifier is not None
    fs = pkg.FeatureSet(4, ["b", "c", "a", "b"])
    assert fs.classes.tolist() == ["a", "b", "c"] and fs.dim == 4 and len(fs) == 0
    with pytest.raises(ValueError, match="5 features, expected 4"):
        fs.append(np.zeros((2, 5), np.float32), ["a", "b"])
    with pytest.raises(ValueError, match="not in classes"):
        fs.append(np.zeros((2, 4), np.float32), ["a", "zz"])
    with pytest.raises(ValueError, match="shape"):
        fs.append(np.zeros((2, 4), np.float32), ["a"])
    with pytest.raises(ValueError):
        pkg.FeatureSet(0, ["a"])
    with pytest.raises(ValueError, match="differ from classes_"):     # first call: the classes handed in are not the set's
        TorchMLPClassifier().partial_fit_rows(fs, classes=["a", "b"])

    class Fitted(TorchMLPClassifier):
        def _fitted(self):
            return True
    clf = Fitted()
    clf.classes_, clf.n_features_in_ = np.array(["a", "b", "c"]), 5
    with pytest.raises(ValueError, match="4 features, expected 5"):
        clf.partial_fit_rows(fs)
    with pytest.raises(ValueError, match="4 features, expected 5"):
        calibration.evaluate(clf, fs)
    clf.classes_, clf.n_features_in_ = np.array(["a", "b", "d"]), 4
    with pytest.raises(ValueError, match="differ from classes_"):
        clf.partial_fit_rows(fs)
    with pytest.raises(ValueError, match="differ from classes_"):
        calibration.calibrate(clf, fs)
    clf.classes_ = np.array(["a", "b", "c"])
    with pytest.raises(ValueError, match="row indices"):
        clf.partial_fit_rows(fs, rows=np.array([0.5, 1.0]))
    clf._h = None   # nothing to release


# ---- GPU --------------------------------------------------------------------------------------------------------------------
def _clf(fx, tag, **kw):
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    cw = {c: float(w) for c, w in zip(fx["classes"], fx["class_weight"])} if tag == "weighted" else None
    args = dict(hidden_layer_sizes=(48, 32), learning_rate_init=1e-3, alpha=1e-3, random_state=0, class_weight=cw)
    args.update(kw)
    return TorchMLPClassifier(**args)


def _fill(fx, parts=(300, 300, 130), rows=None, reserve=0):
    from mermaid_classifier_amd import FeatureSet
    X, y = (fx["X"], fx["y"]) if rows is None else (fx["X"][rows], fx["y"][rows])
    fs = FeatureSet(X.shape[1], fx["classes"], reserve=reserve)
    start = 0
    for n in parts:
        fs.append(X[start:start + n], y[start:start + n])
        start += n
    assert len(fs) == start
    return fs


def _assert_same_state(a, b):
    for u, v in zip(a.parameters(), b.parameters()):
        for p, q in zip(u, v):
            assert np.array_equal(p, q)
    sa, sb = a._adam_state(), b._adam_state()
    assert sa["step"] == sb["step"]
    for name in ("exp_avg", "exp_avg_sq"):
        for u, v in zip(sa[name], sb[name]):
            for p, q in zip(u, v):
                assert np.array_equal(p, q)
    assert a.loss_curve_ == b.loss_curve_ and a.n_iter_ == b.n_iter_


@pytest.fixture(scope="module")
def host_trained(fx):
    """Three host-fed passes per variant: the reference the resident passes must reproduce bit for bit."""
    out = {}
    for tag in ("plain", "weighted"):
        clf = _clf(fx, tag)
        for _ in range(3):
            clf.partial_fit(fx["X"], fx["y"], classes=fx["classes"].tolist())
        out[tag] = clf
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_rows", ["256", None])
@pytest.mark.parametrize("tag", ["plain", "weighted"])
def test_resident_pass_has_the_bits_of_the_host_fed_pass(fx, host_trained, monkeypatch, tag, chunk_rows):
    """At MMC_TRAIN_CHUNK_ROWS=256 a chunk is one 200-row mini-batch, the chunk boundary is crossed three times and the last
    mini-batch has 130 rows; the default takes the pass in one chunk.  The set grows twice while it is filled."""
    if chunk_rows is None:
        monkeypatch.delenv("MMC_TRAIN_CHUNK_ROWS", raising=False)
    else:
        monkeypatch.setenv("MMC_TRAIN_CHUNK_ROWS", chunk_rows)
    fs = _fill(fx)
    X, y = fs.read()
    assert np.array_equal(X, fx["X"]) and np.array_equal(y, fx["y"])       # the rows survived the growth
    X, y = fs.read(295, 10)
    assert np.array_equal(X, fx["X"][295:305]) and np.array_equal(y, fx["y"][295:305])
    clf = _clf(fx, tag)
    for _ in range(3):
        clf.partial_fit_rows(fs, classes=fx["classes"].tolist())
    assert np.array_equal(clf.classes_, fx["classes"]) and clf.n_features_in_ == 64
    _assert_same_state(clf, host_trained[tag])
    fs.close()


@pytest.mark.gpu
def test_resident_pass_over_a_row_subset(fx, monkeypatch):
    monkeypatch.setenv("MMC_TRAIN_CHUNK_ROWS", "200")
    rows = np.arange(729, -1, -2)
    fs = _fill(fx, reserve=730)
    a, b = _clf(fx, "weighted"), _clf(fx, "weighted")
    for _ in range(2):
        a.partial_fit_rows(fs, rows, classes=fx["classes"].tolist())
        b.partial_fit(fx["X"][rows], fx["y"][rows], classes=fx["classes"].tolist())
    _assert_same_state(a, b)
    # without a shuffle and without rows the pass has no visiting order at all
    a, b = _clf(fx, "plain", shuffle=False), _clf(fx, "plain", shuffle=False)
    a.partial_fit_rows(fs)
    b.partial_fit(fx["X"], fx["y"])
    _assert_same_state(a, b)


@pytest.mark.gpu
def test_resident_pass_odd_feature_width():
    """Width 10: rows are neither 16-byte sized nor aligned, the gather moves dwords; the host route shuffles on the host."""
    from mermaid_classifier_amd import FeatureSet
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    rng = np.random.default_rng(2)
    k, nf, n = 5, 10, 333
    yi = rng.integers(0, k, size=n)
    X = (rng.normal(0, 1, size=(k, nf))[yi] + rng.normal(0, 1, size=(n, nf))).astype(np.float32)
    fs = FeatureSet(nf, np.arange(k)).append(X[:100], yi[:100]).append(X[100:], yi[100:])
    a = TorchMLPClassifier(hidden_layer_sizes=(16,), batch_size=50, random_state=1)
    b = TorchMLPClassifier(hidden_layer_sizes=(16,), batch_size=50, random_state=1)
    for _ in range(2):
        a.partial_fit_rows(fs, classes=list(range(k)))
        b.partial_fit(X, yi, classes=list(range(k)))
    _assert_same_state(a, b)
    rows = np.arange(0, n, 3)
    a.partial_fit_rows(fs, rows)
    b.partial_fit(X[rows], yi[rows])
    _assert_same_state(a, b)


@pytest.mark.gpu
def test_evaluate_and_calibrate_from_the_set(fx, host_trained):
    from mermaid_classifier_amd import FeatureSet, _lib, calibration
    clf = host_trained["plain"]
    fs = _fill(fx)
    assert calibration.evaluate(clf, fs) == calibration.evaluate(clf, (fx["X"], fx["y"]))
    lib = _lib.lib()

    def c_call(s, first, n):
        nc, q = C.c_int64(-1), C.c_int64(-1)
        _lib.check(lib.mmc_trainer_evaluate_set_q32(clf._h, s._handle(), first, n, C.byref(nc), C.byref(q), None))
        return np.array([nc.value, q.value], dtype=object)
    whole = c_call(fs, 0, 730)
    assert np.array_equal(c_call(fs, 0, 17) + c_call(fs, 17, 483) + c_call(fs, 500, 230), whole)
    assert np.array_equal(c_call(fs, 730, 0), [0, 0])
    yi = np.ascontiguousarray(fx["y_idx"].astype(np.int32))
    Xc = np.ascontiguousarray(fx["X"])
    nc, q = C.c_int64(-1), C.c_int64(-1)
    _lib.check(lib.mmc_trainer_evaluate_q32(clf._h, Xc.ctypes.data, yi.ctypes.data, 730, C.byref(nc), C.byref(q), None))
    assert [nc.value, q.value] == list(whole)
    for first, n in ((-1, 5), (0, 731), (729, 2), (0, -1)):
        assert lib.mmc_trainer_evaluate_set_q32(clf._h, fs._handle(), first, n, C.byref(nc), C.byref(q), None) == _lib.MMC_ERR_ARG
    # 16 384 + 17 rows: the resident forward crosses its chunk bound
    reps = -(-16401 // 730)
    Xt, yt = np.tile(fx["X"], (reps, 1))[:16401], np.tile(fx["y"], reps)[:16401]
    big = FeatureSet(64, fx["classes"], reserve=16401).append(Xt, yt)
    assert calibration.evaluate(clf, big) == calibration.evaluate(clf, (Xt, yt))
    assert np.array_equal(c_call(big, 0, 16383) + c_call(big, 16383, 18), c_call(big, 0, 16401))
    for s, data in ((fs, (fx["X"], fx["y"])), (big, (Xt, yt))):
        got, want = calibration.calibrate(clf, s), calibration.calibrate(clf, data)
        assert np.array_equal(got.a_, want.a_) and np.array_equal(got.b_, want.b_)
        assert np.array_equal(got.iterations_, want.iterations_)
    fs.close()
    big.close()


@pytest.mark.gpu
def test_append_device(fx, synth_sd):
    import torch
    from mermaid_classifier_amd import Backbone, FeatureSet
    from oracle import efficientnet_b0_ref as ref
    X = np.ascontiguousarray(fx["X"])
    Xd = torch.from_numpy(X).cuda()
    fs = FeatureSet(64, fx["classes"]).append_device(Xd[:400], fx["y"][:400]).append_device(Xd[400:], fx["y"][400:])
    got_X, got_y = fs.read()
    assert np.array_equal(got_X, X) and np.array_equal(got_y, fx["y"])
    for bad in (Xd.double(), Xd.cpu(), Xd[:, :63], Xd.t().contiguous().t(), Xd.reshape(-1), X):
        with pytest.raises(ValueError):
            fs.append_device(bad, fx["y"][:bad.shape[0]])
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="live on"):
            fs.append_device(Xd.to("cuda:1"), fx["y"])
    with pytest.raises(ValueError, match="not in classes"):
        fs.append_device(Xd[:2], ["c0", "nope"])
    assert len(fs) == 730
    # features straight out of the backbone never visit the host
    bb = Backbone(synth_sd, device=0, max_batch=4)
    patches = ref.natural_patches(4, seed=7)
    feats = bb.extract(torch.from_numpy(patches).cuda())
    bset = FeatureSet(bb.feature_dim, [0, 1, 2]).append_device(feats, [2, 0, 1, 2])
    got_X, got_y = bset.read()
    assert np.array_equal(got_X, bb.extract(patches)) and got_y.tolist() == [2, 0, 1, 2]
    bb.close()


@pytest.mark.gpu
def test_train_classifier_matches_the_host_written_loop(fx):
    from mermaid_classifier_amd import FeatureSet, calibration, train_classifier
    X, y, classes = fx["X"], fx["y"], fx["classes"].tolist()
    tr, rf, vl = slice(0, 500), slice(500, 630), slice(630, 730)
    sets = [FeatureSet(64, classes).append(X[s], y[s]) for s in (tr, rf, vl)]
    seen = []
    cal, info, ref_accs = train_classifier(*sets, 4, batch_size=300, early_stopping_patience=2, on_epoch_end=seen.append,
                                           clf=_clf(fx, "plain"))
    # the same loop on host arrays
    import copy
    clf = _clf(fx, "plain")
    want_seen, want_accs = [], []
    best, best_epoch, best_clf, since, reason = float("inf"), None, None, 0, "budget_exhausted"
    for epoch in range(4):
        for start in (0, 300):
            clf.partial_fit(X[tr][start:start + 300], y[tr][start:start + 300], classes=classes)
        want_accs.append(calibration.evaluate(clf, (X[rf], y[rf]))[0])
        va, vloss = calibration.evaluate(clf, (X[vl], y[vl]))
        if vloss < best:
            best, best_epoch, best_clf, since = vloss, epoch, copy.deepcopy(clf), 0
        else:
            since += 1
        stop = since >= 2
        m = {"epoch": epoch, "ref_accuracy": want_accs[-1], "val_accuracy": va, "val_loss": vloss, "training_loss": clf.loss_curve_[-1]}
        if stop or epoch == 3:
            m.update(final_epoch=epoch + 1, early_stopped=stop, best_val_epoch=best_epoch + 1, best_val_loss=best)
        want_seen.append(m)
        if stop:
            reason = "early_stopping"
            break
    if best_epoch != epoch:
        clf = best_clf
    want = calibration.calibrate(clf, (X[rf], y[rf]))
    print("val losses", [m["val_loss"] for m in want_seen], "info", info)
    assert ref_accs == want_accs
    assert [{k: v for k, v in m.items() if k != "cumulative_seconds"} for m in seen] == want_seen
    assert all(m["cumulative_seconds"] >= 0.0 for m in seen)
    assert info == {"enabled": True, "patience": 2, "stop_reason": reason, "final_epoch": epoch + 1,
                    "best_val_epoch": best_epoch + 1, "best_val_loss": best}
    for u, v in zip(cal.weights + cal.biases, want.weights + want.biases):
        assert np.array_equal(u, v)
    assert np.array_equal(cal.a_, want.a_) and np.array_equal(cal.b_, want.b_)


@pytest.mark.gpu
def test_rejected_passes_leave_the_state_alone(fx, monkeypatch):
    fs = _fill(fx, reserve=730)
    classes = fx["classes"].tolist()
    a, b = _clf(fx, "weighted"), _clf(fx, "weighted")
    a.partial_fit_rows(fs, classes=classes)
    b.partial_fit_rows(fs, classes=classes)
    zero = fx["classes"][np.flatnonzero(fx["class_weight"] == 0)[0]]
    dead = np.flatnonzero(fx["y"] == zero)
    assert dead.size > 0
    with pytest.raises(ValueError, match="outside"):
        a.partial_fit_rows(fs, np.array([0, 5, 730]))
    with pytest.raises(ValueError, match="outside"):
        a.partial_fit_rows(fs, np.array([3, -1]))
    with pytest.raises(ValueError, match="zero total class weight"):
        a.partial_fit_rows(fs, dead)
    monkeypatch.setenv("MMC_TRAIN_CHUNK_ROWS", "0")
    with pytest.raises(ValueError, match="MMC_TRAIN_CHUNK_ROWS"):
        a.partial_fit_rows(fs)
    monkeypatch.delenv("MMC_TRAIN_CHUNK_ROWS")
    assert a.n_iter_ == 1 and len(a.loss_curve_) == 1
    a.partial_fit_rows(fs)
    b.partial_fit_rows(fs)
    _assert_same_state(a, b)
