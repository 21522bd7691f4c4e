#!/usr/bin/env python3
"""GPU box: one sha256 line per case over everything a trainer entry point computes, to compare two builds of the library bit for
bit (run it on both checkouts in one visit; the two outputs must be identical line for line: profiles/solo_as_group_bits.txt).

A training case hashes the parameters, both Adam moments, the step count and loss_curve_; the other cases hash the raw bytes of
the outputs they name.  Every case trains one classifier on its own (no grouped call), on the 730 x 64 rows of
tests/golden/trainer_fixture.npz.  Seconds in all."""
import ctypes as C
import hashlib
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from mermaid_classifier_amd import FeatureSet, _lib, calibrate  # noqa: E402
from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier, _ptr_array  # noqa: E402

fx = dict(np.load(ROOT / "tests" / "golden" / "trainer_fixture.npz"))
X, classes = fx["X"], fx["classes"]
y = classes[fx["y_idx"]]
WEIGHTS = {c: float(w) for c, w in zip(classes, fx["class_weight"])}
lib = _lib.lib()


def digest(*parts):
    h = hashlib.sha256()
    for p in parts:
        a = np.ascontiguousarray(p)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def state(clf):
    s = clf._adam_state()
    arrays = [a for part in clf.parameters() for a in part]
    arrays += [a for key in ("exp_avg", "exp_avg_sq") for part in s[key] for a in part]
    return digest(*arrays, np.int64(s["step"]), np.asarray(clf.loss_curve_, np.float64))


def clf_of(hidden=(48, 32), weighted=False, **kw):
    args = dict(hidden_layer_sizes=hidden, learning_rate_init=1e-3, alpha=1e-3, random_state=0, class_weight=WEIGHTS if weighted else None)
    args.update(kw)
    return TorchMLPClassifier(**args)


def heterogeneous():
    """The members of tests/test_sweep.py::_heterogeneous."""
    return [(clf_of((48, 32), weighted=True, batch_size=200), None),
            (clf_of((70,), learning_rate_init=3e-3, alpha=0.0, batch_size=64), np.arange(729, -1, -2)),
            (clf_of((), batch_size="auto"), np.arange(0, 97 * 7, 7)),
            (clf_of((33, 17, 9), random_state=3, batch_size=730), None),
            (clf_of((48, 32), shuffle=False), None)]


def show(name, value):
    print(f"{name:44s} {value}", flush=True)


# host-fed passes: the ordered path (width 64) and the host-shuffle path (width 10)
for weighted in (False, True):
    clf = clf_of(weighted=weighted)
    for _ in range(3):
        clf.partial_fit(X, y, classes=classes.tolist())
    show(f"host-fed ordered {'weighted' if weighted else 'plain'} x3", state(clf))
clf = clf_of(weighted=True, batch_size=64)
clf.partial_fit(X[:, :10], y, classes=classes.tolist())
show("host-fed width 10 weighted", state(clf))

# resident passes, one trainer per call
fs = FeatureSet(64, classes, reserve=730).append(X, y)
for chunk in ("256", None):
    if chunk is None:
        os.environ.pop("MMC_TRAIN_CHUNK_ROWS", None)
    else:
        os.environ["MMC_TRAIN_CHUNK_ROWS"] = chunk
    for i, (clf, rows) in enumerate(heterogeneous()):
        for _ in range(3):
            clf.partial_fit_rows(fs, rows, classes=classes.tolist())
        show(f"resident member {i} chunk {chunk or 'default'} x3", state(clf))
prior = {c: float(v) for c, v in zip(classes, 0.7 * np.log(np.random.default_rng(1).dirichlet(np.ones(len(classes)))))}
KINDS = {"smoothing": dict(label_smoothing=0.1), "focal": dict(focal_gamma=2.0), "prior": dict(logit_prior=prior),
         "all": dict(label_smoothing=0.1, focal_gamma=2.0, logit_prior=prior)}
for kind, opts in KINDS.items():
    clf = clf_of(weighted=True, **opts)
    clf.partial_fit_rows(fs, None, classes=classes.tolist())
    show(f"resident weighted loss {kind}", state(clf))

# the eval-mode forward: host rows, then rows of the set (evaluate totals, Platt a / b)
clf = clf_of(weighted=True)
clf.partial_fit_rows(fs, None, classes=classes.tolist())
logits = np.empty((64, len(classes)), np.float32)
_lib.check(lib.mmc_trainer_logits(clf._h, np.ascontiguousarray(X[:64]).ctypes.data, 64, logits.ctypes.data, None))
show("logits 64 rows", digest(logits))
nc, q = C.c_int64(0), C.c_int64(0)
_lib.check(lib.mmc_trainer_evaluate_set_q32(clf._h, fs._handle(), 0, len(fs), C.byref(nc), C.byref(q), None))
show("evaluate set: correct, loss q32", digest(np.int64(nc.value), np.int64(q.value)))
cal = calibrate(clf, fs)
show("calibrate set: Platt a, b", digest(cal.a_, cal.b_))
fs.close()

# the loss stage alone, weighted, plain and with every option: 203 rows of logits made from the fixture's columns
for K in (3, 130):
    z = np.ascontiguousarray(np.tile(X[:203], (1, 3))[:, :K] * np.float32(4.0) - np.float32(2.0))
    yi = np.ascontiguousarray((fx["y_idx"][:203] * 19 % K).astype(np.int32))
    w = np.ascontiguousarray(np.resize(fx["class_weight"], K))
    pk = np.ascontiguousarray((0.7 * np.log(np.random.default_rng(K).dirichlet(np.ones(K)))).astype(np.float32))
    h = C.c_void_p()
    W0, b0 = [np.zeros((K, 4), np.float32)], [np.zeros(K, np.float32)]
    _lib.check(lib.mmc_trainer_create(_ptr_array(W0), _ptr_array(b0), (C.c_int * 2)(4, K), 1, 1e-3, 0.9, 0.999, 1e-8, 1e-3,
                                      w.ctypes.data_as(C.POINTER(C.c_float)), 0, C.byref(h)))
    for kind, (eps, gamma, p) in {"plain": (0.0, 0.0, None), "all": (0.1, 2.0, pk)}.items():
        _lib.check(lib.mmc_trainer_set_loss(h, eps, gamma, None if p is None else p.ctypes.data_as(C.POINTER(C.c_float))))
        d, rl = np.full(z.shape, np.nan, np.float32), np.full(len(yi), np.nan, np.float32)
        _lib.check(lib.mmc_trainer_loss_gradient(h, z.ctypes.data, yi.ctypes.data, len(yi), d.ctypes.data, rl.ctypes.data, None))
        show(f"loss gradient K {K} weighted {kind}", digest(d, rl))
    lib.mmc_trainer_destroy(h)
