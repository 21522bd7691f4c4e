#!/usr/bin/env python3
"""GPU box: one sha256 line per case over everything a trainer entry point computes, to compare two builds of the library bit for
bit (run it on both checkouts in one visit; the two outputs must be identical line for line: profiles/solo_as_group_bits.txt).

A training case hashes the parameters, both Adam moments, the step count and loss_curve_, and on an "extras" line what its options
keep beside them (the raw parameters, grad_norms_, the averaged weights, log q, the batch-normalisation state and the folded
parameters); the other cases hash the raw bytes of the outputs they name.  The cases: host-fed and resident passes of one
classifier, every loss, regulariser, optimiser, group-robust, taxonomy, normalisation and distillation option on its own, two grouped
passes of heterogeneous members, the eval-mode forward, and the six probes -- all on the 730 x 64 rows of tests/golden/trainer_fixture.npz.
Seconds in all.

    python tools/trainer_bits.py [--grouped-only]     (--grouped-only: the two grouped passes alone, for a kernel trace)"""
import ctypes as C
import hashlib
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from mermaid_classifier_amd import FeatureSet, TargetSet, _lib, calibrate  # noqa: E402
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
    print(f"{name:52s} {value}", flush=True)


N, K = len(X), len(classes)
ROW_W = (0.5 + (np.arange(N) % 7) / 4.0).astype(np.float32)
ROW_G = (np.arange(N) * 3 % 5).astype(np.int32)
LEVELS = {c: [i // 4, None if i % 5 == 0 else i // 2] for i, c in enumerate(classes)}
SOFT = {c: {c: 0.75, classes[(i + 1) % K]: 0.25} for i, c in enumerate(classes)}
fp = C.POINTER(C.c_float)
# per-row targets from the fixture's columns: a softmax in double, stored as float32 (rows sum to 1 within rounding)
_T = np.tile(X, (1, 3))[:, :K].astype(np.float64) * 3.0
TARGETS = np.exp(_T - _T.max(axis=1, keepdims=True))
TARGETS = np.ascontiguousarray((TARGETS / TARGETS.sum(axis=1, keepdims=True)).astype(np.float32))


def extras(clf):
    """What the options of `clf` keep beside the parameters that evaluation reads and the moments: hashed after state(clf)."""
    out = [a for part in clf.raw_parameters() for a in part]
    if clf.max_grad_norm is not None:
        out.append(clf.grad_norms_)
    if clf.ema_decay:
        out += [a for part in clf.averaged_parameters() for a in part]
    if clf.n_groups is not None:
        out.append(clf._group_logq)
    if clf.batch_norm:
        arrays = clf._bn_arrays()
        _lib.check(lib.mmc_trainer_batch_norm_state(clf._h, 0, *[_ptr_array(a) for a in arrays]))
        out += [a for part in arrays for a in part] + [a for part in clf.folded_parameters() for a in part]
    return digest(*out)


def grouped_passes():
    """Two grouped passes of heterogeneous members: between them every loss kernel, both Adam kernels, both dropout GEMMs, the
    clipping norm, group DRO and batch normalisation in the launches of one step.  No entry point takes row arrays and a mixing
    plan, so the mixed members train in a group of their own."""
    from mermaid_classifier_amd.sweep import partial_fit_rows_group
    fs = FeatureSet(64, classes, reserve=730).append(X, y)
    weighted = [(clf_of((48, 32), weighted=True, batch_size=200), None, None, None),
                (clf_of((70,), max_grad_norm=0.5, batch_size=64), np.arange(729, -1, -2), ROW_W, None),
                (clf_of((33, 17), weighted=True, n_groups=5, group_dro_eta=0.5, batch_size=100), None, ROW_W, ROW_G),
                (clf_of((40,), class_levels=LEVELS, level_weights=[1.0, 0.5], ema_decay=0.9, batch_size=128), None, None, None),
                (clf_of((), weighted=True, soft_targets=SOFT, batch_size="auto"), np.arange(0, 97 * 7, 7), ROW_W, None),
                (clf_of((33, 17, 9), batch_norm=True, max_grad_norm=1.0, batch_size=730), None, None, None),
                (clf_of((48,), batch_norm=True, label_smoothing=0.1, batch_size=64), None, None, None),
                (clf_of((48, 32), dropout=0.3, input_dropout=0.1, regularizer_seed=7, shuffle=False), None, None, None)]
    mixed = [(clf_of((48, 32), weighted=True, mixup_alpha=0.4, regularizer_seed=11, batch_size=64), None, None, None),
             (clf_of((70,), focal_gamma=2.0, batch_size=200), np.arange(729, -1, -2), None, None),
             (clf_of((33, 17), mixup_alpha=0.2, dropout=0.2, regularizer_seed=3, max_grad_norm=0.5, ema_decay=0.9), None, None, None)]
    for name, members in (("weighted", weighted), ("mixed", mixed)):
        arrays = {} if name == "mixed" else dict(row_weight=[m[2] for m in members], row_group=[m[3] for m in members])
        for _ in range(2):
            partial_fit_rows_group([m[0] for m in members], fs, [m[1] for m in members], classes=classes.tolist(), **arrays)
        for i, m in enumerate(members):
            show(f"grouped {name} pass member {i} x2", state(m[0]))
            show(f"grouped {name} pass member {i} x2, extras", extras(m[0]))
    fs.close()


if "--grouped-only" in sys.argv:
    grouped_passes()
    sys.exit(0)


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

# ---- the per-trainer and per-pass options, one resident pass each (x2: the second pass starts from a moved state) -----------------
OPTIONS = {
    "dropout hidden + input": (dict(dropout=0.3, input_dropout=0.1, regularizer_seed=7), {}),
    "mixed pass": (dict(mixup_alpha=0.4, regularizer_seed=11, batch_size=64), {}),
    "schedule + clip + ema": (dict(lr_schedule="cosine", warmup_steps=2, schedule_steps=12, final_lr_ratio=0.1, max_grad_norm=0.5,
                                   ema_decay=0.9, batch_size=128), {}),
    "row weights": ({}, dict(row_weight=ROW_W)),
    "row weights + group DRO": (dict(n_groups=5, group_dro_eta=0.5), dict(row_weight=ROW_W, row_group=ROW_G)),
    "hierarchy levels": (dict(class_levels=LEVELS, level_weights=[1.0, 0.5]), {}),
    "soft targets": (dict(soft_targets=SOFT), {}),
    "batch norm": (dict(batch_norm=True, hidden_layer_sizes=(48, 32)), {}),
}
fs = FeatureSet(64, classes, reserve=730).append(X, y)
ts = TargetSet(classes, reserve_rows=730).append(TARGETS)
OPTIONS["distillation"] = (dict(distill_alpha=0.5), dict(targets=ts))
OPTIONS["distillation tau 2 + row weights + group DRO"] = (dict(distill_alpha=0.7, distill_temperature=2.0, n_groups=5, group_dro_eta=0.5),
                                                           dict(targets=ts, row_weight=ROW_W, row_group=ROW_G))
for name, (opts, arrays) in OPTIONS.items():
    clf = clf_of(weighted=True, **opts)
    for _ in range(2):
        clf.partial_fit_rows(fs, None, classes=classes.tolist(), **arrays)
    show(f"resident {name} x2", state(clf))
    show(f"resident {name} x2, extras", extras(clf))
ts.close()
fs.close()
grouped_passes()

# ---- the other probes: the mixed and the weighted loss stage (with and without groups, with and without a hierarchy), the
# batch-normalisation stage with dA
for Kp in (3, 130):
    n = 203
    z = np.ascontiguousarray(np.tile(X[:n], (1, 3))[:, :Kp] * np.float32(4.0) - np.float32(2.0))
    yi = np.ascontiguousarray((fx["y_idx"][:n] * 19 % Kp).astype(np.int32))
    y2 = np.ascontiguousarray((fx["y_idx"][:n] * 7 % Kp).astype(np.int32))
    w = np.ascontiguousarray(np.resize(fx["class_weight"], Kp))
    rw, rg, G = np.ascontiguousarray(ROW_W[:n]), np.ascontiguousarray(ROW_G[:n]), 5
    logq = np.log(np.arange(1, G + 1) / 15.0)
    ids = np.ascontiguousarray(np.stack([np.arange(Kp) // 4, np.where(np.arange(Kp) % 5 == 0, -1, np.arange(Kp) // 2)]).astype(np.int32))
    lamv = np.array([1.0, 0.5], np.float64)
    h = C.c_void_p()
    W0, b0 = [np.zeros((Kp, 4), np.float32)], [np.zeros(Kp, np.float32)]
    _lib.check(lib.mmc_trainer_create(_ptr_array(W0), _ptr_array(b0), (C.c_int * 2)(4, Kp), 1, 1e-3, 0.9, 0.999, 1e-8, 1e-3,
                                      w.ctypes.data_as(fp), 0, C.byref(h)))
    for hier in (False, True):
        tag = f"K {Kp}{' hierarchy' if hier else ''}"
        if hier:
            _lib.check(lib.mmc_trainer_set_hierarchy(h, 2, ids.ctypes.data, lamv.ctypes.data, None))
            d, rl = np.full(z.shape, np.nan, np.float32), np.full(n, np.nan, np.float32)
            _lib.check(lib.mmc_trainer_loss_gradient(h, z.ctypes.data, yi.ctypes.data, n, d.ctypes.data, rl.ctypes.data, None))
            show(f"loss gradient {tag}", digest(d, rl))
        else:
            d, rl = np.full(z.shape, np.nan, np.float32), np.full(n, np.nan, np.float32)
            _lib.check(lib.mmc_trainer_loss_gradient_mixed(h, z.ctypes.data, yi.ctypes.data, y2.ctypes.data, 0.3, n, d.ctypes.data,
                                                           rl.ctypes.data, None))
            show(f"loss gradient mixed {tag}", digest(d, rl))
        for kind, (a_w, a_g) in {"no arrays": (None, None), "weights": (rw, None), "weights + groups": (rw, rg), "groups": (None, rg)}.items():
            d, rl = np.full(z.shape, np.nan, np.float32), np.full(n, np.nan, np.float32)
            lq, gl = np.full(G, np.nan), np.full(G, np.nan)
            _lib.check(lib.mmc_trainer_loss_gradient_weighted(
                h, z.ctypes.data, yi.ctypes.data, None if a_w is None else a_w.ctypes.data, None if a_g is None else a_g.ctypes.data,
                logq.ctypes.data, 0.7, G, n, d.ctypes.data, rl.ctypes.data, lq.ctypes.data, gl.ctypes.data, None))
            show(f"loss gradient weighted {tag} {kind}", digest(d, rl, lq, gl))
    _lib.check(lib.mmc_trainer_set_hierarchy(h, 0, None, None, None))
    qk = np.exp(z.astype(np.float64) * 0.5)
    qk = np.ascontiguousarray((qk / qk.sum(axis=1, keepdims=True)).astype(np.float32))
    for alpha, tau in ((0.5, 1.0), (0.5, 2.0)):
        _lib.check(lib.mmc_trainer_set_distillation(h, alpha, tau))
        d, rl = np.full(z.shape, np.nan, np.float32), np.full(n, np.nan, np.float32)
        _lib.check(lib.mmc_trainer_loss_gradient_distill(h, z.ctypes.data, yi.ctypes.data, qk.ctypes.data, rw.ctypes.data, n, d.ctypes.data,
                                                         rl.ctypes.data, None))
        show(f"loss gradient distill K {Kp} tau {tau:g} weights", digest(d, rl))
        d, rl, lq, gl = np.full(z.shape, np.nan, np.float32), np.full(n, np.nan, np.float32), np.full(G, np.nan), np.full(G, np.nan)
        _lib.check(lib.mmc_trainer_loss_gradient_distill_weighted(h, z.ctypes.data, yi.ctypes.data, qk.ctypes.data, rw.ctypes.data,
                                                                  rg.ctypes.data, logq.ctypes.data, 0.7, G, n, d.ctypes.data, rl.ctypes.data,
                                                                  lq.ctypes.data, gl.ctypes.data, None))
        show(f"loss gradient distill K {Kp} tau {tau:g} weights + groups", digest(d, rl, lq, gl))
    lib.mmc_trainer_destroy(h)

for width, rows in ((24, 203), (130, 50)):
    h = C.c_void_p()
    Wn = [np.zeros((width, 4), np.float32), np.zeros((3, width), np.float32)]
    bn_ = [np.zeros(width, np.float32), np.zeros(3, np.float32)]
    _lib.check(lib.mmc_trainer_create(_ptr_array(Wn), _ptr_array(bn_), (C.c_int * 3)(4, width, 3), 2, 1e-3, 0.9, 0.999, 1e-8, 1e-3,
                                      None, 0, C.byref(h)))
    _lib.check(lib.mmc_trainer_set_batch_norm(h, 1, 1e-5, 0.1))
    Z = np.ascontiguousarray(np.tile(X[:rows], (1, 3))[:, :width] * np.float32(4.0) - np.float32(2.0))
    dA = np.ascontiguousarray(np.tile(X[100:100 + rows], (1, 3))[:, 5:5 + width] - np.float32(0.5))
    for with_dA in (False, True):
        H, dZ = np.full(Z.shape, np.nan, np.float32), np.full(Z.shape, np.nan, np.float32)
        gg, gb, mu, var = (np.full(width, np.nan, np.float32) for _ in range(4))
        _lib.check(lib.mmc_trainer_norm_stage(h, 0, Z.ctypes.data, dA.ctypes.data if with_dA else None, rows, H.ctypes.data, dZ.ctypes.data,
                                              gg.ctypes.data, gb.ctypes.data, mu.ctypes.data, var.ctypes.data, None))
        show(f"norm stage width {width} rows {rows}{' with dA' if with_dA else ''}", digest(H, dZ, gg, gb, mu, var))
    lib.mmc_trainer_destroy(h)
