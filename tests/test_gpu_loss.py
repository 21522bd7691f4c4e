"""Loss formulations of the MLP trainer on the device: label smoothing, focal loss, logit prior (``mmc_trainer_set_loss``).

``mmc_trainer_loss_gradient`` per element against the fp64 checker within the bounds of tests/loss_checker.py (128 units of
2^-24 g w_max on ``dlogits``, 96 units of 2^-24 (|l_i g| + g w_max) on ``row_loss``; tests/test_loss_host.py shows an fp32
evaluation in the kernel's order stays within half of them and wrong kernels miss them by orders of magnitude).  Training against a
torch-CPU fp32 loop within the tolerances of tests/test_trainer.py for this kind of comparison (weights 2e-5, loss curve 1e-5).
Everything else is bit equality: host-fed against resident rows, grouped against solo, pickled twin against original, a rejected or
a default ``mmc_trainer_set_loss`` against none."""

import ctypes as C
import pickle

import numpy as np
import pytest

import loss_checker as lc

pytestmark = pytest.mark.gpu

W_TOL, LOSS_TOL = 2e-5, 1e-5          # tests/test_trainer.py
K7, NF, N = 7, 16, 230


# ---- raw trainers through the C ABI -------------------------------------------------------------------------------------------
class _Raw:
    """An ``mmc_trainer`` made by ``mmc_trainer_create`` alone: nothing has called ``mmc_trainer_set_loss`` on it."""

    def __init__(self, weights, biases, class_weight=None, lr=1e-3, alpha=1e-3):
        from mermaid_classifier_amd import _lib
        from mermaid_classifier_amd.torch_classifier import _ptr_array
        self.lib, self._lib = _lib.lib(), _lib
        self.shapes = [w.shape for w in weights]
        dims = [weights[0].shape[1]] + [w.shape[0] for w in weights]
        self.K = dims[-1]
        self.h = C.c_void_p()
        cw = None if class_weight is None else np.ascontiguousarray(class_weight, np.float32)
        _lib.check(self.lib.mmc_trainer_create(_ptr_array(weights), _ptr_array(biases), (C.c_int * len(dims))(*dims), len(weights),
                                               lr, 0.9, 0.999, 1e-8, alpha,
                                               None if cw is None else cw.ctypes.data_as(C.POINTER(C.c_float)), 0, C.byref(self.h)))

    def set_loss(self, eps=0.0, gamma=0.0, prior=None):
        p = None if prior is None else np.ascontiguousarray(prior, np.float32)
        return self.lib.mmc_trainer_set_loss(self.h, float(eps), float(gamma), None if p is None else p.ctypes.data_as(C.POINTER(C.c_float)))

    def loss_gradient(self, z, y):
        z = np.ascontiguousarray(z, np.float32)
        y32 = np.ascontiguousarray(y, np.int32)
        d, l = np.full(z.shape, np.nan, np.float32), np.full(len(y32), np.nan, np.float32)
        status = self.lib.mmc_trainer_loss_gradient(self.h, z.ctypes.data, y32.ctypes.data, len(y32), d.ctypes.data, l.ctypes.data, None)
        return status, d, l

    def partial_fit(self, X, y, batch_size):
        avg = C.c_double(0.0)
        X, y32 = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(y, np.int32)
        self._lib.check(self.lib.mmc_trainer_partial_fit(self.h, X.ctypes.data, y32.ctypes.data, len(y32), batch_size, C.byref(avg), None))
        return avg.value

    def state(self):
        from mermaid_classifier_amd.torch_classifier import _ptr_array
        out = []
        ws, bs = [np.empty(s, np.float32) for s in self.shapes], [np.empty(s[0], np.float32) for s in self.shapes]
        self._lib.check(self.lib.mmc_trainer_get_params(self.h, _ptr_array(ws), _ptr_array(bs)))
        out += ws + bs
        step = C.c_longlong(0)
        for which in (0, 1):
            ws, bs = [np.empty(s, np.float32) for s in self.shapes], [np.empty(s[0], np.float32) for s in self.shapes]
            self._lib.check(self.lib.mmc_trainer_adam_state(self.h, which, 0, _ptr_array(ws), _ptr_array(bs), C.byref(step)))
            out += ws + bs
        return out, int(step.value)

    def close(self):
        self.lib.mmc_trainer_destroy(self.h)


def _same_raw(a, b):
    (pa, sa), (pb, sb) = a, b
    return sa == sb and len(pa) == len(pb) and all(np.array_equal(u, v) for u, v in zip(pa, pb))


# ---- 3. the loss stage per element ----------------------------------------------------------------------------------------------
def _kinds(prior):
    return [("plain", dict()), ("smoothing", dict(eps=0.1)), ("focal", dict(gamma=2.0)), ("prior", dict(prior=prior)),
            ("all", dict(eps=0.3, gamma=5.0, prior=prior))]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [3, 65, 108, 130])
def test_loss_gradient_per_element_against_the_fp64_checker(K, weighted):
    rng = np.random.default_rng([K, int(weighted)])
    w = lc.class_weights(rng, K) if weighted else None
    prior = lc.dirichlet_prior(rng, K)
    z, y = lc.logit_rows(rng, 203, K, 4.0)          # 203 rows: the last workgroup holds three; the four special rows included
    live = 0 if w is None else int(np.flatnonzero(w > 0)[0])
    z1, y1 = lc.logit_rows(rng, 1, K, 4.0)[0], np.array([live])
    raw = _Raw([np.zeros((K, 4), np.float32)], [np.zeros(K, np.float32)], class_weight=w)
    try:
        for kind, opts in _kinds(prior):
            assert raw.set_loss(**opts) == 0, kind
            for zz, yy in ((z, y), (z1, y1)):
                status, d, l = raw.loss_gradient(zz, yy)
                assert status == 0, raw.lib.mmc_last_error()
                assert np.isfinite(d).all() and np.isfinite(l).all()
                grad, rows, _, _ = lc.checker(zz, yy, w, **opts)
                bd, bl = lc.bounds(yy, w, rows)
                ed, el = float(np.abs(d - grad).max() / bd), float((np.abs(l - rows) / bl).max())
                print(f"K {K} weighted {weighted} {kind:9s} n {len(yy):3d}: dlogits {ed * lc.DLOGITS_UNITS:6.1f} of {lc.DLOGITS_UNITS:.0f} "
                      f"units, row_loss {el * lc.ROW_LOSS_UNITS:6.1f} of {lc.ROW_LOSS_UNITS:.0f} units")
                assert ed <= 1.0 and el <= 1.0, (kind, len(yy), ed, el)
        # what the entry point refuses launches nothing and says why
        from mermaid_classifier_amd import _lib
        bad = y.copy()
        bad[7] = K
        assert raw.loss_gradient(z, bad)[0] == _lib.MMC_ERR_ARG and b"y[7]" in raw.lib.mmc_last_error()
        if weighted:
            dead = np.full(5, int(np.flatnonzero(w == 0)[0]))
            assert raw.loss_gradient(z[:5], dead)[0] == _lib.MMC_ERR_ARG and b"zero total class weight" in raw.lib.mmc_last_error()
    finally:
        raw.close()


# ---- 4. training parity against torch on the CPU ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(17)
    y = rng.integers(0, K7, size=N)
    centres = rng.normal(0, 1.0, (K7, NF))
    X = (centres[y] + rng.normal(0, 1.0, (N, NF))).astype(np.float32)
    w = np.array([1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.75], np.float32)
    counts = np.bincount(y, minlength=K7)
    prior = {k: float(np.log(c / N)) for k, c in enumerate(counts)}
    return dict(X=X, y=y, w=w, cw={k: float(v) for k, v in enumerate(w)}, prior=prior)


_TRAIN_KINDS = {"smoothing": dict(label_smoothing=0.1, weighted=True), "focal": dict(focal_gamma=2.0, weighted=True),
                "prior": dict(use_prior=True, weighted=False), "all": dict(label_smoothing=0.3, focal_gamma=5.0, use_prior=True, weighted=True)}


def _make(data, hidden=(24, 12), label_smoothing=0.0, focal_gamma=0.0, use_prior=False, weighted=False, **kw):
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    args = dict(hidden_layer_sizes=hidden, learning_rate_init=1e-3, alpha=1e-3, random_state=0, batch_size=50,
                class_weight=data["cw"] if weighted else None, label_smoothing=label_smoothing, focal_gamma=focal_gamma,
                logit_prior=data["prior"] if use_prior else None)
    args.update(kw)
    return TorchMLPClassifier(**args)


def _torch_loop(data, clf, passes):
    """The reference's mini-batch loop in torch on the CPU, fp32: same initial parameters and visiting order, torch.optim.Adam, the
    L2 term (0.5 alpha / mb) sum W^2; the loss is F.cross_entropy itself where torch has it, autograd of the definition otherwise."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    clf.classes_, clf.n_features_in_ = np.arange(K7), NF
    w0, b0 = clf._initial_parameters()
    del clf.classes_, clf.n_features_in_
    layers = [nn.Linear(w.shape[1], w.shape[0]) for w in w0]
    with torch.no_grad():
        for m, w, b in zip(layers, w0, b0):
            m.weight.copy_(torch.from_numpy(w))
            m.bias.copy_(torch.from_numpy(b))
    params = [p for m in layers for p in (m.weight, m.bias)]
    opt = torch.optim.Adam(params, lr=clf.learning_rate_init, betas=(clf.beta_1, clf.beta_2), eps=clf.epsilon)
    wt = torch.from_numpy(data["w"]) if clf.class_weight is not None else None
    prior = None if clf.logit_prior is None else torch.tensor([clf.logit_prior[k] for k in range(K7)], dtype=torch.float32)
    eps, gamma = float(clf.label_smoothing), float(clf.focal_gamma)

    def data_loss(logits, yb):
        if gamma == 0.0 and prior is None:
            return F.cross_entropy(logits, yb, weight=wt, label_smoothing=eps)
        u = logits if prior is None else logits + prior
        logp = torch.log_softmax(u, dim=1)
        logpt = logp.gather(1, yb[:, None])[:, 0]
        w = torch.ones(K7) if wt is None else wt
        m = (1.0 - torch.exp(logpt)) ** gamma if gamma != 0.0 else torch.ones_like(logpt)
        l = (1.0 - eps) * w[yb] * m * -logpt + (eps / K7) * -(logp * w).sum(dim=1)
        return l.sum() / w[yb].sum()

    order = np.arange(N)
    np.random.default_rng(0).shuffle(order)                     # the classifier's shuffle: a fresh generator per pass
    Xo, yo = torch.from_numpy(data["X"][order]), torch.from_numpy(data["y"][order].astype(np.int64))
    curve = []
    for _ in range(passes):
        total = 0.0
        for start in range(0, N, 50):
            xb, yb = Xo[start:start + 50], yo[start:start + 50]
            opt.zero_grad()
            h = xb
            for i, m in enumerate(layers):
                h = m(h)
                if i < len(layers) - 1:
                    h = torch.relu(h)
            loss = data_loss(h, yb) + (0.5 * clf.alpha / len(yb)) * sum((m.weight ** 2).sum() for m in layers)
            loss.backward()
            opt.step()
            total += loss.item() * len(yb)
        curve.append(total / N)
    return curve, [m.weight.detach().numpy() for m in layers], [m.bias.detach().numpy() for m in layers]


def _state(clf):
    s = clf._adam_state()
    return ([a.copy() for part in clf.parameters() for a in part], [a.copy() for part in s["exp_avg"] for a in part],
            [a.copy() for part in s["exp_avg_sq"] for a in part], s["step"], list(clf.loss_curve_), clf.n_iter_)


def _assert_same_state(a, b):
    sa, sb = (x if isinstance(x, tuple) else _state(x) for x in (a, b))
    for u, v in zip(sa[:3], sb[:3]):
        assert len(u) == len(v)
        for p, q in zip(u, v):
            assert np.array_equal(p, q)
    assert sa[3:] == sb[3:]


@pytest.mark.parametrize("kind", list(_TRAIN_KINDS))
def test_training_matches_torch_on_both_routes(data, kind):
    from mermaid_classifier_amd import FeatureSet
    want_curve, want_w, want_b = _torch_loop(data, _make(data, **_TRAIN_KINDS[kind]), 3)
    host, resident = _make(data, **_TRAIN_KINDS[kind]), _make(data, **_TRAIN_KINDS[kind])
    fs = FeatureSet(NF, np.arange(K7)).append(data["X"], data["y"])
    for _ in range(3):
        host.partial_fit(data["X"], data["y"], classes=list(range(K7)))
        resident.partial_fit_rows(fs, classes=list(range(K7)))
    fs.close()
    print(kind, "loss curve", host.loss_curve_, "torch", want_curve)
    np.testing.assert_allclose(host.loss_curve_, want_curve, rtol=0, atol=LOSS_TOL)
    ws, bs = host.parameters()
    for i in range(3):
        dw, db = np.abs(ws[i] - want_w[i]).max(), np.abs(bs[i] - want_b[i]).max()
        print(f"layer {i}: max|dW| {dw:.2e} max|db| {db:.2e}")
        assert dw <= W_TOL and db <= W_TOL
    assert host._adam_state()["step"] == 15                     # 50, 50, 50, 50, 30 rows: the last mini-batch is ragged
    _assert_same_state(host, resident)
    # the options shape training alone: the probabilities are those of the raw logits
    logits = np.asarray(data["X"][:9]) @ ws[0].T + bs[0]
    for w, b in zip(ws[1:], bs[1:]):
        logits = np.maximum(logits, 0) @ w.T + b
    p = np.exp(logits - logits.max(axis=1, keepdims=True))
    assert np.abs(host.predict_proba(data["X"][:9]) - p / p.sum(axis=1, keepdims=True)).max() < 1e-5


# ---- 5. grouped equals solo -----------------------------------------------------------------------------------------------------
def _mixed_members(data):
    """Five members of different depth, one per kind, plain among them: a group's kernel switches instantiation per member."""
    return [_make(data, ()), _make(data, (24,), **_TRAIN_KINDS["smoothing"]), _make(data, (24, 12), **_TRAIN_KINDS["focal"]),
            _make(data, (20, 10, 5), batch_size=64, **_TRAIN_KINDS["prior"]), _make(data, (24, 12), random_state=3, **_TRAIN_KINDS["all"])]


def test_mixed_group_has_the_bits_of_the_solo_passes(data):
    from mermaid_classifier_amd import FeatureSet, partial_fit_rows_group
    fs = FeatureSet(NF, np.arange(K7)).append(data["X"], data["y"])
    group, solo = _mixed_members(data), _mixed_members(data)
    for _ in range(2):
        partial_fit_rows_group(group, fs, classes=list(range(K7)))
        for clf in solo:
            clf.partial_fit_rows(fs, classes=list(range(K7)))
    for a, b in zip(group, solo):
        _assert_same_state(a, b)
    assert [c._adam_state()["step"] for c in group] == [10, 10, 10, 8, 10]
    assert len({tuple(c.loss_curve_) for c in group}) == 5
    fs.close()


# ---- 6. state ---------------------------------------------------------------------------------------------------------------------
def test_pickled_twin_carries_the_loss_options(data):
    clf = _make(data, **_TRAIN_KINDS["all"])
    plain = _make(data, weighted=True)
    for c in (clf, plain):
        c.partial_fit(data["X"], data["y"], classes=list(range(K7)))
    assert clf.loss_curve_ != plain.loss_curve_
    twin = pickle.loads(pickle.dumps(clf))
    assert twin.get_params() == clf.get_params()
    clf.partial_fit(data["X"], data["y"])
    twin.partial_fit(data["X"], data["y"])
    _assert_same_state(clf, twin)


def test_set_loss_rejected_or_default_changes_no_bits(data):
    from mermaid_classifier_amd import _lib
    clf = _make(data)
    clf.classes_, clf.n_features_in_ = np.arange(K7), NF
    w0, b0 = clf._initial_parameters()
    X, y = data["X"], data["y"]
    prior = np.array([data["prior"][k] for k in range(K7)], np.float32)
    mk = lambda: _Raw(w0, b0, class_weight=data["w"])
    untouched, default, restored, general, rejected = mk(), mk(), mk(), mk(), mk()
    try:
        assert default.set_loss(0.0, 0.0, None) == 0
        assert restored.set_loss(0.3, 5.0, prior) == 0 and restored.set_loss(0.0, 0.0, None) == 0
        assert general.set_loss(0.3, 5.0, prior) == 0 and rejected.set_loss(0.3, 5.0, prior) == 0
        curves = [[t.partial_fit(X, y, 50)] for t in (untouched, default, restored, general, rejected)]
        nan_prior = prior.copy()
        nan_prior[2] = np.nan
        for args in ((1.0, 0.0, None), (0.1, 0.5, None), (0.0, 9.0, prior), (0.1, 2.0, nan_prior), (-0.1, 0.0, None)):
            assert rejected.set_loss(*args) == _lib.MMC_ERR_ARG
        for t, c in zip((untouched, default, restored, general, rejected), curves):
            c.append(t.partial_fit(X, y, 50))
        assert curves[0] == curves[1] == curves[2] and curves[3] == curves[4] and curves[0] != curves[3]
        assert _same_raw(untouched.state(), default.state()) and _same_raw(untouched.state(), restored.state())
        assert _same_raw(general.state(), rejected.state()) and not _same_raw(untouched.state(), general.state())
    finally:
        for t in (untouched, default, restored, general, rejected):
            t.close()


# ---- 7. a sweep over formulations -------------------------------------------------------------------------------------------------
def test_train_sweep_with_loss_options_equals_train_classifier(data):
    from mermaid_classifier_amd import FeatureSet, SweepConfig, class_counts, logit_adjustment, train_classifier, train_sweep
    X, y = data["X"], data["y"]
    sets = [FeatureSet(NF, np.arange(K7)).append(X[s], y[s]) for s in (slice(0, 130), slice(130, 180), slice(180, 230))]
    counts = class_counts(sets[0])
    assert counts.min() >= 1
    prior = logit_adjustment({k: int(c) for k, c in enumerate(counts)})
    base = dict(hidden_layer_sizes=(24, 12), learning_rate_init=3e-3, alpha=1e-3, random_state=0, batch_size=50)
    configs = [SweepConfig(**base), SweepConfig(**base, label_smoothing=0.1, logit_prior=prior)]
    got = train_sweep(*sets, configs, 4, batch_size=70, early_stopping_patience=2)
    for i, cfg in enumerate(configs):
        cal, info, ref_accs = train_classifier(*sets, 4, batch_size=70, early_stopping_patience=2, clf=cfg.classifier(sets[1].device))
        mine, my_info, my_accs = got[i]
        assert my_info == info and my_accs == ref_accs
        for u, v in zip(mine.weights + mine.biases, cal.weights + cal.biases):
            assert np.array_equal(u, v)
        assert np.array_equal(mine.a_, cal.a_) and np.array_equal(mine.b_, cal.b_)
    assert not all(np.array_equal(u, v) for u, v in zip(got[0][0].weights, got[1][0].weights))
    for s in sets:
        s.close()
