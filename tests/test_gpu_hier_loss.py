"""The taxonomy-aware loss on the device: level-marginal terms and soft labels (``mmc_trainer_set_hierarchy``).

``mmc_trainer_loss_gradient`` and ``mmc_trainer_loss_gradient_weighted`` per element against the fp64 checker within the bounds of
tests/hier_loss_checker.py (derived there from ``ce_grad_rows_hier``'s operation count; tests/test_hier_loss_host.py shows an fp32
evaluation in the kernel's order stays within half of them and wrong kernels miss them by four orders of magnitude).  Training against
a torch-CPU fp32 loop within the tolerances of tests/test_trainer.py for this kind of comparison (weights 2e-5, loss curve 1e-5).
Everything else is bit equality: host-fed against resident rows, grouped against solo, one chunk size against another, pickled twin
against original, a rejected, a default or a restored ``mmc_trainer_set_hierarchy`` against none."""

import ctypes as C
import pickle

import numpy as np
import pytest

import hier_loss_checker as hc
import loss_checker as lc

pytestmark = pytest.mark.gpu

W_TOL, LOSS_TOL = 2e-5, 1e-5          # tests/test_trainer.py
K7, NF, N = 7, 16, 230                # the data of tests/test_gpu_loss.py
LAM4 = [1.5, 0.5, 2.0, 0.25]


# ---- raw trainers through the C ABI -------------------------------------------------------------------------------------------
def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


class _Raw:
    """An ``mmc_trainer`` made by ``mmc_trainer_create`` alone: nothing else has been called on it."""

    def __init__(self, weights, biases, class_weight=None, lr=1e-3, alpha=1e-3):
        from mermaid_classifier_amd import _lib
        from mermaid_classifier_amd.torch_classifier import _ptr_array
        self.lib, self._lib = _lib.lib(), _lib
        self.shapes = [w.shape for w in weights]
        dims = [weights[0].shape[1]] + [w.shape[0] for w in weights]
        self.K = dims[-1]
        self.h = C.c_void_p()
        cw = _f32(class_weight)
        _lib.check(self.lib.mmc_trainer_create(_ptr_array(weights), _ptr_array(biases), (C.c_int * len(dims))(*dims), len(weights),
                                               lr, 0.9, 0.999, 1e-8, alpha,
                                               None if cw is None else cw.ctypes.data_as(C.POINTER(C.c_float)), 0, C.byref(self.h)))

    def set_loss(self, eps=0.0, gamma=0.0, prior=None):
        p = _f32(prior)
        return self.lib.mmc_trainer_set_loss(self.h, float(eps), float(gamma), None if p is None else p.ctypes.data_as(C.POINTER(C.c_float)))

    def set_hierarchy(self, levels=None, lam=None, T=None, n_levels=None):
        ids = None if levels is None else np.ascontiguousarray(levels, np.int32)
        wl = None if lam is None else np.ascontiguousarray(lam, np.float64)
        Tm = _f32(T)
        n = (0 if ids is None else len(ids)) if n_levels is None else n_levels
        return self.lib.mmc_trainer_set_hierarchy(self.h, n, None if ids is None else ids.ctypes.data, None if wl is None else wl.ctypes.data,
                                                  None if Tm is None else Tm.ctypes.data)

    def loss_gradient(self, z, y):
        z, y32 = _f32(z), np.ascontiguousarray(y, np.int32)
        d, l = np.full(z.shape, np.nan, np.float32), np.full(len(y32), np.nan, np.float32)
        status = self.lib.mmc_trainer_loss_gradient(self.h, z.ctypes.data, y32.ctypes.data, len(y32), d.ctypes.data, l.ctypes.data, None)
        return status, d, l

    def loss_gradient_weighted(self, z, y, r=None, a=None, logq=None, eta=0.0, G=0):
        z, y32, r32 = _f32(z), np.ascontiguousarray(y, np.int32), _f32(r)
        a32 = None if a is None else np.ascontiguousarray(a, np.int32)
        d, l = np.full(z.shape, np.nan, np.float32), np.full(len(y32), np.nan, np.float32)
        qi = None if a is None else np.ascontiguousarray(logq, np.float64)
        qo = None if a is None else np.full(G, np.nan)
        status = self.lib.mmc_trainer_loss_gradient_weighted(
            self.h, z.ctypes.data, y32.ctypes.data, None if r32 is None else r32.ctypes.data, None if a32 is None else a32.ctypes.data,
            None if qi is None else qi.ctypes.data, float(eta), int(G), len(y32), d.ctypes.data, l.ctypes.data,
            None if qo is None else qo.ctypes.data, None, None)
        return status, d, l, qo

    def partial_fit(self, X, y, batch_size):
        avg = C.c_double(0.0)
        X, y32 = _f32(X), np.ascontiguousarray(y, np.int32)
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


# ---- 1. the loss stage per element ----------------------------------------------------------------------------------------------
def _peak(err, bound):
    """Peak error over bound; where the bound is 0 (a row of weight zero) the error has to be 0 too."""
    err, bound = np.abs(np.asarray(err, np.float64)), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())


def _kinds(K, prior, T):
    one, four = hc.levels_for(K, 1), hc.levels_for(K, 4)
    return [("one level", dict(levels=one, lam=[1.5])), ("four levels", dict(levels=four, lam=LAM4)), ("T alone", dict(T=T)),
            ("T+levels+prior", dict(levels=four, lam=LAM4, T=T, prior=prior)),
            ("levels on smoothing+focal", dict(levels=four, lam=LAM4, eps=0.1, gamma=2.0))]


def _apply(raw, opts):
    """The options of a kind onto a raw trainer, whichever was set before: back to the defaults first."""
    assert raw.set_hierarchy() == 0 and raw.set_loss() == 0
    assert raw.set_loss(opts.get("eps", 0.0), opts.get("gamma", 0.0), opts.get("prior")) == 0, raw.lib.mmc_last_error()
    assert raw.set_hierarchy(opts.get("levels"), opts.get("lam"), opts.get("T")) == 0, raw.lib.mmc_last_error()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [3, 65, 108, 130])
def test_loss_gradient_per_element_against_the_fp64_checker(K, weighted):
    rng = np.random.default_rng([K, int(weighted), 7])
    w = lc.class_weights(rng, K) if weighted else None
    prior = lc.dirichlet_prior(rng, K)
    T = hc.soft_targets(rng, K)
    bank = hc.level_bank(K)
    z, y = hc.hier_rows(rng, 203, K, 4.0, bank)     # 203 + 2 rows: the last workgroup holds one; every special row included
    assert len(y) == 205 and (bank[3][y] < 0).any() and (K == 3 or (bank[2][y] < 0).any())     # true classes without a node at a level
    if K > 70:
        assert len(set(bank[2][60:71])) == 2 and bank[2][63] == bank[2][65] == 60      # one node on both sides of class 64
    raw = _Raw([np.zeros((K, 4), np.float32)], [np.zeros(K, np.float32)], class_weight=w)
    try:
        for kind, opts in _kinds(K, prior, T):
            _apply(raw, opts)
            status, d, l = raw.loss_gradient(z, y)
            assert status == 0, raw.lib.mmc_last_error()
            assert np.isfinite(d).all() and np.isfinite(l).all()
            grad, rows, _ = hc.checker(z, y, w, **opts)
            bd, bl = hc.bounds(z, y, w, rows, prior=opts.get("prior"), lam=opts.get("lam"))
            ed, el = _peak(d - grad, bd), _peak(l - rows, bl)
            print(f"K {K} weighted {weighted} {kind:26s}: dlogits {ed:.3f} of its bound ({hc.dlogits_units(K, opts.get('lam')):.0f} units), "
                  f"row_loss {el:.3f} of its bound")
            assert ed <= 1.0 and el <= 1.0, (kind, ed, el)
        # the same kernel behind mmc_trainer_loss_gradient_weighted: row weights, then groups
        opts = dict(levels=hc.levels_for(K, 4), lam=LAM4)
        _apply(raw, opts)
        r = rng.uniform(1e-2, 1e2, len(y)).astype(np.float32)
        r[[2, 5]] = 0.0
        status, d, l, _ = raw.loss_gradient_weighted(z, y, r=r)
        assert status == 0, raw.lib.mmc_last_error()
        assert np.isfinite(d).all() and np.isfinite(l).all() and (d[2] == 0).all() and l[5] == 0
        exact = hc.normaliser(y, w, r, exact=True)
        grad, rows, _ = hc.checker(z, y, w, norm=exact, **opts)
        bd, bl = hc.bounds(z, y, w, rows, lam=LAM4, norm=exact)
        ed, el = _peak(d - grad, bd), _peak(l - rows, bl)
        print(f"K {K} weighted {weighted} four levels, row weights  : dlogits {ed:.3f} of its bound, row_loss {el:.3f} of its bound")
        assert ed <= 1.0 and el <= 1.0, (ed, el)
        G, eta = 3, 0.5
        a = rng.integers(0, G, len(y))
        logq = np.log(np.array([0.5, 0.3, 0.2]))
        status, d, l, lq = raw.loss_gradient_weighted(z, y, r=r, a=a, logq=logq, eta=eta, G=G)
        assert status == 0, raw.lib.mmc_last_error()
        assert np.isfinite(d).all() and np.isfinite(l).all() and np.isfinite(lq).all()
        rr = r.astype(np.float64)                                       # with groups the stage's normaliser is r_i itself
        D, R, _ = hc.checker(z, y, w, norm=rr, **opts)
        bD, bR = hc.bounds(z, y, w, R, lam=LAM4, norm=rr)
        v = rr * (1.0 if w is None else w.astype(np.float64)[y])
        ref, bnd = hc.with_groups(D, R, bD, bR, v, a, logq, eta, G)
        ed, el, eq = _peak(d - ref["dlogits"], bnd["dlogits"]), _peak(l - ref["row_loss"], bnd["row_loss"]), _peak(lq - ref["logq"], bnd["logq"])
        print(f"K {K} weighted {weighted} four levels, groups       : dlogits {ed:.3f}, row_loss {el:.3f}, log q {eq:.3f} of their bounds")
        assert ed <= 1.0 and el <= 1.0 and eq <= 1.0, (ed, el, eq)
    finally:
        raw.close()


# ---- 2. training parity against torch on the CPU ----------------------------------------------------------------------------------
PATHS7 = [("hard", "acro"), ("hard", "acro"), ("hard", "pori"), ("sand",), ("soft", "gorg"), ("algae", "turf"), ("algae", "macro")]


@pytest.fixture(scope="module")
def data():
    from mermaid_classifier_amd import hierarchy_levels, soft_labels
    rng = np.random.default_rng(17)
    y = rng.integers(0, K7, size=N)
    centres = rng.normal(0, 1.0, (K7, NF))
    X = (centres[y] + rng.normal(0, 1.0, (N, NF))).astype(np.float32)
    w = np.array([1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.75], np.float32)
    counts = np.bincount(y, minlength=K7)
    prior = {k: float(np.log(c / N)) for k, c in enumerate(counts)}
    levels = hierarchy_levels(PATHS7)                                  # K x 3: depth 1, depth 2, the attribute
    levels[3, 1] = -1                                                  # "sand" has no node at depth 2
    S = np.array([[sum(1 for p, q in zip(a, b) if p == q) / 2.0 for b in PATHS7] for a in PATHS7])
    T = soft_labels(S, 3.0)
    return dict(X=X, y=y, w=w, cw={k: float(v) for k, v in enumerate(w)}, prior=prior, levels=levels, T=T,
                class_levels={k: [None if v < 0 else int(v) for v in levels[k]] for k in range(K7)},
                soft_targets={t: {c: float(T[t, c]) for c in range(K7)} for t in range(K7)})


LAM3 = [1.0, 0.5, 0.25]
_TRAIN_KINDS = {"levels": dict(use_levels=True, weighted=True), "soft": dict(use_T=True, weighted=False),
                "soft+levels+prior": dict(use_levels=True, use_T=True, use_prior=True, weighted=True),
                "levels+smoothing+focal": dict(use_levels=True, label_smoothing=0.1, focal_gamma=2.0, weighted=True)}


def _make(data, hidden=(24, 12), use_levels=False, use_T=False, use_prior=False, weighted=False, **kw):
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    args = dict(hidden_layer_sizes=hidden, learning_rate_init=1e-3, alpha=1e-3, random_state=0, batch_size=50,
                class_weight=data["cw"] if weighted else None, logit_prior=data["prior"] if use_prior else None,
                class_levels=data["class_levels"] if use_levels else None, level_weights=LAM3 if use_levels else None,
                soft_targets=data["soft_targets"] if use_T else None)
    args.update(kw)
    return TorchMLPClassifier(**args)


def _torch_loop(data, clf, passes):
    """The reference's mini-batch loop in torch on the CPU, fp32: same initial parameters and visiting order, torch.optim.Adam, the
    L2 term (0.5 alpha / mb) sum W^2; the loss is autograd of the definition."""
    import torch
    import torch.nn as nn
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
    w = torch.from_numpy(data["w"]) if clf.class_weight is not None else torch.ones(K7)
    prior = None if clf.logit_prior is None else torch.tensor([clf.logit_prior[k] for k in range(K7)], dtype=torch.float32)
    eps, gamma = float(clf.label_smoothing), float(clf.focal_gamma)
    T = None if clf.soft_targets is None else torch.from_numpy(data["T"])
    levels = [] if clf.class_levels is None else [(torch.from_numpy(data["levels"][:, l].astype(np.int64)), float(np.float32(lam)))
                                                  for l, lam in enumerate(clf.level_weights)]

    def data_loss(logits, yb):
        u = logits if prior is None else logits + prior
        logp = torch.log_softmax(u, dim=1)
        if T is None:
            logpt = logp.gather(1, yb[:, None])[:, 0]
            m = (1.0 - torch.exp(logpt)) ** gamma if gamma != 0.0 else torch.ones_like(logpt)
            l = (1.0 - eps) * w[yb] * m * -logpt + (eps / K7) * -(logp * w).sum(dim=1)
        else:
            l = w[yb] * -(T[yb] * logp).sum(dim=1)
        for ids, lam in levels:
            gt = ids[yb]
            has = gt >= 0
            mask = (ids[None, :] == gt[:, None]) | ~has[:, None]
            l = l + w[yb] * lam * has.float() * -torch.logsumexp(logp.masked_fill(~mask, -float("inf")), dim=1)
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
    # the hierarchy shapes training alone: the probabilities are those of the raw logits
    logits = np.asarray(data["X"][:9]) @ ws[0].T + bs[0]
    for w, b in zip(ws[1:], bs[1:]):
        logits = np.maximum(logits, 0) @ w.T + b
    p = np.exp(logits - logits.max(axis=1, keepdims=True))
    assert np.abs(host.predict_proba(data["X"][:9]) - p / p.sum(axis=1, keepdims=True)).max() < 1e-5


# ---- 3. bit equality ------------------------------------------------------------------------------------------------------------------
def _mixed_members(data):
    """Flat, levels, T, levels + group DRO, levels + dropout: members of different depth, one per kind."""
    return [_make(data, ()), _make(data, (24,), **_TRAIN_KINDS["levels"]), _make(data, (24, 12), **_TRAIN_KINDS["soft"]),
            _make(data, (20, 10, 5), batch_size=64, n_groups=3, group_dro_eta=0.5, **_TRAIN_KINDS["levels"]),
            _make(data, (24, 12), random_state=3, dropout=0.2, input_dropout=0.1, **_TRAIN_KINDS["soft+levels+prior"])]


def test_mixed_group_has_the_bits_of_the_solo_passes(data):
    from mermaid_classifier_amd import FeatureSet, partial_fit_rows_group
    fs = FeatureSet(NF, np.arange(K7)).append(data["X"], data["y"])
    group, solo = _mixed_members(data), _mixed_members(data)
    row_group = (np.arange(N) % 3).astype(np.int32)
    groups = [None, None, None, row_group, None]
    for _ in range(2):
        partial_fit_rows_group(group, fs, classes=list(range(K7)), row_group=groups)
        for clf, g in zip(solo, groups):
            clf.partial_fit_rows(fs, classes=list(range(K7)), row_group=g)
    for a, b in zip(group, solo):
        _assert_same_state(a, b)
    assert np.array_equal(group[3].group_weights_, solo[3].group_weights_) and not np.allclose(group[3].group_weights_, 1.0 / 3.0)
    assert [c._adam_state()["step"] for c in group] == [10, 10, 10, 8, 10]
    assert len({tuple(c.loss_curve_) for c in group}) == 5
    fs.close()


def test_chunk_size_of_a_resident_pass_changes_nothing(data, monkeypatch):
    from mermaid_classifier_amd import FeatureSet
    fs = FeatureSet(NF, np.arange(K7)).append(data["X"], data["y"])
    whole, chunked = _make(data, **_TRAIN_KINDS["soft+levels+prior"]), _make(data, **_TRAIN_KINDS["soft+levels+prior"])
    for _ in range(2):
        monkeypatch.delenv("MMC_TRAIN_CHUNK_ROWS", raising=False)
        whole.partial_fit_rows(fs, classes=list(range(K7)))
        monkeypatch.setenv("MMC_TRAIN_CHUNK_ROWS", "100")       # chunks of two mini-batches: 100, 100, 30 rows
        chunked.partial_fit_rows(fs, classes=list(range(K7)))
    monkeypatch.delenv("MMC_TRAIN_CHUNK_ROWS", raising=False)
    _assert_same_state(whole, chunked)
    fs.close()


def test_pickled_twin_carries_the_hierarchy(data):
    clf = _make(data, **_TRAIN_KINDS["soft+levels+prior"])
    flat = _make(data, use_prior=True, weighted=True)
    for c in (clf, flat):
        c.partial_fit(data["X"], data["y"], classes=list(range(K7)))
    assert clf.loss_curve_ != flat.loss_curve_
    twin = pickle.loads(pickle.dumps(clf))
    assert twin.get_params() == clf.get_params()
    clf.partial_fit(data["X"], data["y"])
    twin.partial_fit(data["X"], data["y"])
    _assert_same_state(clf, twin)


def test_set_hierarchy_default_restored_or_rejected_changes_no_bits(data):
    from mermaid_classifier_amd import _lib
    clf = _make(data)
    clf.classes_, clf.n_features_in_ = np.arange(K7), NF
    w0, b0 = clf._initial_parameters()
    X, y = data["X"], data["y"]
    levels, T = np.ascontiguousarray(data["levels"].T), data["T"]
    names = ("untouched", "default", "restored", "rejected", "hier", "hier_rejected", "soft", "soft_rejected", "smooth", "smooth_rejected")
    t = {name: _Raw(w0, b0, class_weight=data["w"]) for name in names}
    try:
        assert t["default"].set_hierarchy() == 0
        assert t["restored"].set_hierarchy(levels, LAM3, T) == 0 and t["restored"].set_hierarchy() == 0
        for name in ("hier", "hier_rejected"):
            assert t[name].set_hierarchy(levels, LAM3, None) == 0
        for name in ("soft", "soft_rejected"):
            assert t[name].set_hierarchy(None, None, T) == 0
        for name in ("smooth", "smooth_rejected"):
            assert t[name].set_loss(0.1, 0.0, None) == 0
        curves = {name: [t[name].partial_fit(X, y, 50)] for name in names}
        nan_T, off_T, neg_T = T.copy(), T.copy(), T.copy()
        nan_T[2, 3] = np.nan
        off_T[4, 4] += 1e-3
        neg_T[1, 0], neg_T[1, 1] = -0.1, neg_T[1, 1] + neg_T[1, 0] + 0.1
        lib = t["rejected"].lib
        for name in ("rejected", "hier_rejected"):
            bad = [(dict(levels=levels, lam=LAM3, n_levels=5), b"n_levels = 5"), (dict(levels=levels, lam=LAM3, n_levels=-1), b"n_levels = -1"),
                   (dict(levels=levels, lam=[1.0, -0.5, 0.25]), b"level_weight[1] = -0.5"),
                   (dict(levels=levels, lam=[1.0, 0.5, np.inf]), b"level_weight[2] = inf"), (dict(T=nan_T), b"soft_targets[2][3]"),
                   (dict(T=neg_T), b"soft_targets[1][0]"), (dict(T=off_T), b"row 4"), (dict(levels=levels, lam=None, n_levels=3), b"needs")]
            for args, says in bad:
                assert t[name].set_hierarchy(**args) == _lib.MMC_ERR_ARG and says in lib.mmc_last_error(), (args, lib.mmc_last_error())
        # T with smoothing or focusing: whichever setter comes second refuses and leaves the trainer as it was
        assert t["smooth_rejected"].set_hierarchy(None, None, T) == _lib.MMC_ERR_ARG and b"label_smoothing" in lib.mmc_last_error()
        assert t["smooth_rejected"].set_hierarchy(levels, LAM3, T) == _lib.MMC_ERR_ARG
        assert t["soft_rejected"].set_loss(0.1, 0.0, None) == _lib.MMC_ERR_ARG and b"soft targets" in lib.mmc_last_error()
        assert t["soft_rejected"].set_loss(0.0, 2.0, None) == _lib.MMC_ERR_ARG
        for name in names:
            curves[name].append(t[name].partial_fit(X, y, 50))
        state = {name: t[name].state() for name in names}
        for a, b in (("untouched", "default"), ("untouched", "restored"), ("untouched", "rejected"), ("hier", "hier_rejected"),
                     ("soft", "soft_rejected"), ("smooth", "smooth_rejected")):
            assert curves[a] == curves[b] and _same_raw(state[a], state[b]), (a, b)
        assert len({tuple(curves[name]) for name in ("untouched", "hier", "soft", "smooth")}) == 4
    finally:
        for raw in t.values():
            raw.close()


# ---- 4. a mixed pass takes no hierarchy -------------------------------------------------------------------------------------------
def test_every_mixed_entry_point_refuses_a_trainer_with_a_hierarchy(data):
    from mermaid_classifier_amd import FeatureSet, _lib
    clf = _make(data)
    clf.classes_, clf.n_features_in_ = np.arange(K7), NF
    w0, b0 = clf._initial_parameters()
    levels = np.ascontiguousarray(data["levels"].T)
    fs = FeatureSet(NF, np.arange(K7)).append(data["X"], data["y"])
    hier, soft, flat = (_Raw(w0, b0, class_weight=data["w"]) for _ in range(3))
    try:
        assert hier.set_hierarchy(levels, LAM3, None) == 0 and soft.set_hierarchy(None, None, data["T"]) == 0
        lib = hier.lib
        before = [t.state() for t in (hier, soft, flat)]
        z = np.zeros((5, K7), np.float32)
        y5 = np.array([0, 1, 2, 4, 5], np.int32)
        d, l = np.empty_like(z), np.empty(5, np.float32)
        visit = np.arange(N, dtype=np.int64)
        partner = np.ascontiguousarray(visit[::-1])
        lam = np.full(5, 0.7, np.float32)
        avg = C.c_double(0.0)
        for t in (hier, soft):
            assert lib.mmc_trainer_loss_gradient_mixed(t.h, z.ctypes.data, y5.ctypes.data, y5.ctypes.data, 0.7, 5, d.ctypes.data, l.ctypes.data,
                                                       None) == _lib.MMC_ERR_ARG and b"hierarchy" in lib.mmc_last_error()
            assert lib.mmc_trainer_partial_fit_set_mixed(t.h, fs._handle(), visit.ctypes.data, partner.ctypes.data, lam.ctypes.data, N, 50,
                                                         C.byref(avg), None) == _lib.MMC_ERR_ARG and b"hierarchy" in lib.mmc_last_error()
        # grouped: the member with the hierarchy and a partner array is refused, and nobody has moved
        handles = (C.c_void_p * 2)(flat.h.value, hier.h.value)
        visits = (C.c_void_p * 2)(visit.ctypes.data, visit.ctypes.data)
        lams = (C.c_void_p * 2)(lam.ctypes.data, lam.ctypes.data)
        ns, bss, avgs = (C.c_int64 * 2)(N, N), (C.c_int * 2)(50, 50), (C.c_double * 2)()
        both = (C.c_void_p * 2)(partner.ctypes.data, partner.ctypes.data)
        assert lib.mmc_trainer_group_partial_fit_set_mixed(handles, 2, fs._handle(), visits, both, lams, ns, bss, avgs,
                                                           None) == _lib.MMC_ERR_ARG and b"member 1" in lib.mmc_last_error()
        assert all(_same_raw(t.state(), s) for t, s in zip((hier, soft, flat), before))
        # the member with the hierarchy is not mixed: the pass runs, the flat member mixed beside it
        only_flat = (C.c_void_p * 2)(partner.ctypes.data, None)
        only_lam = (C.c_void_p * 2)(lam.ctypes.data, None)
        assert lib.mmc_trainer_group_partial_fit_set_mixed(handles, 2, fs._handle(), visits, only_flat, only_lam, ns, bss, avgs, None) == 0, \
            lib.mmc_last_error()
        assert hier.state()[1] == 5 and flat.state()[1] == 5
    finally:
        for t in (hier, soft, flat):
            t.close()
        fs.close()
    mixed = _make(data, mixup_alpha=0.3, **_TRAIN_KINDS["levels"])
    fs = FeatureSet(NF, np.arange(K7)).append(data["X"], data["y"])
    with pytest.raises(ValueError, match="mixup_alpha"):
        mixed.partial_fit_rows(fs, classes=list(range(K7)))
    fs.close()


# ---- 5. a sweep over flat and taxonomy-aware heads ----------------------------------------------------------------------------------
def test_train_sweep_with_a_hierarchy_equals_train_classifier(data):
    from mermaid_classifier_amd import FeatureSet, SweepConfig, hierarchy_levels, soft_labels, train_classifier, train_sweep
    X, y = data["X"], data["y"]
    sets = [FeatureSet(NF, np.arange(K7)).append(X[s], y[s]) for s in (slice(0, 130), slice(130, 180), slice(180, 230))]
    lv = hierarchy_levels(PATHS7, depths=(1,))
    S = np.array([[sum(1 for p, q in zip(a, b) if p == q) / 2.0 for b in PATHS7] for a in PATHS7])
    T = soft_labels(S, 3.0)
    base = dict(hidden_layer_sizes=(24, 12), learning_rate_init=3e-3, alpha=1e-3, random_state=0, batch_size=50)
    configs = [SweepConfig(**base),
               SweepConfig(**base, class_levels={k: lv[k].tolist() for k in range(K7)}, level_weights=[2.0, 0.5],
                           soft_targets={t: {c: float(T[t, c]) for c in range(K7)} for t in range(K7)})]
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
