"""Distillation on the device: the resident target set, ``mmc_ensemble_predict_set``, ``ce_grad_distill_kernel`` and the distilled
passes (include/mmc.h, "distillation").

``mmc_trainer_loss_gradient_distill`` per element against the fp64 checker within the bounds of tests/distill_checker.py (derived
there from ``ce_grad_rows_distill``'s operation count; tests/test_distill_host.py shows an fp32 evaluation in the kernel's order uses
a tenth of them and wrong kernels miss them by four orders of magnitude).  Training against a torch-CPU fp32 loop within the
tolerances of tests/test_trainer.py for this kind of comparison (weights 2e-5, loss curve 1e-5).  Everything else is bit equality or
a refusal that changes nothing.

Group DRO over the distilled stage goes through ``mmc_trainer_loss_gradient_distill_weighted``, the weighted probe's route with the
target rows, and is held to the composition of tests/hier_loss_checker.py's ``with_groups`` as tests/test_gpu_hier_loss.py holds the
hierarchy's kernel to it."""

import ctypes as C
import pickle

import numpy as np
import pytest

import distill_checker as dc
import loss_checker as lc

pytestmark = pytest.mark.gpu

KINDS, _opts, _peak = dc.KINDS, dc.kind_options, dc.peak

W_TOL, LOSS_TOL = 2e-5, 1e-5          # tests/test_trainer.py
K7, NF, N = 7, 16, 230                # the data of tests/test_gpu_loss.py
MMC_ERR_ARG = 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _err():
    from mermaid_classifier_amd import _lib
    return _lib.lib().mmc_last_error().decode()


# ---- raw trainers through the C ABI -------------------------------------------------------------------------------------------
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

    def set_distillation(self, alpha, tau):
        return self.lib.mmc_trainer_set_distillation(self.h, float(alpha), float(tau))

    def set_hierarchy(self, levels=None, lam=None, T=None):
        ids = None if levels is None else np.ascontiguousarray(levels, np.int32)
        wl = None if lam is None else np.ascontiguousarray(lam, np.float64)
        Tm = _f32(T)
        return self.lib.mmc_trainer_set_hierarchy(self.h, 0 if ids is None else len(ids), None if ids is None else ids.ctypes.data,
                                                  None if wl is None else wl.ctypes.data, None if Tm is None else Tm.ctypes.data)

    def loss_gradient_distill(self, z, y, q, r=None):
        z, y32, q32, r32 = _f32(z), np.ascontiguousarray(y, np.int32), _f32(q), _f32(r)
        d, l = np.full(z.shape, np.nan, np.float32), np.full(len(y32), np.nan, np.float32)
        status = self.lib.mmc_trainer_loss_gradient_distill(self.h, z.ctypes.data, y32.ctypes.data, q32.ctypes.data,
                                                            None if r32 is None else r32.ctypes.data, len(y32), d.ctypes.data, l.ctypes.data, None)
        return status, d, l

    def loss_gradient_distill_weighted(self, z, y, q, r=None, a=None, logq=None, eta=0.0, G=0):
        z, y32, q32, r32 = _f32(z), np.ascontiguousarray(y, np.int32), _f32(q), _f32(r)
        a32 = None if a is None else np.ascontiguousarray(a, np.int32)
        d, l = np.full(z.shape, np.nan, np.float32), np.full(len(y32), np.nan, np.float32)
        qi = None if a is None else np.ascontiguousarray(logq, np.float64)
        qo = None if a is None else np.full(G, np.nan)
        status = self.lib.mmc_trainer_loss_gradient_distill_weighted(
            self.h, z.ctypes.data, y32.ctypes.data, q32.ctypes.data, None if r32 is None else r32.ctypes.data,
            None if a32 is None else a32.ctypes.data, None if qi is None else qi.ctypes.data, float(eta), int(G), len(y32), d.ctypes.data,
            l.ctypes.data, None if qo is None else qo.ctypes.data, None, None)
        return status, d, l, qo

    def pass_distill(self, fs, ts, visit=None, rw=None, rg=None, n=None, batch_size=50):
        """-> (status, avg loss) of mmc_trainer_partial_fit_set_distill; ``ts`` None is the NULL target set."""
        v = None if visit is None else np.ascontiguousarray(visit, np.int64)
        w, g = _f32(rw), None if rg is None else np.ascontiguousarray(rg, np.int32)
        avg = C.c_double(-1.0)
        status = self.lib.mmc_trainer_partial_fit_set_distill(
            self.h, fs._handle(), None if ts is None else ts._handle(), None if v is None else v.ctypes.data,
            None if w is None else w.ctypes.data, None if g is None else g.ctypes.data, len(fs) if n is None else n, batch_size,
            C.byref(avg), None)
        return status, avg.value

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
    return sa == sb and len(pa) == len(pb) and all(np.array_equal(bits(u), bits(v)) for u, v in zip(pa, pb))


# ---- 1. the loss stage per element ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [3, 65, 108, 130])
def test_loss_gradient_per_element_against_the_fp64_checker(K, weighted):
    rng = np.random.default_rng([K, int(weighted), 7])
    w = lc.class_weights(rng, K) if weighted else None
    prior = lc.dirichlet_prior(rng, K)
    z, y = lc.logit_rows(rng, 205, K, 4.0)          # 205 rows: the last workgroup holds one; the four special rows included
    q = dc.teacher_rows(rng, y, K)
    raw = _Raw([np.zeros((K, 4), np.float32)], [np.zeros(K, np.float32)], class_weight=w)
    try:
        for name, kind in KINDS:
            alpha, tau, o = _opts(kind, prior)
            assert raw.set_loss(o.get("eps", 0.0), o.get("gamma", 0.0), o.get("prior")) == 0, _err()
            assert raw.set_distillation(alpha, tau) == 0, _err()
            status, d, l = raw.loss_gradient_distill(z, y, q)
            assert status == 0, _err()
            assert np.isfinite(d).all() and np.isfinite(l).all()
            grad, rows, k = dc.checker(z, y, q, alpha, tau, w, **o)
            bd, bl = dc.bounds(z, y, q, alpha, tau, w, rows, k, prior=o.get("prior"))
            ed, el = _peak(d - grad, bd), _peak(l - rows, bl)
            print(f"K {K} weighted {weighted} {name:26s}: dlogits {ed:.3f} of its bound, row_loss {el:.3f} of its bound")
            assert ed <= 1.0 and el <= 1.0, (name, ed, el)
        # row weights ride the same kernel; two rows of weight 0 are exactly 0
        assert raw.set_loss() == 0 and raw.set_distillation(0.3, 2.0) == 0
        r = rng.uniform(1e-2, 1e2, len(y)).astype(np.float32)
        r[[2, 5]] = 0.0
        status, d, l = raw.loss_gradient_distill(z, y, q, r=r)
        assert status == 0, _err()
        assert np.isfinite(d).all() and np.isfinite(l).all() and (d[2] == 0).all() and (d[5] == 0).all() and l[2] == 0 and l[5] == 0
        exact = dc.normaliser(y, w, r, exact=True)
        grad, rows, k = dc.checker(z, y, q, 0.3, 2.0, w, norm=exact)
        bd, bl = dc.bounds(z, y, q, 0.3, 2.0, w, rows, k, norm=exact)
        ed, el = _peak(d - grad, bd), _peak(l - rows, bl)
        print(f"K {K} weighted {weighted} a=0.3 t=2, row weights    : dlogits {ed:.3f} of its bound, row_loss {el:.3f} of its bound")
        assert ed <= 1.0 and el <= 1.0, (ed, el)
        # the weighted probe's route without groups is the probe above, bit for bit
        status, d2, l2, _ = raw.loss_gradient_distill_weighted(z, y, q, r=r)
        assert status == 0 and np.array_equal(bits(d2), bits(d)) and np.array_equal(bits(l2), bits(l)), _err()
        # three groups with eta = 0.5: the stage's normaliser is r_i itself, then the DRO update and every row's share
        G, eta = 3, 0.5
        a = rng.integers(0, G, len(y))
        logq = np.log(np.array([0.5, 0.3, 0.2]))
        status, d, l, lq = raw.loss_gradient_distill_weighted(z, y, q, r=r, a=a, logq=logq, eta=eta, G=G)
        assert status == 0, _err()
        assert np.isfinite(d).all() and np.isfinite(l).all() and np.isfinite(lq).all() and (d[2] == 0).all() and l[5] == 0
        rr = r.astype(np.float64)
        D, R, k = dc.checker(z, y, q, 0.3, 2.0, w, norm=rr)
        bD, bR = dc.bounds(z, y, q, 0.3, 2.0, w, R, k, norm=rr)
        v = rr * (1.0 if w is None else w.astype(np.float64)[y])
        ref, bnd = dc.with_groups(D, R, bD, bR, v, a, logq, eta, G)
        ed, el, eq = _peak(d - ref["dlogits"], bnd["dlogits"]), _peak(l - ref["row_loss"], bnd["row_loss"]), _peak(lq - ref["logq"], bnd["logq"])
        print(f"K {K} weighted {weighted} a=0.3 t=2, groups         : dlogits {ed:.3f}, row_loss {el:.3f}, log q {eq:.3f} of their bounds")
        assert ed <= 1.0 and el <= 1.0 and eq <= 1.0, (ed, el, eq)
    finally:
        raw.close()


# ---- 2. the target set and mmc_ensemble_predict_set -----------------------------------------------------------------------------------
def _member(rng, dims, classes):
    from mermaid_classifier_amd import CalibratedMLP
    K = dims[-1]
    W = [rng.normal(0, 0.5, (dims[i + 1], dims[i])).astype(np.float32) for i in range(len(dims) - 1)]
    b = [rng.normal(0, 0.2, dims[i + 1]).astype(np.float32) for i in range(len(dims) - 1)]
    return CalibratedMLP(W, b, classes, rng.uniform(-3, -0.5, K), rng.uniform(-1, 1, K))


def test_predict_set_has_the_bits_of_ensemble_topk_proba():
    from mermaid_classifier_amd import FeatureSet, HeadEnsemble, TargetSet, _lib, teacher_targets
    rng = np.random.default_rng(5)
    dim, K, n, first = 8, 7, 4100, 3               # 16 members: 4096-row ensemble chunks, so the call crosses one
    classes = list(range(K))
    members = [_member(rng, (dim, 5, K), classes) for _ in range(16)]
    X = rng.normal(0, 1, (n + first, dim)).astype(np.float32)
    fs = FeatureSet(dim, classes).append(X, rng.integers(0, K, n + first))
    ens = HeadEnsemble(members)
    assert _lib.lib().mmc_ensemble_chunk_rows(ens._handle(), 1) == 4096
    want = ens.topk(X[first:], 1, want_proba=True)[2]
    ts = TargetSet(classes)
    _lib.check(_lib.lib().mmc_ensemble_predict_set(ens._handle(), fs._handle(), first, n, ts._handle(), None))
    assert len(ts) == n
    got = ts.read()
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(ts.read(4090, 10)), bits(want[4090:]))
    # the Python route over the whole set, and one member against mmc_head_predict
    whole = teacher_targets(ens, fs)
    assert len(whole) == n + first and np.array_equal(bits(whole.read(first)), bits(want))
    one = teacher_targets(members[3], fs)
    assert np.array_equal(bits(one.read()), bits(members[3]._device_head().predict(X, want_argmax=False)[0]))
    # read returns what append stored, from host and from device; growth keeps the rows
    import torch
    store = TargetSet(classes, reserve_rows=2)
    store.append(want[:5]).append(torch.from_numpy(want[5:900]).cuda()).append(want[900:])
    assert len(store) == n and np.array_equal(bits(store.read()), bits(want)) and store.read(7, 0).shape == (0, K)
    for t in (ts, whole, one, store):
        t.close()
    ens.close()
    fs.close()


# ---- 3. training parity against torch on the CPU ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data():
    from mermaid_classifier_amd import FeatureSet, HeadEnsemble, teacher_targets
    rng = np.random.default_rng(17)
    y = rng.integers(0, K7, size=N)
    centres = rng.normal(0, 1.0, (K7, NF))
    X = (centres[y] + rng.normal(0, 1.0, (N, NF))).astype(np.float32)
    w = np.array([1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.75], np.float32)
    classes = list(range(K7))
    fs = FeatureSet(NF, classes).append(X, y)
    mrng = np.random.default_rng(23)
    ens_a = HeadEnsemble([_member(mrng, (NF,) + h + (K7,), classes) for h in ((), (12,), (10, 6))])
    ens_b = HeadEnsemble([_member(mrng, (NF, 9, K7), classes) for _ in range(2)])
    ts_a, ts_b = teacher_targets(ens_a, fs), teacher_targets(ens_b, fs)
    d = dict(X=X, y=y, w=w, cw={k: float(v) for k, v in enumerate(w)}, fs=fs, ts_a=ts_a, ts_b=ts_b, Q_a=ts_a.read(), Q_b=ts_b.read(),
             rw=rng.uniform(0.25, 4.0, N).astype(np.float32), rg=rng.integers(0, 3, N).astype(np.int32))
    yield d
    for h in (ts_a, ts_b, fs, ens_a, ens_b):
        h.close()


def _make(hidden=(24, 12), weighted=False, data=None, **kw):
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    args = dict(hidden_layer_sizes=hidden, learning_rate_init=1e-3, alpha=1e-3, random_state=0, batch_size=50,
                class_weight=data["cw"] if weighted else None)
    args.update(kw)
    return TorchMLPClassifier(**args)


def _torch_loop(data, clf, Q, passes):
    """The reference's mini-batch loop in torch on the CPU, fp32: same initial parameters and visiting order, torch.optim.Adam, the L2
    term (0.5 alpha / mb) sum W^2; the loss is autograd of the distillation definition."""
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
    alpha, tau = float(clf.distill_alpha), float(clf.distill_temperature)

    def data_loss(logits, yb, qb):
        logp = torch.log_softmax(logits, dim=1)
        base = w[yb] * -logp.gather(1, yb[:, None])[:, 0]
        if tau == 1.0:
            qt, logpt = qb, logp
        else:
            qt = qb ** (1.0 / tau)
            qt = qt / qt.sum(dim=1, keepdim=True)
            logpt = torch.log_softmax(logits / tau, dim=1)
        k = -(qt * logpt).sum(dim=1)
        return ((1.0 - alpha) * base + alpha * tau * tau * w[yb] * k).sum() / w[yb].sum()

    order = np.arange(N)
    np.random.default_rng(0).shuffle(order)                     # the classifier's shuffle: a fresh generator per pass
    Xo, yo = torch.from_numpy(data["X"][order]), torch.from_numpy(data["y"][order].astype(np.int64))
    Qo = torch.from_numpy(Q[order])
    curve = []
    for _ in range(passes):
        total = 0.0
        for start in range(0, N, 50):
            xb, yb, qb = Xo[start:start + 50], yo[start:start + 50], Qo[start:start + 50]
            opt.zero_grad()
            h = xb
            for i, m in enumerate(layers):
                h = m(h)
                if i < len(layers) - 1:
                    h = torch.relu(h)
            loss = data_loss(h, yb, qb) + (0.5 * clf.alpha / len(yb)) * sum((m.weight ** 2).sum() for m in layers)
            loss.backward()
            opt.step()
            total += loss.item() * len(yb)
        curve.append(total / N)
    return curve, [m.weight.detach().numpy() for m in layers], [m.bias.detach().numpy() for m in layers]


@pytest.mark.parametrize("tau", [1.0, 2.0])
def test_training_matches_torch(data, tau):
    kw = dict(weighted=True, data=data, distill_alpha=0.6, distill_temperature=tau)
    assert (data["Q_a"] > 0).all()                                 # the torch loop's pow has no zero to step around
    want_curve, want_w, want_b = _torch_loop(data, _make(**kw), data["Q_a"], 3)
    clf = _make(**kw)
    for _ in range(3):
        clf.partial_fit_rows(data["fs"], classes=list(range(K7)), targets=data["ts_a"])
    print("tau", tau, "loss curve", clf.loss_curve_, "torch", want_curve)
    np.testing.assert_allclose(clf.loss_curve_, want_curve, rtol=0, atol=LOSS_TOL)
    ws, bs = clf.parameters()
    for i in range(3):
        dw, db = np.abs(ws[i] - want_w[i]).max(), np.abs(bs[i] - want_b[i]).max()
        print(f"layer {i}: max|dW| {dw:.2e} max|db| {db:.2e}")
        assert dw <= W_TOL and db <= W_TOL
    assert clf._adam_state()["step"] == 15                       # 50, 50, 50, 50, 30 rows: the last mini-batch is ragged


# ---- 4. bit equality ------------------------------------------------------------------------------------------------------------------
def _state(clf):
    s = clf._adam_state()
    return ([a.copy() for part in clf.parameters() for a in part], [a.copy() for part in s["exp_avg"] for a in part],
            [a.copy() for part in s["exp_avg_sq"] for a in part], s["step"], list(clf.loss_curve_), clf.n_iter_)


def _assert_same_state(a, b):
    sa, sb = (x if isinstance(x, tuple) else _state(x) for x in (a, b))
    for u, v in zip(sa[:3], sb[:3]):
        assert len(u) == len(v)
        for p, q in zip(u, v):
            assert np.array_equal(bits(p), bits(q))
    assert sa[3:] == sb[3:]


def _raw7(rng_seed=3, class_weight=None):
    rng = np.random.default_rng(rng_seed)
    dims = (NF, 12, K7)
    W = [rng.normal(0, 0.3, (dims[i + 1], dims[i])).astype(np.float32) for i in range(2)]
    return _Raw(W, [np.zeros(dims[i + 1], np.float32) for i in range(2)], class_weight=class_weight)


def test_visiting_order_is_applied_to_the_target_rows_in_place(data):
    from mermaid_classifier_amd import FeatureSet, TargetSet
    perm = np.random.default_rng(4).permutation(N)
    fs2 = FeatureSet(NF, list(range(K7))).append(data["X"][perm], data["y"][perm])
    ts2 = TargetSet(list(range(K7))).append(data["Q_a"][perm])
    runs = []
    for fs, ts, visit in ((data["fs"], data["ts_a"], perm), (fs2, ts2, None), (fs2, ts2, np.arange(N))):
        raw = _raw7(class_weight=data["w"])
        assert raw.set_distillation(0.5, 2.0) == 0
        out = [raw.pass_distill(fs, ts, visit=visit, rw=data["rw"][perm]) for _ in range(2)]
        assert all(s == 0 for s, _ in out), _err()
        runs.append((raw.state(), [a for _, a in out]))
        raw.close()
    for other in runs[1:]:
        assert _same_raw(runs[0][0], other[0]) and runs[0][1] == other[1]
    ts2.close()
    fs2.close()


def test_chunk_size_of_a_resident_pass_changes_nothing(data, monkeypatch):
    visit = np.random.default_rng(6).permutation(N)
    runs = []
    for chunk in (None, "100"):                                  # mini-batch 50, N = 230: target rows are fetched across chunk boundaries
        if chunk is not None:
            monkeypatch.setenv("MMC_TRAIN_CHUNK_ROWS", chunk)
        raw = _raw7(class_weight=data["w"])
        assert raw.set_distillation(0.4, 2.0) == 0
        out = [raw.pass_distill(data["fs"], data["ts_b"], visit=visit, rw=data["rw"]) for _ in range(2)]
        assert all(s == 0 for s, _ in out), _err()
        runs.append((raw.state(), [a for _, a in out]))
        raw.close()
    assert _same_raw(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


def _members(data):
    """A plain member, one on set A at tau = 1, one on set B at tau = 2, one on set A with row weights, one on set A with groups."""
    clfs = [_make((), data=data), _make((24,), weighted=True, data=data, distill_alpha=0.5),
            _make((24, 12), data=data, distill_alpha=0.7, distill_temperature=2.0, random_state=3),
            _make((20, 10, 5), weighted=True, data=data, batch_size=64, distill_alpha=1.0),
            _make((9,), data=data, distill_alpha=0.3, distill_temperature=4.0, n_groups=3, group_dro_eta=0.5)]
    targets = [None, data["ts_a"], data["ts_b"], data["ts_a"], data["ts_a"]]
    weights = [None, None, None, data["rw"], data["rw"]]
    groups = [None, None, None, None, data["rg"]]
    return clfs, targets, weights, groups


def test_grouped_pass_has_the_bits_of_the_solo_passes(data):
    from mermaid_classifier_amd import partial_fit_rows_group
    solo, targets, weights, groups = _members(data)
    grouped, _, _, _ = _members(data)
    classes = list(range(K7))
    rows = np.random.default_rng(8).permutation(N)[:170]
    for r in (None, rows):
        for clf, t, w, g in zip(solo, targets, weights, groups):
            clf.partial_fit_rows(data["fs"], r, classes=classes, row_weight=w, row_group=g, targets=t)
        partial_fit_rows_group(grouped, data["fs"], r, classes=classes, row_weight=weights, row_group=groups, targets=targets)
    for a, b in zip(solo, grouped):
        _assert_same_state(a, b)
    assert np.array_equal(solo[4].group_weights_, grouped[4].group_weights_)
    # the plain member never saw the targets: it has the bits of a pass without any
    alone = _make((), data=data)
    for r in (None, rows):
        alone.partial_fit_rows(data["fs"], r, classes=classes)
    _assert_same_state(alone, grouped[0])
    # and a pass is reproducible
    again, _, _, _ = _members(data)
    for r in (None, rows):
        partial_fit_rows_group(again, data["fs"], r, classes=classes, row_weight=weights, row_group=groups, targets=targets)
    for a, b in zip(again, grouped):
        _assert_same_state(a, b)


def test_pickled_twin_carries_the_options(data):
    classes = list(range(K7))
    clf = _make(weighted=True, data=data, distill_alpha=0.6, distill_temperature=2.0)
    clf.partial_fit_rows(data["fs"], classes=classes, targets=data["ts_a"])
    twin = pickle.loads(pickle.dumps(clf))
    assert (twin.distill_alpha, twin.distill_temperature) == (0.6, 2.0)
    for c in (clf, twin):
        c.partial_fit_rows(data["fs"], classes=classes, targets=data["ts_a"])
    _assert_same_state(clf, twin)


def test_default_restored_or_unused_distillation_changes_no_bits(data):
    def run(prepare):
        raw = _raw7(class_weight=data["w"])
        prepare(raw)
        avg = [raw.partial_fit(data["X"], data["y"], 50) for _ in range(2)]
        s, a = raw.pass_distill(data["fs"], None, rw=data["rw"])      # ts == NULL: the weighted pass
        assert s == 0, _err()
        out = raw.state(), avg + [a]
        raw.close()
        return out

    def restored(raw):
        assert raw.set_distillation(0.5, 2.0) == 0 and raw.set_distillation(0.0, 1.0) == 0

    def unused(raw):
        assert raw.set_distillation(0.5, 2.0) == 0                # set, but no pass is given targets

    base = run(lambda raw: None)
    for prepare in (restored, unused):
        got = run(prepare)
        assert _same_raw(base[0], got[0]) and base[1] == got[1]
    # ts == NULL is mmc_trainer_partial_fit_set_weighted, bit for bit
    raw = _raw7(class_weight=data["w"])
    rw = _f32(data["rw"])
    for _ in range(2):
        raw.partial_fit(data["X"], data["y"], 50)
    avg = C.c_double(0.0)
    assert raw.lib.mmc_trainer_partial_fit_set_weighted(raw.h, data["fs"]._handle(), None, rw.ctypes.data, None, N, 50, C.byref(avg), None) == 0
    assert _same_raw(base[0], raw.state()) and avg.value == base[1][2]
    raw.close()


# ---- 5. refusals change nothing ---------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(data):
    from mermaid_classifier_amd import FeatureSet, HeadEnsemble, TargetSet, _lib
    lib = _lib.lib()
    classes = list(range(K7))
    raw = _raw7(class_weight=data["w"])
    assert raw.set_distillation(0.5, 2.0) == 0
    assert raw.pass_distill(data["fs"], data["ts_a"])[0] == 0
    before = raw.state()
    rows_before = len(data["ts_a"])

    def refused(status, *words):
        msg = _err()
        assert status == MMC_ERR_ARG, (status, msg)
        for word in words:
            assert word in msg, (word, msg)
        assert _same_raw(before, raw.state()) and len(data["ts_a"]) == rows_before

    for a, t, word in ((-0.1, 1.0, "alpha"), (1.1, 1.0, "alpha"), (float("nan"), 1.0, "alpha"), (0.5, 0.2, "temperature"),
                       (0.5, 65.0, "temperature"), (0.5, float("nan"), "temperature")):
        refused(raw.set_distillation(a, t), word)
    assert raw.pass_distill(data["fs"], data["ts_a"])[0] == 0        # the options are still alpha = 0.5, tau = 2
    before = raw.state()
    # K, row-count and device mismatches (one card: the device check is read in the source's order by the message of the others)
    ts_k = TargetSet(list(range(K7 + 1))).append(np.full((N, K7 + 1), 1.0 / (K7 + 1), np.float32))
    refused(raw.pass_distill(data["fs"], ts_k)[0], "target set has 8 classes, trainer 7")
    ts_n = TargetSet(classes).append(data["Q_a"][:-1])
    refused(raw.pass_distill(data["fs"], ts_n)[0], "target set has 229 rows, feature set 230")
    # a hierarchy, in both orders
    levels = np.array([[0, 0, 1, 1, 2, 2, 2]], np.int32)
    refused(raw.set_hierarchy(levels, [1.0]), "distillation")
    assert raw.set_distillation(0.0, 1.0) == 0 and raw.set_hierarchy(levels, [1.0]) == 0
    refused(raw.set_distillation(0.5, 2.0), "hierarchy")
    refused(raw.pass_distill(data["fs"], data["ts_a"])[0], "alpha > 0")          # alpha = 0 now: the message of the row_group precedent
    assert raw.set_hierarchy() == 0
    refused(raw.pass_distill(data["fs"], data["ts_a"])[0], "needs mmc_trainer_set_distillation(alpha > 0)")
    z = np.zeros((5, K7), np.float32)
    st, _, _ = raw.loss_gradient_distill(z, np.arange(5), data["Q_a"][:5])
    refused(st, "needs mmc_trainer_set_distillation(alpha > 0)")
    assert raw.set_distillation(0.5, 2.0) == 0
    # a mixed pass with targets: the Python surface refuses, and the library has no entry point that takes both
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    mixed = TorchMLPClassifier(hidden_layer_sizes=(9,), mixup_alpha=0.4, distill_alpha=0.5, random_state=0)
    with pytest.raises(ValueError, match="mixup_alpha > 0 cannot be combined with targets"):
        mixed.partial_fit_rows(data["fs"], classes=classes, targets=data["ts_a"])
    assert not mixed._fitted()
    # invalid rows: appended, and in the probe
    good = data["Q_a"][:20].copy()
    store = TargetSet(classes).append(good)
    for col, value, words in ((5, -0.25, ("row 17", "entry 5 = -0.25")), (5, np.nan, ("row 17", "entry 5 = nan")), (None, 0.93, ("row 17 sums to 0.93",))):
        bad = good.copy()
        if col is None:
            bad[17] *= value
        else:
            bad[17, col] = value
        status = lib.mmc_targetset_append(store._handle(), bad.ctypes.data, 20, _lib.MMC_IN_HOST, None)
        msg = _err()
        assert status == MMC_ERR_ARG and all(wd in msg for wd in words), msg
        assert len(store) == 20 and np.array_equal(bits(store.read()), bits(good))
        with pytest.raises(ValueError, match="row 17"):
            store.append(bad)
        st, _, _ = raw.loss_gradient_distill(np.zeros((20, K7), np.float32), np.zeros(20, np.int64), bad)
        refused(st, "row 17")
    store.append(good)                                             # the refused rows were never committed: the next rows follow row 19
    assert len(store) == 40 and np.array_equal(bits(store.read(20)), bits(good))
    # mmc_ensemble_predict_set over a set row with a NaN feature
    Xn = data["X"][:50].copy()
    Xn[31, 4] = np.nan
    fsn = FeatureSet(NF, classes).append(Xn, data["y"][:50])
    # (a member without a hidden layer: its logits carry the NaN, where a ReLU's fmaxf would have swallowed it)
    ens = HeadEnsemble([_member(np.random.default_rng(2), (NF, 6, K7), classes), _member(np.random.default_rng(3), (NF, K7), classes)])
    status = lib.mmc_ensemble_predict_set(ens._handle(), fsn._handle(), 10, 40, store._handle(), None)
    msg = _err()
    assert status == MMC_ERR_ARG and "row 31" in msg and "nan" in msg, msg
    assert len(store) == 40
    assert lib.mmc_ensemble_predict_set(ens._handle(), fsn._handle(), 0, 31, store._handle(), None) == 0 and len(store) == 71
    # cells past MMC_TARGETSET_MAX_CELLS: refused arithmetically, before the pointer is read or anything is allocated
    too_many = _lib.MMC_TARGETSET_MAX_CELLS // K7 + 1
    status = lib.mmc_targetset_append(store._handle(), good.ctypes.data, too_many, _lib.MMC_IN_HOST, None)
    assert status == MMC_ERR_ARG and "MMC_TARGETSET_MAX_CELLS" in _err() and len(store) == 71
    h = C.c_void_p()
    assert lib.mmc_targetset_create(K7, 0, too_many, C.byref(h)) == MMC_ERR_ARG and "MMC_TARGETSET_MAX_CELLS" in _err() and not h.value
    refused(MMC_ERR_ARG)                                           # and the trainer is where it was
    for hnd in (store, ts_k, ts_n, fsn, ens):
        hnd.close()
    raw.close()


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------------
def test_sweep_to_ensemble_to_distilled_artifact(data, tmp_path):
    from mermaid_classifier_amd import (FeatureSet, HeadEnsemble, SweepConfig, distill, export_artifact, load_predictor, train_sweep)
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    classes = list(range(K7))
    X, y = data["X"], data["y"]
    train = FeatureSet(NF, classes).append(X[:150], y[:150])
    ref = FeatureSet(NF, classes).append(X[150:190], y[150:190])
    val = FeatureSet(NF, classes).append(X[190:], y[190:])
    configs = [SweepConfig(hidden_layer_sizes=(9,), learning_rate_init=lr, random_state=s) for lr, s in ((1e-2, 0), (3e-3, 1), (1e-3, 2))]
    results = train_sweep(train, ref, val, configs, 2, batch_size=50)
    ens = HeadEnsemble.from_sweep(results, val, top=3)
    student = TorchMLPClassifier(hidden_layer_sizes=(9,), learning_rate_init=1e-2, random_state=0, distill_alpha=0.7, distill_temperature=2.0)
    cal, info, accs = distill(ens, train, ref, val, 2, batch_size=50, alpha=0.7, temperature=2.0, clf=student)
    assert info["final_epoch"] == 2 and len(accs) == 2
    export_artifact(cal, tmp_path / "student", X[:20])
    back = load_predictor(tmp_path / "student" / "model.pt", tmp_path / "student" / "model.json")
    assert np.array_equal(back.predict_proba(X[190:]), cal.predict_proba(X[190:]))
    # label-only and distilled students side by side on one shared target set
    pair = [SweepConfig(hidden_layer_sizes=(9,), learning_rate_init=1e-2, random_state=0),
            SweepConfig(hidden_layer_sizes=(9,), learning_rate_init=1e-2, random_state=0, distill_alpha=0.7, distill_temperature=2.0)]
    with_teacher = train_sweep(train, ref, val, pair, 2, batch_size=50, teacher=ens)
    without = train_sweep(train, ref, val, pair[:1], 2, batch_size=50)
    for a, b in zip(with_teacher[0][0].weights + with_teacher[0][0].biases, without[0][0].weights + without[0][0].biases):
        assert np.array_equal(bits(a), bits(b))
    # the distilled member is the student of distill(): same configuration, same teacher, same bits
    for a, b in zip(with_teacher[1][0].weights + with_teacher[1][0].biases, cal.weights + cal.biases):
        assert np.array_equal(bits(a), bits(b))
    assert not np.array_equal(bits(with_teacher[1][0].weights[0]), bits(without[0][0].weights[0]))
    with pytest.raises(ValueError, match="targets or teacher, not both"):
        train_sweep(train, ref, val, pair, 1, batch_size=50, teacher=ens, targets=data["ts_a"])
    for h in (train, ref, val, ens):
        h.close()
