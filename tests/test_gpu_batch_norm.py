"""Batch normalisation in the MLP trainer on the device (include/mmc.h, "batch normalisation"; ``mmc_trainer_set_batch_norm``).

1. ``mmc_trainer_norm_stage`` -- the step's ``bn_forward_kernel`` and ``bn_backward_kernel`` -- per element against the float64 checker
   within the bounds of tests/batch_norm_checker.py (tests/test_batch_norm_host.py shows an fp32 evaluation in the kernels' order stays
   within half of them and wrong kernels miss them by orders of magnitude), the running statistics of one real step likewise.
2. Training against a torch-CPU fp32 loop of ``Linear -> BatchNorm1d -> ReLU`` within the tolerances of tests/test_trainer.py (weights
   2e-5, loss curve 1e-5; the torch fp32 and fp64 loops differ by under a tenth of them).
3. The fold per element against the float64 fold of the device's own state; eval-mode logits against a plain trainer made of the folded
   parameters, bit for bit; the frozen biases.
4. Everything else is bit equality: host-fed against resident, grouped against solo, two chunk sizes, pickled twin against original,
   ``set_batch_norm(0)`` against never called, a rejected call against none.
5. End to end: ``train_classifier`` -> ``export_artifact`` -> ``load_predictor``, and a sweep of plain and normalised heads."""

import ctypes as C
import pickle

import numpy as np
import pytest

import batch_norm_checker as ck

pytestmark = pytest.mark.gpu

F32 = np.float32
K7, NF, N = ck.K7, ck.NF, ck.NROWS


class _Raw:
    """An ``mmc_trainer`` through the C ABI alone."""

    def __init__(self, weights, biases, class_weight=None, lr=1e-3, alpha=1e-3):
        from mermaid_classifier_amd import _lib
        from mermaid_classifier_amd.torch_classifier import _ptr_array
        self.lib, self._lib, self._pa = _lib.lib(), _lib, _ptr_array
        self.shapes = [w.shape for w in weights]
        self.dims = [weights[0].shape[1]] + [w.shape[0] for w in weights]
        self.h = C.c_void_p()
        cw = None if class_weight is None else np.ascontiguousarray(class_weight, F32)
        _lib.check(self.lib.mmc_trainer_create(_ptr_array(weights), _ptr_array(biases), (C.c_int * len(self.dims))(*self.dims), len(weights),
                                               lr, 0.9, 0.999, 1e-8, alpha, None if cw is None else cw.ctypes.data_as(C.POINTER(C.c_float)),
                                               0, C.byref(self.h)))

    def set_bn(self, enable=1, eps=1e-5, mom=0.1):
        return self.lib.mmc_trainer_set_batch_norm(self.h, enable, eps, mom)

    def bn_state(self, arrays=None):
        """Read (None) or write the eight per-layer lists: gamma, beta, rm, rv, m_gamma, v_gamma, m_beta, v_beta."""
        write = arrays is not None
        if not write:
            arrays = [[np.empty(n, F32) for n in self.dims[1:-1]] for _ in range(8)]
        self._lib.check(self.lib.mmc_trainer_batch_norm_state(self.h, int(write), *[self._pa(a) for a in arrays]))
        return arrays

    def norm_stage(self, layer, Z, dA):
        Z, dA = np.ascontiguousarray(Z, F32), np.ascontiguousarray(dA, F32)
        M, n = Z.shape
        out = dict(H=np.full((M, n), np.nan, F32), dZ=np.full((M, n), np.nan, F32), g_gamma=np.full(n, np.nan, F32),
                   g_beta=np.full(n, np.nan, F32), mu=np.full(n, np.nan, F32), v=np.full(n, np.nan, F32))
        status = self.lib.mmc_trainer_norm_stage(self.h, layer, Z.ctypes.data, dA.ctypes.data, M, out["H"].ctypes.data, out["dZ"].ctypes.data,
                                                 out["g_gamma"].ctypes.data, out["g_beta"].ctypes.data, out["mu"].ctypes.data,
                                                 out["v"].ctypes.data, None)
        return status, out

    def _empty(self):
        return [np.empty(s, F32) for s in self.shapes], [np.empty(s[0], F32) for s in self.shapes]

    def params(self, folded=False):
        ws, bs = self._empty()
        fn = self.lib.mmc_trainer_folded_params if folded else self.lib.mmc_trainer_get_params
        self._lib.check(fn(self.h, self._pa(ws), self._pa(bs)))
        return ws, bs

    def partial_fit(self, X, y, batch_size):
        avg = C.c_double(0.0)
        X, y32 = np.ascontiguousarray(X, F32), np.ascontiguousarray(y, np.int32)
        status = self.lib.mmc_trainer_partial_fit(self.h, X.ctypes.data, y32.ctypes.data, len(y32), batch_size, C.byref(avg), None)
        return status, avg.value

    def fit_set(self, fs, visit, batch_size):
        avg = C.c_double(0.0)
        v = np.ascontiguousarray(visit, np.int64)
        status = self.lib.mmc_trainer_partial_fit_set(self.h, fs._handle(), v.ctypes.data, len(v), batch_size, C.byref(avg), None)
        return status, avg.value

    def logits(self, X):
        X = np.ascontiguousarray(X, F32)
        out = np.empty((len(X), self.dims[-1]), F32)
        self._lib.check(self.lib.mmc_trainer_logits(self.h, X.ctypes.data, len(X), out.ctypes.data, None))
        return out

    def state(self, bn=True):
        """Every array the trainer owns, and its step count."""
        out = [a for part in self.params() for a in part]
        step = C.c_longlong(0)
        for which in (0, 1):
            ws, bs = self._empty()
            self._lib.check(self.lib.mmc_trainer_adam_state(self.h, which, 0, self._pa(ws), self._pa(bs), C.byref(step)))
            out += ws + bs
        if bn:
            out += [a for part in self.bn_state() for a in part]
        return out, int(step.value)

    def close(self):
        self.lib.mmc_trainer_destroy(self.h)


def _same(a, b):
    (pa, sa), (pb, sb) = a, b
    return sa == sb and len(pa) == len(pb) and all(np.array_equal(u, v) for u, v in zip(pa, pb))


def _group_fit(trainers, fs, visits, batch_sizes):
    lib = trainers[0].lib
    count = len(trainers)
    vs = [np.ascontiguousarray(v, np.int64) for v in visits]
    avg = (C.c_double * count)()
    status = lib.mmc_trainer_group_partial_fit_set((C.c_void_p * count)(*[t.h for t in trainers]), count, fs._handle(),
                                                   (C.c_void_p * count)(*[v.ctypes.data for v in vs]), (C.c_int64 * count)(*[len(v) for v in vs]),
                                                   (C.c_int * count)(*batch_sizes), avg, None)
    return status, list(avg)


def _head(rng, dims):
    ws = [(rng.normal(0, 1, (o, i)) * np.sqrt(2.0 / i)).astype(F32) for i, o in zip(dims[:-1], dims[1:])]
    bs = [rng.normal(0, 0.1, o).astype(F32) for o in dims[1:]]
    return ws, bs


@pytest.fixture(scope="module")
def data():
    return ck.train_data()


# ---- 1. the stage per element --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_", ck.NS)
def test_norm_stage_per_element_against_the_fp64_checker(N_):
    rng = np.random.default_rng(N_)
    raw = _Raw(*_head(rng, [4, N_, 3]))
    try:
        assert raw.set_bn() == 0, raw.lib.mmc_last_error()
        for M in ck.MBS:
            Z, dA, gamma, beta, rm, rv = ck.stage_case(M, N_)
            arrays = raw.bn_state()
            arrays[0][0][:], arrays[1][0][:] = gamma, beta
            raw.bn_state(arrays)
            before = raw.state()
            status, got = raw.norm_stage(0, Z, dA)
            assert status == 0, raw.lib.mmc_last_error()
            assert _same(before, raw.state())                                  # the hook touches no state
            want, bound = ck.stage_ref(Z, dA, gamma, beta, rm, rv)
            assert all(np.isfinite(a).all() for a in got.values())
            peaks = {k: ck.peak(got[k], want[k], bound[k]) for k in got}
            print(f"mb {M:3d} N {N_:3d} peak error / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in peaks.items()))
            assert max(peaks.values()) <= 1.0, (M, peaks)
            if N_ >= 7:
                assert got["v"][ck.CONST_COL] <= bound["v"][ck.CONST_COL] and (got["H"][:, ck.DEAD_COL] == 0).all()
                assert got["v"][ck.STIFF_COL] > 0
        from mermaid_classifier_amd import _lib
        for layer, rows in ((1, 5), (-1, 5), (0, 1)):
            Z = np.zeros((rows, N_), F32)
            assert raw.norm_stage(layer, Z, Z)[0] == _lib.MMC_ERR_ARG
    finally:
        raw.close()


def test_running_statistics_of_one_step_against_the_checker():
    rng = np.random.default_rng(3)
    dims = [16, 65, 7]
    ws, bs = _head(rng, dims)
    X = rng.normal(0, 1, (203, 16)).astype(F32)
    y = rng.integers(0, 7, 203)
    raw = _Raw(ws, bs)
    try:
        mom = 0.25
        assert raw.set_bn(1, 1e-3, mom) == 0
        arrays = raw.bn_state()
        arrays[2][0][:] = rng.normal(0, 1, 65).astype(F32)
        arrays[3][0][:] = rng.uniform(0.5, 2, 65).astype(F32)
        raw.bn_state(arrays)
        rm0, rv0 = arrays[2][0].copy(), arrays[3][0].copy()
        assert raw.partial_fit(X, y, 203)[0] == 0
        after = raw.bn_state()
        Z64 = X.astype(np.float64) @ ws[0].astype(np.float64).T + bs[0]
        Z = Z64.astype(F32)
        want, bound = ck.stage_ref(Z, np.zeros_like(Z), np.ones(65), np.zeros(65), rm0, rv0, eps=1e-3, mom=mom)
        # the step's Z is the GEMM's, not the rounded float64 product: 16 terms and the bias, one ulp of the sum of magnitudes each, moves
        # mu by its mean and v by 2 mean(|z - mu| dz)
        gemm = 17 * ck.ULP * (np.abs(X.astype(np.float64)) @ np.abs(ws[0].astype(np.float64)).T + np.abs(bs[0]))
        slack_m = mom * gemm.mean(axis=0)
        slack_v = mom * 2 * (np.abs(Z64 - Z64.mean(axis=0)) * gemm).mean(axis=0) * 203 / 202
        pm, pv = ck.peak(after[2][0], want["rm"], bound["rm"] + slack_m), ck.peak(after[3][0], want["rv"], bound["rv"] + slack_v)
        print(f"running statistics after one step: peak error / bound  rm {pm:.3f}  rv {pv:.3f}")
        assert pm <= 1.0 and pv <= 1.0
    finally:
        raw.close()


# ---- 2. training against torch -------------------------------------------------------------------------------------------------------
def _make(data, kind="plain", lr=1e-3, **kw):
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    opts = ck.TRAIN_KINDS[kind]
    args = dict(hidden_layer_sizes=(24, 12), learning_rate_init=lr, alpha=1e-3, random_state=0, batch_size=ck.BATCH, batch_norm=True,
                class_weight=data["cw"] if opts.get("weighted") else None, label_smoothing=opts.get("label_smoothing", 0.0),
                max_grad_norm=opts.get("max_norm"), lr_schedule=opts.get("schedule", "constant"),
                schedule_steps=15 if opts.get("schedule") else None)
    args.update(kw)
    return TorchMLPClassifier(**args)


def _clf_state(clf):
    s = clf._adam_state()
    arrays = [a.copy() for part in clf.raw_parameters() for a in part] + [a.copy() for part in clf.parameters() for a in part]
    arrays += [a.copy() for key in ("exp_avg", "exp_avg_sq") for part in s[key] for a in part]
    arrays += [a.copy() for group in s.get("batch_norm", []) for a in group]
    return arrays, (s["step"], list(clf.loss_curve_), clf.n_iter_)


@pytest.mark.parametrize("kind", list(ck.TRAIN_KINDS))
def test_training_matches_torch_on_both_routes(data, kind):
    import torch
    from mermaid_classifier_amd import FeatureSet
    want = ck.torch_loop(data, torch.float32, **ck.TRAIN_KINDS[kind])
    host, resident = _make(data, kind), _make(data, kind)
    fs = FeatureSet(NF, np.arange(K7)).append(data["X"], data["y"])
    try:
        for _ in range(3):
            host.partial_fit(data["X"], data["y"], classes=list(range(K7)))
            resident.partial_fit_rows(fs, classes=list(range(K7)))
        ws, bs = host.raw_parameters()
        st = host.batch_norm_state()
        got = dict(curve=host.loss_curve_, W=ws, b=bs, gamma=st["gamma"], beta=st["beta"], rm=st["running_mean"], rv=st["running_var"])
        dw, dl = ck.train_gap(got, want)
        print(f"{kind}: against torch fp32: parameters and statistics {dw:.2e} (tolerance {ck.W_TOL:g}), loss curve {dl:.2e} ({ck.LOSS_TOL:g})")
        assert dw <= ck.W_TOL and dl <= ck.LOSS_TOL
        assert host._adam_state()["step"] == 15                                # 50, 50, 50, 50, 30 rows
        assert _same(_clf_state(host), _clf_state(resident))                   # host-fed against resident rows
        w0, b0 = ck.initial_parameters()
        assert all(np.array_equal(b, z) for b, z in zip(bs[:-1], b0[:-1]))     # the frozen biases
        # evaluation reads the folded stack
        fw, fb = host.parameters()
        logits = data["X"][:9].astype(np.float64)
        for l, (w, b) in enumerate(zip(fw, fb)):
            logits = logits @ w.T.astype(np.float64) + b
            if l < 2:
                logits = np.maximum(logits, 0)
        p = np.exp(logits - logits.max(axis=1, keepdims=True))
        assert np.abs(host.predict_proba(data["X"][:9]) - p / p.sum(axis=1, keepdims=True)).max() < 1e-5
    finally:
        fs.close()
        host._release()
        resident._release()


# ---- 3. the fold ---------------------------------------------------------------------------------------------------------------------
def test_fold_per_element_bit_equal_logits_and_frozen_biases(data):
    rng = np.random.default_rng(4)
    dims = [NF, 65, 24, K7]
    ws, bs = _head(rng, dims)
    raw = _Raw(ws, bs, lr=1e-2)
    try:
        assert raw.set_bn() == 0
        plain_w, plain_b = raw.params(folded=True)                             # fresh: gamma 1, rm 0, rv 1 -> s = 1 / sqrt(1 + eps)
        assert not np.array_equal(plain_w[0], ws[0]) and np.array_equal(plain_w[2], ws[2])
        for _ in range(2):
            assert raw.partial_fit(data["X"], data["y"], 50)[0] == 0
        rw, rb = raw.params()
        assert all(np.array_equal(b, b0) for b, b0 in zip(rb[:-1], bs[:-1])) and not np.array_equal(rb[-1], bs[-1])
        assert not np.array_equal(rw[0], ws[0])
        gamma, beta, rm, rv = raw.bn_state()[:4]
        assert not np.array_equal(gamma[0], np.ones(65, F32)) and not np.array_equal(rm[1], np.zeros(24, F32))
        fw, fb = raw.params(folded=True)
        want_w, want_b, ew, eb = ck.fold_ref(rw, rb, gamma, beta, rm, rv)
        peaks = [max(ck.peak(fw[l], want_w[l], ew[l]), ck.peak(fb[l], want_b[l], eb[l])) for l in range(3)]
        print("fold peak error / bound per layer:", [f"{p:.3f}" for p in peaks])
        assert max(peaks) <= 1.0
        from mermaid_classifier_amd import fold_batch_norm
        hw, hb = fold_batch_norm(rw, rb, gamma, beta, rm, rv, 1e-5)            # the host mirror: the same operations
        assert all(ck.peak(a, w, e) <= 1.0 for a, w, e in zip(hw + hb, want_w + want_b, ew + eb))
        twin = _Raw(fw, fb)
        try:
            X = data["X"][:97]
            assert np.array_equal(raw.logits(X), twin.logits(X))
            assert np.array_equal(twin.params(folded=True)[0][0], fw[0])        # without the option: get_params
        finally:
            twin.close()
    finally:
        raw.close()


# ---- 4. bit equalities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", ["100", "150"])
def test_grouped_equals_solo_whatever_the_chunk(data, chunk, monkeypatch):
    from mermaid_classifier_amd import FeatureSet
    rng = np.random.default_rng(8)
    heads = [_head(rng, [NF, 24, 12, K7]), _head(rng, [NF, 65, K7]), _head(rng, [NF, 30, K7])]
    normalised = [True, False, True]
    visits = [rng.permutation(N)[:n] for n in (230, 230, 203)]
    sizes = [50, 50, 67]
    fs = FeatureSet(NF, np.arange(K7)).append(data["X"], data["y"])

    def make():
        ts = [_Raw(*h, lr=3e-3) for h in heads]
        for t, bn in zip(ts, normalised):
            assert not bn or t.set_bn() == 0
        return ts
    solo, group = make(), make()
    try:
        monkeypatch.delenv("MMC_TRAIN_CHUNK_ROWS", raising=False)
        solo_avg = []
        for _ in range(2):
            solo_avg = [t.fit_set(fs, v, mb) for t, v, mb in zip(solo, visits, sizes)]
        assert all(s == 0 for s, _ in solo_avg), solo[0].lib.mmc_last_error()
        monkeypatch.setenv("MMC_TRAIN_CHUNK_ROWS", chunk)                      # read at every call
        for _ in range(2):
            status, avgs = _group_fit(group, fs, visits, sizes)
            assert status == 0, group[0].lib.mmc_last_error()
        assert avgs == [a for _, a in solo_avg]
        for s, g, bn in zip(solo, group, normalised):
            assert _same(s.state(bn), g.state(bn))
            assert all(np.array_equal(u, v) for u, v in zip(s.params(folded=True)[0], g.params(folded=True)[0]))
    finally:
        fs.close()
        for t in solo + group:
            t.close()


def test_pickled_twin_continues_bit_for_bit(data):
    from mermaid_classifier_amd import FeatureSet
    clf = _make(data, "weights_clip_cosine", lr=3e-3, schedule_steps=40)
    fs = FeatureSet(NF, np.arange(K7)).append(data["X"], data["y"])
    try:
        clf.partial_fit_rows(fs, classes=list(range(K7)))
        twin = pickle.loads(pickle.dumps(clf))
        assert _same(_clf_state(clf), _clf_state(twin))
        for c in (clf, twin):
            c.partial_fit_rows(fs)
            c.partial_fit(data["X"], data["y"])
        assert _same(_clf_state(clf), _clf_state(twin))
        assert np.array_equal(clf.predict_proba(data["X"][:20]), twin.predict_proba(data["X"][:20]))
        twin._release()
    finally:
        fs.close()
        clf._release()


def test_disabled_is_the_trainer_it_was_never_called_on(data):
    rng = np.random.default_rng(9)
    head = _head(rng, [NF, 24, 12, K7])
    never, off, back = _Raw(*head), _Raw(*head), _Raw(*head)
    try:
        assert off.set_bn(0, 0.0, 0.0) == 0                                    # the scalars of a disabling call are not read
        assert back.set_bn() == 0 and back.set_bn(0) == 0
        for t in (never, off, back):
            assert t.partial_fit(data["X"], data["y"], 50)[0] == 0
        assert _same(never.state(False), off.state(False)) and _same(never.state(False), back.state(False))
        X = data["X"][:33]
        assert np.array_equal(never.logits(X), off.logits(X))
        assert all(np.array_equal(u, v) for u, v in zip(never.params(folded=True)[0], never.params()[0]))
        from mermaid_classifier_amd import _lib
        arrays = [[np.empty(n, F32) for n in (24, 12)] for _ in range(8)]
        assert never.lib.mmc_trainer_batch_norm_state(never.h, 0, *[never._pa(a) for a in arrays]) == _lib.MMC_ERR_ARG
    finally:
        for t in (never, off, back):
            t.close()


def test_rejected_calls_leave_the_state_unchanged(data):
    from mermaid_classifier_amd import FeatureSet, _lib
    rng = np.random.default_rng(10)
    head = _head(rng, [NF, 24, 12, K7])
    t, plain = _Raw(*head), _Raw(*head)
    fs = FeatureSet(NF, np.arange(K7)).append(data["X"], data["y"])
    lib = t.lib
    try:
        assert t.set_bn() == 0 and t.partial_fit(data["X"], data["y"], 50)[0] == 0
        before = t.state()
        logits = t.logits(data["X"][:17])

        def rejected(status, word):
            assert status == _lib.MMC_ERR_ARG and word in lib.mmc_last_error(), lib.mmc_last_error()
            assert _same(before, t.state()) and np.array_equal(logits, t.logits(data["X"][:17]))
        for eps, mom in ((0.0, 0.1), (-1.0, 0.1), (float("nan"), 0.1), (1e-60, 0.1), (1e-5, 0.0), (1e-5, 1.5), (1e-5, float("nan"))):
            rejected(t.set_bn(1, eps, mom), b"eps" if mom == 0.1 else b"momentum")
        rejected(lib.mmc_trainer_set_dropout(t.h, 0.0, 0.2, 1), b"batch normalisation")           # hidden dropout second
        rejected(lib.mmc_trainer_set_ema(t.h, 0.9), b"batch normalisation")                       # averaged weights second
        assert lib.mmc_trainer_set_dropout(t.h, 0.1, 0.0, 1) == 0 and lib.mmc_trainer_set_dropout(t.h, 0.0, 0.0, 0) == 0   # input dropout composes
        # a 1-row mini-batch: 201 rows at batch 200, host-fed, resident and in a group; and a batch size of 1
        rejected(t.partial_fit(data["X"][:201], data["y"][:201], 200)[0], b"at least 2 rows")
        rejected(t.fit_set(fs, np.arange(201), 200)[0], b"at least 2 rows")
        rejected(t.partial_fit(data["X"], data["y"], 1)[0], b"at least 2 rows")
        plain_before = plain.state(False)
        status, _ = _group_fit([plain, t], fs, [np.arange(201), np.arange(201)], [200, 200])
        rejected(status, b"member 1")
        assert _same(plain_before, plain.state(False))
        assert plain.partial_fit(data["X"][:201], data["y"][:201], 200)[0] == 0                    # a plain trainer takes it
        # batch normalisation second
        assert lib.mmc_trainer_set_dropout(plain.h, 0.0, 0.3, 1) == 0
        assert plain.set_bn() == _lib.MMC_ERR_ARG and b"dropout" in lib.mmc_last_error()
        assert lib.mmc_trainer_set_dropout(plain.h, 0.0, 0.0, 0) == 0 and lib.mmc_trainer_set_ema(plain.h, 0.9) == 0
        assert plain.set_bn() == _lib.MMC_ERR_ARG and b"averaged" in lib.mmc_last_error()
        assert lib.mmc_trainer_set_ema(plain.h, 0.0) == 0 and plain.set_bn() == 0
    finally:
        fs.close()
        t.close()
        plain.close()


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------
def test_train_export_predict_and_a_mixed_sweep(tmp_path):
    from mermaid_classifier_amd import FeatureSet, SweepConfig, load_predictor, train_classifier, train_sweep
    from mermaid_classifier_amd.calibration import export_artifact
    rng = np.random.default_rng(12)
    centres = rng.standard_normal((4, 68))
    y = np.arange(240) % 4
    X = (centres[y] + 0.7 * rng.standard_normal((240, 68))).astype(F32)
    sets = [FeatureSet(68, [0, 1, 2, 3]).append(X[s], y[s]) for s in (slice(0, 160), slice(160, 200), slice(200, 240))]
    base = dict(hidden_layer_sizes=(65, 24), random_state=0, batch_size=40)
    configs = [SweepConfig(**base, learning_rate_init=1e-4), SweepConfig(**base, learning_rate_init=1e-4, batch_norm=True),
               SweepConfig(**base, learning_rate_init=1e-3, batch_norm=True, max_grad_norm=1.0)]
    own = configs[2].classifier(sets[1].device)
    try:
        got = train_sweep(*sets, configs, 2, batch_size=160)
        model, info, accs = train_classifier(*sets, 2, batch_size=160, clf=own)
        fw, fb = own.parameters()
        rw, rb = own.raw_parameters()
        proba = model.predict_proba(X)
        pt, manifest, gap = export_artifact(model, tmp_path, X[:64])
        pred = load_predictor(pt, tmp_path / "model.json", device=0)
        dp = float(np.abs(pred.predict_proba(X) - proba).max())
    finally:
        own._release()
        for s in sets:
            s.close()
    print(f"end to end: exported head against the calibrated model {dp:.1e}, export gap {gap:.1e}")
    assert gap <= 1e-6 and dp <= 1e-6
    assert len(got) == 3 and all(np.isfinite(a).all() for g in got for a in g[0].weights + g[0].biases)
    for u, v in zip(got[2][0].weights + got[2][0].biases, model.weights + model.biases):          # a member of the sweep is its solo run
        assert np.array_equal(u, v)
    for u, v in zip(model.weights + model.biases, fw + fb):                                       # the calibrated model holds the folded stack
        assert np.array_equal(u, v)
    assert not np.array_equal(fw[0], rw[0]) and np.array_equal(fw[2], rw[2])
    assert not np.array_equal(got[0][0].weights[0], got[1][0].weights[0])
