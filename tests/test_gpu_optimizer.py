"""-m gpu: the trainer's optimiser options (include/mmc.h, "optimiser options"; ``csrc/trainer.hip``): learning-rate schedule,
gradient-norm clipping, averaged (EMA) weights.

Bit for bit where the definition fixes the bits -- the defaults against an untouched trainer, a scheduled step against a plain
trainer created with that step's rate, a non-clipping ``max_norm`` against the unclipped step, the clipped gradient against
``fl(g coef)`` of the reported norm, the shadow against a numpy float32 replay, averaged-mode evaluation against a plain trainer
holding the shadow, group against solo under two chunk sizes, resume, rejections -- and against the float64 reference of
``tests/optimizer_checker.py`` where the device's summation order is its own: the norm within 1 x the derived bound, the clipped
gradient per element within 2 x.  Layer widths (1028, 65, 130) with K = 5 and K = 108, mini-batches of 67, three steps with a ragged
last one; a step is observed through ``beta1 = 0`` one-step passes, as in ``tests/test_gpu_trainer_step.py``.

Measured max |got - ref| / bound per case and tensor: ``profiles/optimizer_options.txt`` (written per test into the directory
``MMC_OPTIMIZER_PARITY_OUT`` names)."""

import ctypes as C
import os
import pickle

import numpy as np
import pytest

import optimizer_checker as oc
from oracle import mlp_step_ref as sr
from test_gpu_regularizers import _T, _fs, _group_call
from test_gpu_trainer_step import _named

from mermaid_classifier_amd import optim

pytestmark = pytest.mark.gpu

FACTOR = 2.0
MB, N3 = oc.MB, oc.ROWS
CONSTANT, LINEAR, COSINE = 0, 1, 2
RAW, AVERAGED = 0, 1
F32 = np.float32


class _O(_T):
    """``_T`` plus the optimiser options' entry points."""

    def set_schedule(self, kind, warmup, total, ratio):
        return self.lib.mmc_trainer_set_lr_schedule(self.h, kind, warmup, total, ratio)

    def lr_at(self, step):
        out = C.c_double(np.nan)
        self._lib.check(self.lib.mmc_trainer_lr_at(self.h, step, C.byref(out)))
        return out.value

    def set_clip(self, max_norm):
        return self.lib.mmc_trainer_set_grad_clip(self.h, max_norm)

    def grad_norms(self):
        steps = C.c_int(-1)
        self._lib.check(self.lib.mmc_trainer_grad_norms(self.h, None, 0, C.byref(steps)))
        out = np.full(steps.value, np.nan, F32)
        if steps.value:
            self._lib.check(self.lib.mmc_trainer_grad_norms(self.h, out.ctypes.data, steps.value, C.byref(steps)))
        return out

    def set_ema(self, decay):
        return self.lib.mmc_trainer_set_ema(self.h, decay)

    def ema_status(self, set_, ws, bs):
        return self.lib.mmc_trainer_ema_state(self.h, set_, self._pa(ws), self._pa(bs))

    def shadow(self):
        ws, bs = self._empty()
        self._lib.check(self.ema_status(0, ws, bs))
        return ws + bs

    def eval_weights(self, which):
        return self.lib.mmc_trainer_eval_weights(self.h, which)

    def options(self):
        kind, which = C.c_int(-1), C.c_int(-1)
        warm, total = C.c_longlong(-1), C.c_longlong(-1)
        ratio, max_norm, decay = C.c_double(np.nan), C.c_double(np.nan), C.c_double(np.nan)
        self._lib.check(self.lib.mmc_trainer_optimizer_options(self.h, C.byref(kind), C.byref(warm), C.byref(total), C.byref(ratio),
                                                               C.byref(max_norm), C.byref(decay), C.byref(which)))
        return kind.value, warm.value, total.value, ratio.value, max_norm.value, decay.value, which.value

    def full_state(self):
        """``state()`` plus the shadow (or None) and the last pass's norms."""
        decay = self.options()[5]
        return self.state() + (self.shadow() if decay else None, self.grad_norms())


def _same(a, b):
    """Two ``state()`` / ``full_state()`` tuples, bit for bit."""
    if a[3] != b[3] or len(a) != len(b):
        return False
    lists = list(zip(a[:3], b[:3]))
    if len(a) > 4:
        if (a[4] is None) != (b[4] is None):
            return False
        if a[4] is not None:
            lists.append((a[4], b[4]))
        if not np.array_equal(a[5], b[5]):
            return False
    return all(len(u) == len(v) and all(np.array_equal(p, q) for p, q in zip(u, v)) for u, v in lists)


def _finish(name, lines, failures):
    print("\n".join(lines))
    out_dir = os.environ.get("MMC_OPTIMIZER_PARITY_OUT")          # tools: keep the table (profiles/optimizer_options.txt)
    if out_dir:
        with open(os.path.join(out_dir, f"optimizer_parity_{name}.txt"), "w") as f:
            f.write("\n".join(lines + failures) + "\n")
    assert not failures, "\n".join(failures)


@pytest.fixture(scope="module")
def cases():
    """K -> (weights, biases, class weights, X, y, visit) of ``optimizer_checker.make_case``, read only; and the float64 step of the
    first mini-batch, computed once."""
    out = {}
    for K in (5, 108):
        ws, bs, cw, X, y = oc.make_case(K)
        visit = np.arange(N3, dtype=np.int64)
        for a in (X, y, visit) + ((cw,) if cw is not None else ()):
            a.setflags(write=False)
        out[K] = (ws, bs, cw, X, y, visit, sr.step_ref(ws, bs, X[:MB], y[:MB], oc.ALPHA, cw))
    return out


def _moments_like(ws, bs, seed):
    rng = np.random.default_rng([31, seed])
    p = ws + bs
    m = [(1e-3 * rng.standard_normal(a.shape)).astype(F32) for a in p]
    v = [rng.uniform(1e-9, 1e-5, a.shape).astype(F32) for a in p]
    return m, v


# ---- 1. the defaults --------------------------------------------------------------------------------------------------------------------
def test_off_values_give_the_bits_of_an_untouched_trainer(cases):
    ws, bs, cw, X, y, visit, _ = cases[5]
    fs = _fs(X, y)
    a, b = _O(ws, bs, cw, alpha=oc.ALPHA), _O(ws, bs, cw, alpha=oc.ALPHA)
    try:
        assert b.set_schedule(COSINE, 3, 9, 0.5) == 0 and b.set_clip(0.25) == 0 and b.set_ema(0.9) == 0     # on, then off again
        assert b.set_schedule(CONSTANT, 0, 0, 0.0) == 0 and b.set_clip(0.0) == 0 and b.set_ema(0.0) == 0
        assert b.options() == (CONSTANT, 0, 0, 0.0, 0.0, 0.0, RAW) == a.options()
        avg_a, avg_b = a.fit_set(fs, visit, MB), b.fit_set(fs, visit, MB)
        sa, sb = a.state(), b.state()
        assert len(b.grad_norms()) == 0
    finally:
        a.close()
        b.close()
        fs.close()
    assert sa[3] == 3 and _same(sa, sb) and avg_a == avg_b and np.isfinite(avg_a)


# ---- 2. the schedule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [LINEAR, COSINE], ids=["linear", "cosine"])
def test_scheduled_step_is_a_plain_step_at_that_rate(cases, kind):
    """Warm-up 4, decay to step 12, final ratio 0.1: step 2 (warm-up), step 8 (mid-decay) and step 15 (past the end)."""
    ws, bs, cw, X, y, _, _ = cases[108]
    m0, v0 = _moments_like(ws, bs, kind)
    L, lr = len(ws), 1e-3
    sched = _O(ws, bs, cw, lr=lr, alpha=oc.ALPHA)
    rates = []
    try:
        assert sched.set_schedule(kind, 4, 12, 0.1) == 0
        for s in (2, 8, 15):
            rate = sched.lr_at(s)
            rates.append(rate)
            plain = _O(ws, bs, cw, lr=rate, alpha=oc.ALPHA)
            twin = _O(ws, bs, cw, lr=lr, alpha=oc.ALPHA)
            try:
                assert twin.set_schedule(kind, 4, 12, 0.1) == 0
                for t in (plain, twin):
                    t.set_moments(0, m0[:L], m0[L:], s - 1)
                    t.set_moments(1, v0[:L], v0[L:], s - 1)
                rows = slice(0, MB) if s != 15 else slice(2 * MB, N3)          # the ragged mini-batch too
                (st_p, avg_p), (st_t, avg_t) = plain.fit(X[rows], y[rows], MB), twin.fit(X[rows], y[rows], MB)
                assert st_p == st_t == 0
                sp, stw = plain.state(), twin.state()
            finally:
                plain.close()
                twin.close()
            assert sp[3] == s and _same(sp, stw) and avg_p == avg_t, f"step {s}"
            assert not all(np.array_equal(p, q) for p, q in zip(sp[0], ws + bs))
    finally:
        sched.close()
    assert abs(rates[0] - lr * 0.5) <= 1e-18 and 0.1 * lr < rates[1] < lr and abs(rates[2] - 0.1 * lr) <= 1e-18
    for s, rate in zip((2, 8, 15), rates):
        want = optim.lr_at(s, lr, "linear" if kind == LINEAR else "cosine", 4, 12, 0.1)
        assert abs(rate - want) <= 1e-15 * want


# ---- 3. clipping -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 108])
def test_clipping_against_the_float64_reference(cases, K):
    ws, bs, cw, X, y, _, (ref, bound) = cases[K]
    L = len(ws)
    names = oc.grad_names(L)
    n_ref, n_bound = oc.norm_ref(ref, bound, L)
    max_norm = 0.37 * n_ref
    c_ref, c_bound, want, want_bound = oc.clip_ref(ref, bound, L, max_norm)
    ts = [_O(ws, bs, cw, beta1=0.0, alpha=oc.ALPHA) for _ in range(3)]
    plain, loose, tight = ts
    try:
        assert loose.set_clip(1e6 * n_ref) == 0 and tight.set_clip(max_norm) == 0
        out = [t.fit(X[:MB], y[:MB], MB) for t in ts]
        assert all(st == 0 for st, _ in out), plain.lib.mmc_last_error()
        sp, sl, st = plain.state(), loose.state(), tight.state()
        norms = [t.grad_norms() for t in ts]
    finally:
        for t in ts:
            t.close()
    lines, failures = [f"# clipping, widths {oc.dims_of(K)}, mb {MB}: float64 norm {n_ref:.9g}, max_norm {max_norm:.9g}"], []
    # the reported norm
    assert len(norms[0]) == 0 and norms[1].shape == norms[2].shape == (1,) and norms[1][0] == norms[2][0]
    norm = norms[1][0]
    lines.append(f"clip-K{K:<29d} norm    |got-ref|/bound {abs(float(norm) - n_ref) / n_bound:9.2e} (got {float(norm):.9g})")
    assert abs(float(norm) - n_ref) <= n_bound, (norm, n_ref, n_bound)
    # the summation alone: against the float64 norm of the device's own gradient, which exp_avg of the unclipped step is
    g = dict(zip(names, [a for l in range(L) for a in (sp[1][l], sp[1][L + l])]))
    own, own_bound = oc.norm_ref(g, None, L)
    lines.append(f"clip-K{K:<29d} norm    |got-own|/bound {abs(float(norm) - own) / own_bound:9.2e} (summation order alone)")
    assert abs(float(norm) - own) <= own_bound
    # max_norm above the norm: coefficient exactly 1.0f through adam_opt_kernel
    assert _same(sp, sl) and out[0][1] == out[1][1]
    # max_norm at a fraction of the norm: per element against coef_ref g_ref ...
    coef = optim.clip_coefficient(norm, max_norm)
    assert abs(float(coef) - c_ref) <= c_bound
    got = _named(st[1][:L], st[1][L:])
    for k in names:
        gk = np.asarray(got[k])
        assert gk.shape == want[k].shape and np.isfinite(gk).all()
        ratio, idx = sr.worst_ratio(gk, want[k], want_bound[k])
        lines.append(f"clip-K{K:<29d} {k:7s} max|got-ref|/bound {ratio:9.2e} at {idx}")
        over = np.abs(gk.astype(np.float64) - want[k]) > FACTOR * want_bound[k]
        if over.any():
            failures.append(f"{k}: worst element {idx}: got {float(gk[idx]):.9g} ref {float(want[k][idx]):.9g} bound "
                            f"{float(want_bound[k][idx]):.3g}; {int(over.sum())} of {over.size} over {FACTOR:g} x bound")
        # ... and bit for bit the unclipped gradient times the coefficient of the reported norm, one rounding
        assert np.array_equal(gk, g[k] * coef), k
    assert st[3] == 1 and out[2][1] == out[0][1]                                  # the loss is the pre-update loss either way
    _finish(f"clip_K{K}", lines, failures)


# ---- 4. averaged weights ------------------------------------------------------------------------------------------------------------------
def test_shadow_is_the_float32_replay_and_averaged_evaluation_reads_it(cases):
    ws, bs, cw, X, y, _, _ = cases[5]
    decay = 0.9
    fs = _fs(X, y)
    t = _O(ws, bs, cw, alpha=oc.ALPHA)
    twins = []
    lines = [f"# EMA decay {decay}, widths {oc.dims_of(5)}: shadow after each of three one-step passes against the numpy float32 replay"]
    try:
        assert t.eval_weights(AVERAGED) != 0                                    # no shadow yet
        assert t.set_ema(decay) == 0
        s = t.shadow()
        assert all(np.array_equal(a, b) for a, b in zip(s, ws + bs))            # usable from step 0
        for i, rows in enumerate((slice(0, MB), slice(MB, 2 * MB), slice(2 * MB, N3))):
            assert t.fit(X[rows], y[rows], MB)[0] == 0
            p = t.params()
            p = p[0] + p[1]
            want = [oc.ema_replay(a, b, decay) for a, b in zip(s, p)]
            s = t.shadow()
            differing = sum(int((a != b).sum()) for a, b in zip(s, want))
            lines.append(f"ema-step{i + 1:<27d} shadow  elements differing from the replay: {differing}")
            assert differing == 0
            assert not np.array_equal(s[0], p[0])
        L = len(ws)
        raw = t.params()
        z_raw = t.logits(X)                                                     # the default reads the raw weights
        assert t.eval_weights(AVERAGED) == 0
        z_avg, e_avg = t.logits(X), t.evaluate_set(fs)
        assert t.eval_weights(RAW) == 0
        z_raw2, e_raw = t.logits(X), t.evaluate_set(fs)
        got_raw = t.params()
        twins = [_O(s[:L], s[L:], cw), _O(raw[0], raw[1], cw)]
        z_s, e_s = twins[0].logits(X), twins[0].evaluate_set(fs)
        z_r, e_r = twins[1].logits(X), twins[1].evaluate_set(fs)
        # writing the shadow: what ema_state(set = 1) stores is what the averaged forward reads
        assert t.ema_status(1, raw[0], raw[1]) == 0 and t.eval_weights(AVERAGED) == 0
        z_set = t.logits(X)
        assert t.set_ema(0.0) == 0 and t.options()[6] == RAW and t.eval_weights(AVERAGED) != 0
    finally:
        t.close()
        for tw in twins:
            tw.close()
        fs.close()
    assert np.isfinite(z_avg).all() and np.array_equal(z_avg, z_s) and e_avg == e_s
    assert np.array_equal(z_raw, z_r) and np.array_equal(z_raw2, z_r) and e_raw == e_r and not np.array_equal(z_avg, z_raw)
    assert all(np.array_equal(a, b) for a, b in zip(got_raw[0] + got_raw[1], raw[0] + raw[1]))
    assert np.array_equal(z_set, z_r)
    _finish("ema", lines, [])


def _classifier(**kw):
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    return TorchMLPClassifier(hidden_layer_sizes=(65, 130), learning_rate_init=1e-3, alpha=1e-3, random_state=0, batch_size=MB, **kw)


def _plain_from(clf, weights, biases):
    """A classifier without averaging that holds ``weights`` / ``biases`` as its raw parameters."""
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    state = {k: v for k, v in clf.__getstate__().items() if k not in ("_optimizer_state", "_eval_weights", "grad_norms_")}
    state.update(ema_decay=0.0, _module_state=([w.copy() for w in weights], [b.copy() for b in biases]))
    out = TorchMLPClassifier.__new__(TorchMLPClassifier)
    out.__setstate__(state)
    return out


def test_averaging_classifier_evaluates_and_calibrates_its_average(cases):
    from mermaid_classifier_amd import calibrate, evaluate
    ws, bs, cw, X, y, _, _ = cases[5]
    fs = _fs(X, y)
    clf = _classifier(ema_decay=0.9)
    plain = raw_twin = None
    try:
        for _ in range(2):
            clf.partial_fit_rows(fs)
        avg_w, avg_b = clf.averaged_parameters()
        raw_w, raw_b = clf.raw_parameters()
        assert not np.array_equal(avg_w[0], raw_w[0])
        got_w, got_b = clf.parameters()                                          # averaged mode is the default
        assert all(np.array_equal(a, b) for a, b in zip(got_w + got_b, avg_w + avg_b))
        plain, raw_twin = _plain_from(clf, avg_w, avg_b), _plain_from(clf, raw_w, raw_b)
        assert np.array_equal(clf.predict_proba(X), plain.predict_proba(X))
        assert evaluate(clf, fs) == evaluate(plain, fs)
        cal, cal_plain = calibrate(clf, fs), calibrate(plain, fs)
        assert all(np.array_equal(a, b) for a, b in zip(cal.weights + cal.biases, avg_w + avg_b))
        assert np.array_equal(cal.a_, cal_plain.a_) and np.array_equal(cal.b_, cal_plain.b_)
        pa, pb = cal.predict_proba(X), cal_plain.predict_proba(X)
        assert np.isfinite(pa).all() and np.array_equal(pa, pb)
        clf.use_weights("raw")                                                   # raw mode: today's result
        assert np.array_equal(clf.predict_proba(X), raw_twin.predict_proba(X)) and evaluate(clf, fs) == evaluate(raw_twin, fs)
        assert all(np.array_equal(a, b) for a, b in zip(clf.parameters()[0], raw_w))
        assert not np.array_equal(clf.predict_proba(X), plain.predict_proba(X))
    finally:
        for c in (clf, plain, raw_twin):
            if c is not None:
                c._release()
        fs.close()


# ---- 5. group equals solo ----------------------------------------------------------------------------------------------------------------
def _group_members(cases):
    ws, bs, cw, X, y, visit, _ = cases[5]
    rng = np.random.default_rng(55)
    live = int(np.flatnonzero(cw > 0)[0])
    anchor = int(np.flatnonzero(y == live)[0])
    members = []
    for i in range(5):
        v = rng.permutation(N3).astype(np.int64)
        v[[0, MB, 2 * MB]] = anchor                                              # every mini-batch carries weight
        members.append(dict(visit=v))
    members[1].update(clip=1.0)
    members[2].update(schedule=(COSINE, 1, 3, 0.1), ema=0.9)
    members[3].update(schedule=(LINEAR, 2, 40, 0.0), clip=2.0, ema=0.99, drop=(0.1, 0.5))
    v = members[4]["visit"]
    members[4].update(ema=0.5, lam=np.asarray([0.3, 1.0, 0.8], F32),
                      partner=np.concatenate([v[s:s + MB][rng.permutation(len(v[s:s + MB]))] for s in range(0, N3, MB)]))
    return ws, bs, cw, X, y, members


def _make(ws, bs, cw, m):
    t = _O(ws, bs, cw, alpha=oc.ALPHA)
    if "drop" in m:
        assert t.set_dropout(*m["drop"]) == 0
    if "schedule" in m:
        assert t.set_schedule(*m["schedule"]) == 0
    if "clip" in m:
        assert t.set_clip(m["clip"]) == 0
    if "ema" in m:
        assert t.set_ema(m["ema"]) == 0
    return t


@pytest.mark.parametrize("chunk", ["67", "100000"])
def test_group_members_equal_their_solo_runs(cases, chunk, monkeypatch):
    ws, bs, cw, X, y, members = _group_members(cases)
    fs = _fs(X, y)
    solo, group = [_make(ws, bs, cw, m) for m in members], [_make(ws, bs, cw, m) for m in members]
    try:
        monkeypatch.delenv("MMC_TRAIN_CHUNK_ROWS", raising=False)
        solo_avg = []
        for t, m in zip(solo, members):
            status, avg = t.fit_set_mixed(fs, m["visit"], m.get("partner"), m.get("lam"), MB)
            assert status == 0, t.lib.mmc_last_error()
            solo_avg.append(avg)
        monkeypatch.setenv("MMC_TRAIN_CHUNK_ROWS", chunk)                       # read at every call
        status, avgs = _group_call(group, fs, [m["visit"] for m in members], [m.get("partner") for m in members],
                                   [m.get("lam") for m in members], [MB] * len(members))
        assert status == 0, group[0].lib.mmc_last_error()
        ss, gs = [t.full_state() for t in solo], [t.full_state() for t in group]
    finally:
        for t in solo + group:
            t.close()
        fs.close()
    for i, (s, g) in enumerate(zip(ss, gs)):
        assert s[3] == 3 and _same(s, g) and solo_avg[i] == avgs[i], f"member {i}"
        assert len(s[5]) == (3 if "clip" in members[i] else 0) and (s[4] is not None) == ("ema" in members[i])
    assert np.isfinite(solo_avg).all() and np.isfinite(ss[1][5]).all() and (ss[1][5] > 1.0).all()    # member 1 did clip
    assert not _same(ss[0][:4], ss[1][:4])


# ---- 6. resume ---------------------------------------------------------------------------------------------------------------------------
def test_pickled_classifier_continues_schedule_shadow_and_step(cases):
    ws, bs, cw, X, y, _, _ = cases[5]
    fs = _fs(X, y)
    kw = dict(lr_schedule="cosine", warmup_steps=2, schedule_steps=10, final_lr_ratio=0.1, max_grad_norm=0.5, ema_decay=0.9)
    a, b = _classifier(**kw), None
    try:
        for _ in range(2):
            a.partial_fit_rows(fs)
        b = pickle.loads(pickle.dumps(a))
        assert b._adam_state()["step"] == 6 and b.n_iter_ == 2
        for _ in range(2):
            a.partial_fit_rows(fs)
            b.partial_fit_rows(fs)
        pa, pb = a.raw_parameters(), b.raw_parameters()
        oa, ob = a._adam_state(), b._adam_state()
        za, zb = a.predict_proba(X), b.predict_proba(X)
    finally:
        a._release()
        if b is not None:
            b._release()
        fs.close()
    assert oa["step"] == ob["step"] == 12 and a.loss_curve_ == b.loss_curve_ and len(a.loss_curve_) == 4
    for u, v in ((pa, pb), (oa["exp_avg"], ob["exp_avg"]), (oa["exp_avg_sq"], ob["exp_avg_sq"]), (oa["ema"], ob["ema"])):
        assert all(np.array_equal(p, q) for p, q in zip(u[0] + u[1], v[0] + v[1]))
    assert np.array_equal(a.grad_norms_, b.grad_norms_) and a.grad_norms_.shape == (3,) and np.array_equal(za, zb)
    assert not np.array_equal(oa["ema"][0][0], pa[0][0])


# ---- 7. rejections -----------------------------------------------------------------------------------------------------------------------
def test_rejected_setters_change_nothing(cases):
    from mermaid_classifier_amd import _lib
    ws, bs, cw, X, y, _, _ = cases[5]
    t, bare = _O(ws, bs, cw, alpha=oc.ALPHA), _O(ws, bs, cw, alpha=oc.ALPHA)
    nan, inf = float("nan"), float("inf")
    try:
        assert t.set_schedule(LINEAR, 2, 40, 0.25) == 0 and t.set_clip(1.5) == 0 and t.set_ema(0.9) == 0 and t.eval_weights(AVERAGED) == 0
        assert t.fit(X[:MB], y[:MB], MB)[0] == 0
        before, options = t.full_state(), t.options()
        assert options == (LINEAR, 2, 40, 0.25, 1.5, 0.9, AVERAGED) and before[3] == 1

        def rejected(status, text):
            assert status == _lib.MMC_ERR_ARG and text in t.lib.mmc_last_error().decode(), (status, t.lib.mmc_last_error())
            assert t.options() == options and _same(t.full_state(), before)

        for args, text in (((3, 0, 10, 0.0), "kind"), ((-1, 0, 10, 0.0), "kind"), ((COSINE, -1, 10, 0.0), "warmup_steps"),
                           ((CONSTANT, -5, 0, 0.0), "warmup_steps"), ((LINEAR, 10, 10, 0.0), "total_steps"),
                           ((COSINE, 10, 3, 0.0), "total_steps"), ((LINEAR, 0, 10, -0.5), "final_ratio"),
                           ((COSINE, 0, 10, 1.5), "final_ratio"), ((CONSTANT, 0, 0, nan), "final_ratio")):
            rejected(t.set_schedule(*args), text)
        for v in (-1.0, inf, nan, 1e39, 1e-50):
            rejected(t.set_clip(v), "max_norm")
        for v in (1.0, -0.1, 1.5, nan):
            rejected(t.set_ema(v), "decay")
        rejected(t.eval_weights(2), "which")
        rejected(t.eval_weights(-1), "which")
        w0, b0 = bare._empty()
        assert bare.eval_weights(AVERAGED) == _lib.MMC_ERR_ARG and bare.ema_status(0, w0, b0) == _lib.MMC_ERR_ARG
        assert bare.options() == (CONSTANT, 0, 0, 0.0, 0.0, 0.0, RAW)
        assert t.lr_at(1) == 1e-3 * 0.5 * (1.0 - 0.75 * 0.0) and t.lr_at(40) == 1e-3 * 0.25
    finally:
        t.close()
        bare.close()


# ---- 8. end to end -------------------------------------------------------------------------------------------------------------------------
def test_sweep_with_a_default_member_and_one_with_every_option():
    from mermaid_classifier_amd import FeatureSet, SweepConfig, train_classifier, train_sweep
    rng = np.random.default_rng(12)
    centres = rng.standard_normal((4, 68))
    y = np.arange(240) % 4
    X = (centres[y] + 0.7 * rng.standard_normal((240, 68))).astype(F32)
    sets = [FeatureSet(68, [0, 1, 2, 3]).append(X[s], y[s]) for s in (slice(0, 160), slice(160, 200), slice(200, 240))]
    base = dict(hidden_layer_sizes=(65,), learning_rate_init=1e-2, random_state=0, batch_size=MB)
    opts = dict(lr_schedule="cosine", warmup_steps=2, final_lr_ratio=0.1, max_grad_norm=0.05, ema_decay=0.8)
    configs = [SweepConfig(**base), SweepConfig(**base, **opts)]
    own = configs[1].classifier(sets[1].device)
    try:
        seen = []
        got = train_sweep(*sets, configs, 2, batch_size=160, on_epoch_end=seen.append)
        solo0 = train_classifier(*sets, 2, batch_size=160, clf=configs[0].classifier(sets[1].device))
        solo1 = train_classifier(*sets, 2, batch_size=160, clf=own)
        assert own.schedule_steps == 2 * 3                                       # filled in: two epochs of three steps
        avg_w, avg_b = own.averaged_parameters()
        raw_w, _ = own.raw_parameters()
        norms = own.grad_norms_
    finally:
        own._release()
        for s in sets:
            s.close()
    assert len(got) == 2 and len(seen) == 4
    assert all(np.isfinite(m["training_loss"]) and np.isfinite(m["val_loss"]) for m in seen)
    for mine, solo in ((got[0], solo0), (got[1], solo1)):
        for u, v in zip(mine[0].weights + mine[0].biases, solo[0].weights + solo[0].biases):
            assert np.array_equal(u, v)
        assert np.array_equal(mine[0].a_, solo[0].a_) and np.array_equal(mine[0].b_, solo[0].b_) and mine[2] == solo[2]
    for u, v in zip(got[1][0].weights + got[1][0].biases, avg_w + avg_b):        # the calibrated model holds the averaged weights
        assert np.array_equal(u, v)
    assert not np.array_equal(got[1][0].weights[0], raw_w[0]) and not np.array_equal(got[1][0].weights[0], got[0][0].weights[0])
    assert norms.shape == (3,) and (norms > 0.05).all()
