"""-m gpu: dropout and mixup in the MLP trainer (include/mmc.h, "regularisers"; ``csrc/trainer.hip``, ``csrc/philox.h``).

Bit for bit where the definition fixes the bits -- input dropout against a plain trainer fed ``X o keep * scale`` from the numpy
Philox, the defaults against an untouched trainer, eval paths, reproducibility, resume, group against solo under two chunk sizes,
rejections -- and per element against the float64 step of ``tests/regularizer_checker.py`` (|got - ref| <= 2 x its derived bound; the
loss stage alone within 1 x the combined bound of ``tests/loss_checker.py``) where a GEMM's summation order is the device's own.
Shapes are the smallest that cross a 64-wide tile with a ragged edge: widths 70, 65, 130, 132, K = 5 and 108, mini-batches of 67,
three steps with a ragged last one.  A step is observed through ``beta1 = 0`` one-step passes, as in ``tests/test_gpu_trainer_step.py``.

Measured max |got - ref| / bound per case and tensor: ``profiles/regularizers.txt`` (written per test into the directory
``MMC_REGULARIZER_PARITY_OUT`` names)."""

import ctypes as C
import os

import numpy as np
import pytest

import loss_checker as lc
import regularizer_checker as rc
from oracle import mlp_step_ref as sr
from test_gpu_trainer_step import _Trainer, _named

pytestmark = pytest.mark.gpu

FACTOR = 2.0
SEED = rc.MASK_SEED
MB = rc.MB
N3 = 2 * MB + 30            # three steps, the last one ragged


class _T(_Trainer):
    """``_Trainer`` plus the regularisers' entry points."""

    def set_dropout(self, p_input, p_hidden, seed=SEED):
        return self.lib.mmc_trainer_set_dropout(self.h, p_input, p_hidden, seed)

    def set_loss(self, eps=0.0, gamma=0.0, prior=None):
        p = None if prior is None else np.ascontiguousarray(prior, np.float32).ctypes.data_as(C.POINTER(C.c_float))
        self._lib.check(self.lib.mmc_trainer_set_loss(self.h, eps, gamma, p))

    def set_step(self, step):
        """Zero moments at step count ``step``: a ``beta1 = 0`` pass from here still returns its gradient as ``exp_avg``."""
        zw, zb = [np.zeros(s, np.float32) for s in self.shapes], [np.zeros(s[0], np.float32) for s in self.shapes]
        for which in (0, 1):
            self.set_moments(which, zw, zb, step)

    def fit_set_mixed(self, fs, visit, partner, lam, batch_size):
        """-> (status, avg_loss); any of visit / partner / lam may be None."""
        from mermaid_classifier_amd.backbone import _current_stream_ptr
        keep = [None if a is None else np.ascontiguousarray(a, dt) for a, dt in ((visit, np.int64), (partner, np.int64), (lam, np.float32))]
        n = len(fs) if keep[0] is None else len(keep[0])
        avg = C.c_double(np.nan)
        status = self.lib.mmc_trainer_partial_fit_set_mixed(self.h, fs._handle(), *[None if a is None else a.ctypes.data for a in keep], n,
                                                            batch_size, C.byref(avg), _current_stream_ptr(0))
        return status, avg.value

    def loss_gradient_mixed(self, z, y, y2, lam):
        z, y, y2 = np.ascontiguousarray(z, np.float32), np.ascontiguousarray(y, np.int32), np.ascontiguousarray(y2, np.int32)
        d, l = np.full(z.shape, np.nan, np.float32), np.full(len(y), np.nan, np.float32)
        status = self.lib.mmc_trainer_loss_gradient_mixed(self.h, z.ctypes.data, y.ctypes.data, y2.ctypes.data, lam, len(y), d.ctypes.data,
                                                          l.ctypes.data, None)
        return status, d, l

    def evaluate_set(self, fs):
        from mermaid_classifier_amd.backbone import _current_stream_ptr
        correct, q32 = C.c_int64(-1), C.c_int64(-1)
        self._lib.check(self.lib.mmc_trainer_evaluate_set_q32(self.h, fs._handle(), 0, len(fs), C.byref(correct), C.byref(q32),
                                                              _current_stream_ptr(0)))
        return correct.value, q32.value

    def state(self):
        """(parameters, exp_avg, exp_avg_sq) as flat lists, and the step count."""
        pw, pb = self.params()
        mw, mb_, step = self.moments(0)
        vw, vb, step_v = self.moments(1)
        assert step == step_v
        return pw + pb, mw + mb_, vw + vb, step


def _same(a, b):
    return a[3] == b[3] and all(len(u) == len(v) and all(np.array_equal(p, q) for p, q in zip(u, v)) for u, v in zip(a[:3], b[:3]))


def _group_call(ts, fs, visits, partners, lams, batch_sizes, mixed_entry=True):
    from mermaid_classifier_amd import _lib
    from mermaid_classifier_amd.backbone import _current_stream_ptr
    count = len(ts)
    keep = [[None if a is None else np.ascontiguousarray(a, dt) for a in arrs]
            for arrs, dt in ((visits, np.int64), (partners, np.int64), (lams, np.float32))]
    ptrs = [(C.c_void_p * count)(*[None if a is None else a.ctypes.data for a in arrs]) for arrs in keep]
    avg = (C.c_double * count)()
    handles = (C.c_void_p * count)(*[t.h.value for t in ts])
    n = (C.c_int64 * count)(*[len(v) for v in keep[0]])
    bsz = (C.c_int * count)(*batch_sizes)
    lib = _lib.lib()
    if mixed_entry:
        status = lib.mmc_trainer_group_partial_fit_set_mixed(handles, count, fs._handle(), ptrs[0], ptrs[1], ptrs[2], n, bsz, avg,
                                                             _current_stream_ptr(0))
    else:
        status = lib.mmc_trainer_group_partial_fit_set(handles, count, fs._handle(), ptrs[0], n, bsz, avg, _current_stream_ptr(0))
    return status, list(avg)


def _hold(label, got, ref, bound, lines, failures, n_layers):
    for k, g in got.items():
        g = np.asarray(g)
        assert g.shape == ref[k].shape == bound[k].shape and np.isfinite(g).all() and np.isfinite(bound[k]).all(), (label, k)
        ratio, idx = sr.worst_ratio(g, ref[k], bound[k])
        lines.append(f"{label:34s} {k:7s} max|got-ref|/bound {ratio:7.4f} at {idx}")
        rep = sr.exceed_report(k, n_layers, g, ref[k], bound[k], FACTOR)
        if rep:
            failures.append(f"{label}: {rep}")


def _finish(name, lines, failures):
    print("\n".join(lines))
    out_dir = os.environ.get("MMC_REGULARIZER_PARITY_OUT")       # tools: keep the table (profiles/regularizers.txt)
    if out_dir:
        with open(os.path.join(out_dir, f"regularizer_parity_{name}.txt"), "w") as f:
            f.write("\n".join(lines + failures) + "\n")
    assert not failures, f"{len(failures)} tensors exceed {FACTOR:g} x bound\n" + "\n".join(failures)


@pytest.fixture(scope="module")
def pass_data():
    """164 rows of width 70 and of width 132 with 5 classes, their visiting order, class weights and parameters per width: what the
    bit-for-bit tests share (read only)."""
    out = {}
    for dim0, hidden in ((70, (65,)), (132, (130, 65))):
        rng = np.random.default_rng([21, dim0])
        dims = (dim0,) + hidden + (5,)
        ws, bs = sr.make_params(rng, dims)
        cw = sr.make_weights(rng, 5)
        X, y = sr.make_rows(rng, 200, dim0, 5)
        visit = rng.permutation(200)[:N3].astype(np.int64)
        live = int(np.flatnonzero(cw > 0)[0])
        y[visit[[0, MB, 2 * MB]]] = live                          # every mini-batch carries weight
        for a in (X, y, visit, cw):
            a.setflags(write=False)
        out[dim0] = (dims, ws, bs, cw, X, y, visit)
    return out


def _fs(X, y, K=5):
    from mermaid_classifier_amd import FeatureSet
    return FeatureSet(X.shape[1], np.arange(K)).append(X, y)


# ---- input dropout, bit for bit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,dim0", [("set-70", 70), ("host-132", 132)])
def test_input_dropout_is_a_plain_pass_over_masked_rows(pass_data, route, dim0):
    """Three steps with p_input = 0.25: parameters, both moments and avg_loss equal those of a plain trainer fed
    ``X o keep * scale``, each step's mask built by the numpy Philox from that step's own counter."""
    dims, ws, bs, cw, X, y, visit = pass_data[dim0]
    Xv, yv = X[visit], y[visit]
    fed = np.concatenate([rc.dropped_input(Xv[s:s + MB], rc.keep_mask(SEED, t, 0, len(Xv[s:s + MB]), dim0, 0.25), 0.25)
                          for t, s in enumerate(range(0, N3, MB))])
    assert fed.shape == Xv.shape and 0.2 < (fed == 0).mean() < 0.3
    a, b = _T(ws, bs, cw), _T(ws, bs, cw)
    fs = None
    try:
        assert a.set_dropout(0.25, 0.0) == 0
        before = Xv.copy()
        if route.startswith("set"):
            fs = _fs(X, y)
            avg_a = a.fit_set(fs, visit, MB)
            assert np.array_equal(fs.read()[0], X)                                       # the set's rows are never written
        else:
            status, avg_a = a.fit(Xv, yv, MB)
            assert status == 0, a.lib.mmc_last_error()
            assert np.array_equal(Xv, before)                                            # nor the caller's
        status, avg_b = b.fit(fed, yv, MB)
        assert status == 0, b.lib.mmc_last_error()
        sa, sb = a.state(), b.state()
    finally:
        a.close()
        b.close()
        if fs is not None:
            fs.close()
    assert sa[3] == 3 and _same(sa, sb) and avg_a == avg_b


# ---- hidden dropout, per element -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.DROP_CASES, ids=[c.id for c in rc.DROP_CASES])
def test_hidden_dropout_step_within_twice_the_bound(case):
    ws, bs, cw, X, y, masks = rc.make_drop_case(case)
    ref, bound = rc.step(ws, bs, X, y, rc.ALPHA, cw, masks, eps=case.eps)
    ref.pop("logits"), bound.pop("logits")                        # a dropping forward is seen through the gradients alone
    t = _T(ws, bs, cw, beta1=0.0, alpha=rc.ALPHA)
    try:
        assert t.set_dropout(0.0, case.p) == 0
        if case.eps:
            t.set_loss(eps=case.eps)
        t.set_step(case.step0)
        status, avg = t.fit(X, y, MB)
        assert status == 0, t.lib.mmc_last_error()
        gw, gb, step = t.moments(0)
    finally:
        t.close()
    assert step == case.step0 + 1
    got = {"loss": np.asarray(avg), **_named(gw, gb)}
    assert set(got) == set(ref)
    lines, failures = [f"# {case.id}: dims {case.dims}, mb {MB}, p_hidden {case.p}, step {case.step0}"], []
    _hold(case.id, got, ref, bound, lines, failures, len(ws))
    _finish("drop_" + case.id, lines, failures)


# ---- mixed loss stage, per element ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 108])
def test_mixed_loss_gradient_within_the_combined_bound(K):
    rng = np.random.default_rng([31, K])
    z, ya = lc.logit_rows(rng, MB, K, 4.0)
    yb = rng.integers(0, K, size=MB)
    w, prior = lc.class_weights(rng, K), lc.dirichlet_prior(rng, K)
    ya[0] = yb[0] = int(np.flatnonzero(w > 0)[0])
    dims = (70, K)
    ws, bs = sr.make_params(rng, dims)
    lines, worst = [f"# mmc_trainer_loss_gradient_mixed, n {MB}, K {K}: max |got - ref| / bound"], 0.0
    for kind, cw, opts in (("plain", None, {}), ("general", w, dict(eps=0.1, gamma=2.0, prior=prior))):
        t = _T(ws, bs, cw)
        try:
            if opts:
                t.set_loss(**opts)
            for lam in (0.0, 0.3, 1.0):
                status, d, l = t.loss_gradient_mixed(z, ya, yb, lam)
                assert status == 0, t.lib.mmc_last_error()
                grad, rows, bd, bl = rc.mixed_loss(z, ya, yb, lam, cw, **opts)
                ed, el = float((np.abs(d - grad) / bd).max()), float((np.abs(l - rows) / bl).max())
                lines.append(f"mixed-loss K{K:<4d} {kind:8s} lam {lam:3.1f}   dlogits {ed:7.4f}  row_loss {el:7.4f}")
                worst = max(worst, ed, el)
            assert t.moments(0)[2] == 0
        finally:
            t.close()
    print("\n".join(lines))
    out_dir = os.environ.get("MMC_REGULARIZER_PARITY_OUT")
    if out_dir:
        with open(os.path.join(out_dir, f"regularizer_parity_mixed_loss_K{K}.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    assert worst <= 1.0, "\n".join(lines)


def test_mixed_step_over_a_feature_set_within_twice_the_bound():
    """One step with visit, partner and lam over a resident set, hidden dropout 0.25 at step 1, against the checker fed the
    numpy-fp32 mixed rows."""
    ws, bs, cw, X, y, visit, partner, lam, masks = rc.mixed_step_case()
    Xm = rc.mix_rows(X, visit, partner, lam[0])
    ref, bound = rc.step(ws, bs, Xm, y[visit], rc.ALPHA, cw, masks, y2=y[partner], lam=lam[0])
    ref.pop("logits"), bound.pop("logits")
    t = _T(ws, bs, cw, beta1=0.0, alpha=rc.ALPHA)
    fs = _fs(X, y)
    try:
        assert t.set_dropout(0.0, 0.25) == 0
        t.set_step(1)
        status, avg = t.fit_set_mixed(fs, visit, partner, lam, MB)
        assert status == 0, t.lib.mmc_last_error()
        gw, gb, step = t.moments(0)
    finally:
        t.close()
        fs.close()
    assert step == 2
    got = {"loss": np.asarray(avg), **_named(gw, gb)}
    lines, failures = ["# mixed step: dims (70, 130, 65, 5), 67 of 100 rows, lam 0.3, p_hidden 0.25, step 1"], []
    _hold("mixed-step", got, ref, bound, lines, failures, len(ws))
    _finish("mixed_step", lines, failures)


@pytest.mark.parametrize("dim0", [70, 132], ids=["dword-lanes-70", "16-byte-lanes-132"])
def test_lam_one_and_zero_select_rows_and_labels(pass_data, dim0, monkeypatch):
    """lam = 1 keeps row a and its label, lam = 0 takes the partner's: ``1 a + 0 b`` is ``a`` in fp32 and ``1 l(ya) + 0 l(yb)`` is
    ``l(ya)``, so a mixed pass with lam (1, 0, 1) has the bits of the mixed pass with lam 1 over the rows it selects -- through both
    gather lanes, with one mini-batch per chunk, so a partner or lam read at the wrong offset of the pass shows."""
    dims, ws, bs, cw, X, y, visit = pass_data[dim0]
    partner = visit[np.random.default_rng(3).permutation(N3)]
    lam = np.asarray([1.0, 0.0, 1.0], np.float32)
    rows = np.concatenate([visit[:MB], partner[MB:2 * MB], visit[2 * MB:]])
    Xm = np.concatenate([rc.mix_rows(X, visit[s:s + MB], partner[s:s + MB], lam[i]) for i, s in enumerate(range(0, N3, MB))])
    assert np.array_equal(Xm, X[rows]) and not np.array_equal(rows, visit)
    a, b = _T(ws, bs, cw), _T(ws, bs, cw)
    fs = _fs(X, y)
    try:
        monkeypatch.setenv("MMC_TRAIN_CHUNK_ROWS", str(MB))
        status_a, avg_a = a.fit_set_mixed(fs, visit, partner, lam, MB)
        monkeypatch.delenv("MMC_TRAIN_CHUNK_ROWS")
        status_b, avg_b = b.fit_set_mixed(fs, rows, visit, np.ones(3, np.float32), MB)
        assert status_a == status_b == 0, a.lib.mmc_last_error()
        sa, sb = a.state(), b.state()
    finally:
        a.close()
        b.close()
        fs.close()
    assert sa[3] == 3 and _same(sa, sb) and avg_a == avg_b


# ---- defaults ----------------------------------------------------------------------------------------------------------------------
def test_defaults_give_the_bits_of_an_untouched_trainer(pass_data):
    dims, ws, bs, cw, X, y, visit = pass_data[70]
    fs = _fs(X, y)
    ts = [_T(ws, bs, cw) for _ in range(4)]
    try:
        avg0 = ts[0].fit_set(fs, visit, MB)                                     # never touched
        assert ts[1].set_dropout(0.3, 0.3) == 0 and ts[1].set_dropout(0.0, 0.0, 12345) == 0
        avg1 = ts[1].fit_set(fs, visit, MB)
        status, avg2 = ts[2].fit_set_mixed(fs, visit, None, None, MB)           # the mixed entry point without a plan
        assert status == 0, ts[2].lib.mmc_last_error()
        assert ts[3].set_dropout(1e-12, 1e-12) == 0                              # thresh 0: off
        status, avgs = _group_call([ts[3]], fs, [visit], [None], [None], [MB])
        assert status == 0, ts[3].lib.mmc_last_error()
        states = [t.state() for t in ts]
    finally:
        for t in ts:
            t.close()
        fs.close()
    assert states[0][3] == 3
    for s, avg in zip(states[1:], (avg1, avg2, avgs[0])):
        assert _same(states[0], s) and avg == avg0


# ---- eval paths ------------------------------------------------------------------------------------------------------------------------
def test_eval_paths_of_a_dropping_trainer_are_the_plain_forward(pass_data):
    dims, ws, bs, cw, X, y, visit = pass_data[132]
    fs = _fs(X, y)
    a = _T(ws, bs, cw)
    b = None
    try:
        assert a.set_dropout(0.25, 0.5) == 0
        a.fit_set(fs, visit, MB)
        pw, pb = a.params()
        assert not np.array_equal(pw[0], ws[0])
        b = _T(pw, pb, cw)                                                       # a plain trainer holding the same parameters
        za, zb = a.logits(X), b.logits(X)
        ea, eb = a.evaluate_set(fs), b.evaluate_set(fs)
        status, da, la = a.loss_gradient_mixed(za, y, y, 1.0)
        status_b, db, lb = b.loss_gradient_mixed(zb, y, y, 1.0)
    finally:
        a.close()
        if b is not None:
            b.close()
        fs.close()
    assert np.isfinite(za).all() and np.array_equal(za, zb) and ea == eb and ea[0] >= 0
    assert status == status_b == 0 and np.array_equal(da, db) and np.array_equal(la, lb)


# ---- reproducibility and resume -------------------------------------------------------------------------------------------------------------
def _regularized_pass(pass_data, seed, dim0=70):
    dims, ws, bs, cw, X, y, visit = pass_data[dim0]
    partner = np.concatenate([visit[s:s + MB][np.random.default_rng([4, s]).permutation(len(visit[s:s + MB]))] for s in range(0, N3, MB)])
    lam = np.asarray([0.3, 0.85, 0.5], np.float32)
    fs = _fs(X, y)
    t = _T(ws, bs, cw)
    try:
        assert t.set_dropout(0.1, 0.5, seed) == 0
        status, avg = t.fit_set_mixed(fs, visit, partner, lam, MB)
        assert status == 0, t.lib.mmc_last_error()
        return t.state(), avg
    finally:
        t.close()
        fs.close()


def test_same_seed_same_bits_another_seed_other_bits(pass_data):
    (s1, a1), (s2, a2), (s3, a3) = (_regularized_pass(pass_data, seed) for seed in (SEED, SEED, SEED ^ (1 << 40)))
    assert np.isfinite(a1) and _same(s1, s2) and a1 == a2
    assert not _same(s1, s3) and a1 != a3 and s1[3] == s3[3] == 3               # a bit of the key's high word


def test_resumed_trainer_continues_the_mask_sequence(pass_data):
    dims, ws, bs, cw, X, y, visit = pass_data[132]
    a = _T(ws, bs, cw)
    b = None
    try:
        assert a.set_dropout(0.25, 0.5) == 0
        assert a.fit(X[visit[:MB]], y[visit[:MB]], MB)[0] == 0
        pw, pb = a.params()
        mw, mb_, step = a.moments(0)
        vw, vb, _ = a.moments(1)
        assert step == 1
        b = _T(pw, pb, cw)                                                       # a fresh trainer given pass 1's state and the seed
        assert b.set_dropout(0.25, 0.5) == 0
        b.set_moments(0, mw, mb_, 1)
        b.set_moments(1, vw, vb, 1)
        rows = visit[MB:2 * MB]
        sa, avg_a = a.fit(X[rows], y[rows], MB)
        sb, avg_b = b.fit(X[rows], y[rows], MB)
        assert sa == sb == 0
        fin_a, fin_b = a.state(), b.state()
        # ... and a trainer whose step count did not come along draws step 0's masks again: other bits
        c = _T(pw, pb, cw)
        try:
            assert c.set_dropout(0.25, 0.5) == 0
            c.set_moments(0, mw, mb_, 0)
            c.set_moments(1, vw, vb, 0)
            assert c.fit(X[rows], y[rows], MB)[0] == 0
            gc = c.moments(0)
        finally:
            c.close()
    finally:
        a.close()
        if b is not None:
            b.close()
    assert fin_a[3] == 2 and _same(fin_a, fin_b) and avg_a == avg_b
    assert not all(np.array_equal(u, v) for u, v in zip(fin_a[1], gc[0] + gc[1]))


# ---- group equals solo ------------------------------------------------------------------------------------------------------------------
def _group_members(pass_data):
    """Three unlike members over one set of width 70: plain (no hidden layer, unweighted), dropout (one hidden layer, class weights,
    its own rows and mini-batch), dropout + mixup (two hidden layers, label smoothing)."""
    dims, ws, bs, cw, X, y, visit = pass_data[70]
    rng = np.random.default_rng(77)
    members = []
    for hidden, rows, mb in (((), 150, 50), ((65,), N3, MB), ((130, 65), N3, MB)):
        w, b = sr.make_params(rng, (70,) + hidden + (5,))
        members.append(dict(ws=w, bs=b, visit=rng.permutation(200)[:rows].astype(np.int64), mb=mb))
    members[1].update(cw=cw, drop=(0.1, 0.5))
    v = members[1]["visit"]
    members[1]["visit"] = np.concatenate([visit[:1], v[1:MB], visit[:1], v[MB + 1:2 * MB], visit[:1], v[2 * MB + 1:]])   # weight in every batch
    v = members[2]["visit"]
    members[2].update(drop=(0.25, 0.25), eps=0.1, lam=np.asarray([0.3, 0.0, 0.9], np.float32),
                      partner=np.concatenate([v[s:s + MB][rng.permutation(len(v[s:s + MB]))] for s in range(0, N3, MB)]))
    return X, y, members


def _make(m):
    t = _T(m["ws"], m["bs"], m.get("cw"))
    if "drop" in m:
        assert t.set_dropout(*m["drop"]) == 0
    if "eps" in m:
        t.set_loss(eps=m["eps"])
    return t


@pytest.mark.parametrize("chunk", ["67", "100000"])
def test_group_members_equal_their_solo_runs(pass_data, chunk, monkeypatch):
    X, y, members = _group_members(pass_data)
    fs = _fs(X, y)
    solo, group = [_make(m) for m in members], [_make(m) for m in members]
    try:
        monkeypatch.delenv("MMC_TRAIN_CHUNK_ROWS", raising=False)
        solo_avg = []
        for t, m in zip(solo, members):
            status, avg = t.fit_set_mixed(fs, m["visit"], m.get("partner"), m.get("lam"), m["mb"])
            assert status == 0, t.lib.mmc_last_error()
            solo_avg.append(avg)
        monkeypatch.setenv("MMC_TRAIN_CHUNK_ROWS", chunk)                       # read at every call
        status, avgs = _group_call(group, fs, [m["visit"] for m in members], [m.get("partner") for m in members],
                                   [m.get("lam") for m in members], [m["mb"] for m in members])
        assert status == 0, group[0].lib.mmc_last_error()
        ss, gs = [t.state() for t in solo], [t.state() for t in group]
    finally:
        for t in solo + group:
            t.close()
        fs.close()
    for i, (s, g) in enumerate(zip(ss, gs)):
        assert s[3] == 3 and _same(s, g) and solo_avg[i] == avgs[i], f"member {i}"
    assert np.isfinite(solo_avg).all()


# ---- rejections -----------------------------------------------------------------------------------------------------------------------------
def test_rejections_launch_nothing_and_change_nothing(pass_data):
    from mermaid_classifier_amd import _lib
    dims, ws, bs, cw, X, y, visit = pass_data[70]
    fs = _fs(X, y)
    t, other = _T(ws, bs, cw), _T(ws, bs, None)
    partner = visit[::-1].copy()
    lam = np.asarray([0.3, 0.5, 0.7], np.float32)
    try:
        assert t.set_dropout(0.1, 0.5) == 0
        assert t.fit_set_mixed(fs, visit, partner, lam, MB)[0] == 0             # a state with non-zero moments and step 3
        before = t.state()
        other_before = other.state()

        def rejected(status, text):
            assert status == _lib.MMC_ERR_ARG and text in t.lib.mmc_last_error().decode(), (status, t.lib.mmc_last_error())
            assert _same(t.state(), before) and _same(other.state(), other_before)

        for p_in, p_hid, text in ((-0.1, 0.0, "p_input"), (0.95, 0.0, "p_input"), (float("nan"), 0.0, "p_input"), (0.0, 0.91, "p_hidden"),
                                  (0.0, float("inf"), "p_hidden")):
            rejected(t.set_dropout(p_in, p_hid), text)
        bad = partner.copy()
        bad[100] = 200
        rejected(t.fit_set_mixed(fs, visit, bad, lam, MB)[0], "partner[100] = 200")
        bad[100] = -1
        rejected(t.fit_set_mixed(fs, visit, bad, lam, MB)[0], "partner[100] = -1")
        for i, v in ((0, float("nan")), (1, 1.5), (2, -0.25), (1, float("inf"))):
            wrong = lam.copy()
            wrong[i] = v
            rejected(t.fit_set_mixed(fs, visit, partner, wrong, MB)[0], f"lam[{i}]")
        rejected(t.fit_set_mixed(fs, visit, partner, None, MB)[0], "only partner")
        rejected(t.fit_set_mixed(fs, visit, None, lam, MB)[0], "only lam")
        # a mini-batch whose mixed weight sum is not positive: every row and every partner of mini-batch 1 in the class without weight
        dead = int(np.flatnonzero(cw == 0)[0])
        rows_dead = np.flatnonzero(y == dead)
        assert len(rows_dead) > 0
        v2, p2 = visit.copy(), partner.copy()
        v2[MB:2 * MB] = rows_dead[0]
        p2[MB:2 * MB] = rows_dead[-1]
        rejected(t.fit_set_mixed(fs, v2, p2, lam, MB)[0], "mini-batch 1 has zero total mixed class weight")
        # in a group: the faulty member is named and the sound member does not move either
        status, _ = _group_call([other, t], fs, [visit, visit], [None, bad], [None, lam], [MB, MB])
        rejected(status, "member 1: partner[100]")
        status, _ = _group_call([other, t], fs, [visit, visit], [partner, partner], [None, lam], [MB, MB])
        rejected(status, "member 0: partner and lam go together")
        # the same pass, sound, still runs afterwards and gives the bits of a trainer that saw no rejection
        twin = _T(ws, bs, cw)
        try:
            assert twin.set_dropout(0.1, 0.5) == 0
            for tt in (t, twin):
                for _ in range(1 if tt is t else 2):
                    assert tt.fit_set_mixed(fs, visit, partner, lam, MB)[0] == 0
            assert _same(t.state(), twin.state()) and t.state()[3] == 6
        finally:
            twin.close()
    finally:
        t.close()
        other.close()
        fs.close()


# ---- smoke: a sweep --------------------------------------------------------------------------------------------------------------------------
def test_sweep_with_plain_dropout_and_mixup_members():
    """Two epochs of ``train_sweep`` over features the synthetic backbone (``synthetic.py``) extracts from synthetic patches, with
    configurations [plain, dropout 0.2, mixup 0.2]: finite losses, and member 0 bit-equal to the plain solo run."""
    from mermaid_classifier_amd import FeatureSet, SweepConfig, train_classifier, train_sweep
    from mermaid_classifier_amd.backbone import Backbone
    from mermaid_classifier_amd.synthetic import synthetic_state_dict
    from oracle import efficientnet_b0_ref as ref
    from conftest import GOLDEN
    sd = synthetic_state_dict(seed=0, bn_stats=dict(np.load(GOLDEN / "synth_bn_stats.npz")))
    bb = Backbone(sd, device=0, max_batch=16)
    try:
        feats = bb.extract(np.concatenate([ref.natural_patches(24, seed=5), ref.synthetic_patches(24, seed=6)]))
    finally:
        bb.close()
    assert feats.shape == (48, 1280) and np.isfinite(feats).all()
    # 240 rows: the 48 feature vectors with seeded noise, four classes by patch index
    rng = np.random.default_rng(8)
    X = (np.tile(feats, (5, 1)) * (1.0 + 0.05 * rng.standard_normal((240, 1280)))).astype(np.float32)
    y = np.tile(np.arange(48) % 4, 5)
    classes = [0, 1, 2, 3]
    sets = [FeatureSet(1280, classes).append(X[s], y[s]) for s in (slice(0, 160), slice(160, 200), slice(200, 240))]
    base = dict(hidden_layer_sizes=(70, 65), learning_rate_init=1e-3, random_state=0, batch_size=67)
    configs = [SweepConfig(**base), SweepConfig(**base, dropout=0.2, input_dropout=0.1), SweepConfig(**base, mixup_alpha=0.2)]
    try:
        seen = []
        got = train_sweep(*sets, configs, 2, batch_size=160, on_epoch_end=seen.append)
        solo = train_classifier(*sets, 2, batch_size=160, clf=configs[0].classifier(sets[1].device))
    finally:
        for s in sets:
            s.close()
    assert len(got) == 3 and len(seen) == 6
    assert all(np.isfinite(m["training_loss"]) and np.isfinite(m["val_loss"]) for m in seen)
    for u, v in zip(got[0][0].weights + got[0][0].biases, solo[0].weights + solo[0].biases):
        assert np.array_equal(u, v)
    assert np.array_equal(got[0][0].a_, solo[0].a_) and got[0][2] == solo[2]
    for i in (1, 2):                                                              # the regularised members trained something else
        assert not np.array_equal(got[i][0].weights[0], got[0][0].weights[0])
        assert all(np.isfinite(w).all() for w in got[i][0].weights)
