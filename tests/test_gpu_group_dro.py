"""Group-robust training on the device (include/mmc.h, "group-robust training"): per-row weights and group DRO in resident passes.

``mmc_trainer_loss_gradient_weighted`` per element against the float64 checker within the bounds of tests/group_dro_checker.py
(derived there; tests/test_group_dro_host.py shows an fp32 emulation stays within a twentieth of them and wrong stages miss them by
orders of magnitude).  Everything else is bit equality: all-ones weights against the unweighted pass, a member of a group against
its solo pass, one chunk bound against another, the stage against the pass, a resumed trainer against the original, a rejected call
against none, ``train_sweep`` against ``train_classifier``.

Shapes: K = 5 (one class weight zero) and K = 70 (a second 64-lane stride), widths 12 and 16, one hidden layer of 9, 17 rows in
mini-batches of 7 (three steps, the last of 3 rows; loss blocks of 4 rows with a ragged tail), G = 3 / 1 / 1024."""

import ctypes as C
import pickle

import numpy as np
import pytest

import group_dro_checker as gc

pytestmark = pytest.mark.gpu

HIDDEN = 9
SHAPES = [(5, 12), (70, 16)]                       # (classes, feature width)


class _Raw:
    """An ``mmc_trainer`` through the C ABI alone."""

    def __init__(self, weights, biases, class_weight=None, lr=1e-2, alpha=1e-3):
        from mermaid_classifier_amd import _lib
        from mermaid_classifier_amd.torch_classifier import _ptr_array
        self.lib, self._lib, self._ptr_array = _lib.lib(), _lib, _ptr_array
        self.shapes = [w.shape for w in weights]
        dims = [weights[0].shape[1]] + [w.shape[0] for w in weights]
        self.K, self.G = dims[-1], 0
        self.h = C.c_void_p()
        cw = None if class_weight is None else np.ascontiguousarray(class_weight, np.float32)
        _lib.check(self.lib.mmc_trainer_create(_ptr_array(weights), _ptr_array(biases), (C.c_int * len(dims))(*dims), len(weights),
                                               lr, 0.9, 0.999, 1e-8, alpha,
                                               None if cw is None else cw.ctypes.data_as(C.POINTER(C.c_float)), 0, C.byref(self.h)))

    def set_dro(self, G, eta):
        status = self.lib.mmc_trainer_set_group_dro(self.h, int(G), float(eta))
        if status == 0:
            self.G = int(G)
        return status

    def logq(self, new=None):
        if new is not None:
            new = np.ascontiguousarray(new, np.float64)
            return self.lib.mmc_trainer_group_dro_state(self.h, 1, new.ctypes.data)
        out = np.full(self.G, np.nan)
        self._lib.check(self.lib.mmc_trainer_group_dro_state(self.h, 0, out.ctypes.data))
        return out

    def set_loss(self, eps=0.0, gamma=0.0, prior=None):
        p = None if prior is None else np.ascontiguousarray(prior, np.float32)
        self._lib.check(self.lib.mmc_trainer_set_loss(self.h, float(eps), float(gamma),
                                                      None if p is None else p.ctypes.data_as(C.POINTER(C.c_float))))

    def fit(self, fs, rw=None, rg=None, mb=gc.MB, weighted=True):
        """One pass over every row of ``fs`` in stored order -> (status, avg_loss)."""
        avg = C.c_double(-1.0)
        rw = None if rw is None else np.ascontiguousarray(rw, np.float32)
        rg = None if rg is None else np.ascontiguousarray(rg, np.int32)
        if weighted:
            status = self.lib.mmc_trainer_partial_fit_set_weighted(self.h, fs._handle(), None, None if rw is None else rw.ctypes.data,
                                                                   None if rg is None else rg.ctypes.data, len(fs), mb, C.byref(avg), None)
        else:
            status = self.lib.mmc_trainer_partial_fit_set(self.h, fs._handle(), None, len(fs), mb, C.byref(avg), None)
        return status, avg.value

    def stage(self, z, y, rw=None, rg=None, logq=None, eta=0.0, G=0, group_loss=True):
        z, y32 = np.ascontiguousarray(z, np.float32), np.ascontiguousarray(y, np.int32)
        rw = None if rw is None else np.ascontiguousarray(rw, np.float32)
        rg = None if rg is None else np.ascontiguousarray(rg, np.int32)
        lq = None if logq is None else np.ascontiguousarray(logq, np.float64)
        d, l = np.full(z.shape, np.nan, np.float32), np.full(len(y32), np.nan, np.float32)
        qo, gl = np.full(max(G, 1), np.nan), np.full(max(G, 1), -7.0)
        status = self.lib.mmc_trainer_loss_gradient_weighted(
            self.h, z.ctypes.data, y32.ctypes.data, None if rw is None else rw.ctypes.data, None if rg is None else rg.ctypes.data,
            None if lq is None else lq.ctypes.data, float(eta), int(G), len(y32), d.ctypes.data, l.ctypes.data, qo.ctypes.data,
            gl.ctypes.data if group_loss else None, None)
        return status, d, l, qo[:G], gl[:G]

    def logits(self, X):
        X = np.ascontiguousarray(X, np.float32)
        out = np.empty((len(X), self.K), np.float32)
        self._lib.check(self.lib.mmc_trainer_logits(self.h, X.ctypes.data, len(X), out.ctypes.data, None))
        return out

    def _buffers(self):
        return [np.empty(s, np.float32) for s in self.shapes], [np.empty(s[0], np.float32) for s in self.shapes]

    def params(self):
        ws, bs = self._buffers()
        self._lib.check(self.lib.mmc_trainer_get_params(self.h, self._ptr_array(ws), self._ptr_array(bs)))
        return ws, bs

    def adam(self, which, new=None, step=0):
        s = C.c_longlong(step)
        ws, bs = self._buffers() if new is None else new
        self._lib.check(self.lib.mmc_trainer_adam_state(self.h, which, 0 if new is None else 1, self._ptr_array(ws), self._ptr_array(bs),
                                                        C.byref(s)))
        return (ws, bs), int(s.value)

    def state(self):
        """Parameters, both moments, the step count and log q (when kept)."""
        arrays = [a for part in self.params() for a in part]
        step = 0
        for which in (0, 1):
            (ws, bs), step = self.adam(which)
            arrays += ws + bs
        if self.G:
            arrays.append(self.logq())
        return arrays, step

    def close(self):
        self.lib.mmc_trainer_destroy(self.h)


def _same(a, b):
    (pa, sa), (pb, sb) = a, b
    return sa == sb and len(pa) == len(pb) and all(u.tobytes() == v.tobytes() for u, v in zip(pa, pb))


def _init(K, NF, seed=0):
    rng = np.random.default_rng([K, NF, seed])
    return ([(rng.standard_normal((HIDDEN, NF)) * 0.4).astype(np.float32), (rng.standard_normal((K, HIDDEN)) * 0.4).astype(np.float32)],
            [(rng.standard_normal(HIDDEN) * 0.1).astype(np.float32), (rng.standard_normal(K) * 0.1).astype(np.float32)])


@pytest.fixture(scope="module")
def sets():
    """Per shape: the shared inputs' labels and weights, 17 feature rows, and the resident set of them."""
    from mermaid_classifier_amd import FeatureSet
    out = {}
    for K, NF in SHAPES:
        inp = gc.inputs(K)
        X = np.random.default_rng([K, NF]).standard_normal((gc.N_ROWS, NF)).astype(np.float32)
        out[K] = dict(inp, X=X, NF=NF, fs=FeatureSet(NF, np.arange(K)).append(X, inp["y"]))
    yield out
    for v in out.values():
        v["fs"].close()


def _trainer(s, K, G=0, eta=0.0, **kw):
    t = _Raw(*_init(K, s["NF"]), class_weight=s["w"], **kw)
    if G:
        assert t.set_dro(G, eta) == 0
    return t


# ---- 1. the stage per element ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 70])
def test_weighted_loss_gradient_per_element_against_the_float64_checker(K):
    inp = gc.inputs(K)
    w = inp["w"]
    trainers = {}
    try:
        for kind, opts in gc.LOSS_KINDS:
            trainers[kind] = _Raw([np.zeros((K, 4), np.float32)], [np.zeros(K, np.float32)], class_weight=w)
            loss = gc.loss_options(opts, inp["prior"])
            trainers[kind].set_loss(loss["eps"], loss["gamma"], loss["prior"])
        peak = [0.0, 0.0, 0.0]
        for name, K_, G, sl, eta, kind, opts, logq in gc.stage_cases():
            if K_ != K:
                continue
            z, y, r, a = inp["z"][sl], inp["y"][sl], inp["r"][sl], gc.row_groups(G)[sl]
            loss = gc.loss_options(opts, inp["prior"])
            status, d, l, qo, gl = trainers[kind].stage(z, y, r, a, logq, eta, G)
            assert status == 0, (name, trainers[kind].lib.mmc_last_error())
            assert np.isfinite(d).all() and np.isfinite(l).all() and np.isfinite(qo).all()
            ref = gc.checker(z, y, w, r, a, logq, eta, G, **loss)
            bnd = gc.bounds(ref, y, w, r, a, eta, G)
            rd, rl, rq = gc.ratios(d, l, qo, ref, bnd)
            print(f"{name}: dlogits {rd:.3f} row_loss {rl:.3f} logq {rq:.3f} of the bound")
            assert rd <= 1.0 and rl <= 1.0 and rq <= 1.0, (name, rd, rl, rq)
            peak = [max(p, v) for p, v in zip(peak, (rd, rl, rq))]
            # a group without mass has no loss; the others' losses are the checker's
            none = ~(ref["V"] > 0)
            assert np.array_equal(np.isnan(gl), none), name
            np.testing.assert_allclose(gl[~none], ref["group_loss"][~none], rtol=1e-5)
            assert np.all(d[r == 0] == 0) and np.all(l[r == 0] == 0), name                 # a zero weight is an exact zero
        for kind, opts in gc.LOSS_KINDS:                     # row weights only; and neither array: the unweighted stage's bits
            loss = gc.loss_options(opts, inp["prior"])
            for r in (inp["r"], None):
                status, d, l, _, _ = trainers[kind].stage(inp["z"], inp["y"], r)
                assert status == 0
                ref = gc.checker(inp["z"], inp["y"], w, r, **loss)
                bnd = gc.bounds(ref, inp["y"], w, r)
                rd, rl, _ = gc.ratios(d, l, None, ref, bnd)
                print(f"K{K} {kind} weights {'yes' if r is not None else 'no'}: dlogits {rd:.3f} row_loss {rl:.3f} of the bound")
                assert rd <= 1.0 and rl <= 1.0, (kind, rd, rl)
            z32, y32 = np.ascontiguousarray(inp["z"]), np.ascontiguousarray(inp["y"], np.int32)
            d0, l0 = np.empty_like(z32), np.empty(len(y32), np.float32)
            t = trainers[kind]
            assert t.lib.mmc_trainer_loss_gradient(t.h, z32.ctypes.data, y32.ctypes.data, len(y32), d0.ctypes.data, l0.ctypes.data, None) == 0
            assert d.tobytes() == d0.tobytes() and l.tobytes() == l0.tobytes()
            ones = np.ones(len(y32), np.float32)
            _, d1, l1, _, _ = t.stage(inp["z"], inp["y"], ones)
            assert d1.tobytes() == d0.tobytes() and l1.tobytes() == l0.tobytes()
        print(f"K{K} peak over bound: dlogits {peak[0]:.3f} row_loss {peak[1]:.3f} logq {peak[2]:.3f}")
    finally:
        for t in trainers.values():
            t.close()


# ---- 2. all-ones weights are the unweighted pass ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 70])
def test_all_ones_weights_have_the_bits_of_the_unweighted_pass(sets, K):
    s = sets[K]
    plain, ones, null = _trainer(s, K), _trainer(s, K), _trainer(s, K)
    try:
        for _ in range(2):
            a = plain.fit(s["fs"], weighted=False)
            b = ones.fit(s["fs"], rw=np.ones(gc.N_ROWS, np.float32))
            c = null.fit(s["fs"])                                             # both arrays NULL
            assert a[0] == b[0] == c[0] == 0 and a[1] == b[1] == c[1] and np.isfinite(a[1])
        assert _same(plain.state(), ones.state()) and _same(plain.state(), null.state())
        assert plain.state()[1] == 6
        other = _trainer(s, K)
        assert other.fit(s["fs"], rw=s["r"])[0] == 0 and not _same(other.state(), _one_pass_state(s, K))
        other.close()
    finally:
        for t in (plain, ones, null):
            t.close()


def _one_pass_state(s, K):
    t = _trainer(s, K)
    try:
        assert t.fit(s["fs"], weighted=False)[0] == 0
        return t.state()
    finally:
        t.close()


# ---- 3. a member of a group is its solo pass -------------------------------------------------------------------------------------------
def _members(s, K, G):
    """DRO with weights, row weights only, plain, plain with dropout, DRO with clipping: (trainer, row_weight, row_group) each."""
    a = gc.row_groups(G)
    dro = _trainer(s, K, G, 0.5)
    only_w = _trainer(s, K)
    plain = _trainer(s, K)
    drop = _trainer(s, K)
    drop._lib.check(drop.lib.mmc_trainer_set_dropout(drop.h, 0.1, 0.3, 99))
    clip = _trainer(s, K, G, 1.0)
    clip._lib.check(clip.lib.mmc_trainer_set_grad_clip(clip.h, 0.05))
    return [(dro, s["r"], a), (only_w, s["r"], None), (plain, None, None), (drop, None, None), (clip, None, a)]


@pytest.mark.parametrize("K,G", [(5, 3), (70, 1024), (5, 1)])
def test_group_members_have_the_bits_of_their_solo_passes(sets, K, G):
    s = sets[K]
    group, solo = _members(s, K, G), _members(s, K, G)
    lib = group[0][0].lib
    try:
        count = len(group)
        keep = [(None if w is None else np.ascontiguousarray(w, np.float32), None if g is None else np.ascontiguousarray(g, np.int32))
                for _, w, g in group]
        for _ in range(2):
            handles = (C.c_void_p * count)(*[t.h.value for t, _, _ in group])
            visit = (C.c_void_p * count)(*[None] * count)
            rw = (C.c_void_p * count)(*[None if w is None else w.ctypes.data for w, _ in keep])
            rg = (C.c_void_p * count)(*[None if g is None else g.ctypes.data for _, g in keep])
            n = (C.c_int64 * count)(*[gc.N_ROWS] * count)
            mb = (C.c_int * count)(*[gc.MB, gc.MB, 5, gc.MB, gc.MB])               # the plain member steps differently
            avg = (C.c_double * count)()
            assert lib.mmc_trainer_group_partial_fit_set_weighted(handles, count, s["fs"]._handle(), visit, rw, rg, n, mb, avg, None) == 0, \
                lib.mmc_last_error()
            for i, (t, w, g) in enumerate(solo):
                status, one = t.fit(s["fs"], w, g, mb=mb[i])
                assert status == 0 and one == avg[i], i
        for (t, _, _), (u, _, _) in zip(group, solo):
            assert _same(t.state(), u.state())
        states = [t.state() for t, _, _ in group]
        assert not _same(states[0], states[4]) and not _same(states[1], states[2]) and not _same(states[2], states[3])
        q = np.exp(group[0][0].logq())
        assert abs(q.sum() - 1.0) < 1e-12 and (G == 1 or q.max() > 1.0 / G)        # q has moved
    finally:
        for t, _, _ in group + solo:
            t.close()


# ---- 4. the chunk bound changes nothing ------------------------------------------------------------------------------------------------
def test_chunk_rows_do_not_change_the_bits(sets, monkeypatch):
    s, K, G = sets[70], 70, 3
    states = []
    for bound in ("7", "15", None):                     # one mini-batch per chunk; two (the bound rounds down to 14); the whole pass
        if bound is None:
            monkeypatch.delenv("MMC_TRAIN_CHUNK_ROWS", raising=False)
        else:
            monkeypatch.setenv("MMC_TRAIN_CHUNK_ROWS", bound)
        t = _trainer(s, K, G, 0.5)
        try:
            got = [t.fit(s["fs"], s["r"], gc.row_groups(G)) for _ in range(2)]
            assert all(st == 0 for st, _ in got)
            states.append((t.state(), [a for _, a in got]))
        finally:
            t.close()
    for st, avgs in states[1:]:
        assert _same(st, states[0][0]) and avgs == states[0][1]


# ---- 5. the pass runs the stage ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,eta", [(5, 0.5), (70, 0.0), (70, 2.0)])
def test_one_step_pass_is_the_stage_on_its_logits(K, eta):
    """alpha = 0 and one mini-batch of 7 rows: log q after the pass is the stage's log_q_out, bit for bit, and avg_loss is the sum of
    the stage's row losses.  loss_finalize_kernel adds them in fp32: thread i holds row_loss[i] (fmaf(0, q, s) = s at alpha = 0),
    the tree over 256 threads adds the 7 of them in ceil(log2 7) = 3 levels, the other operands being zeros, so with u = 2^-24
    |avg_loss - sum| <= ((1 + u)^3 - 1) sum |row_loss_i|; the double sum it is compared with adds nothing of that order."""
    from mermaid_classifier_amd import FeatureSet
    G, NF = 3, dict(SHAPES)[K]
    inp = gc.inputs(K)
    rows = slice(0, gc.MB)
    X = np.random.default_rng([K, 5]).standard_normal((gc.MB, NF)).astype(np.float32)
    y, r, a = inp["y"][rows], inp["r"][rows], gc.row_groups(G)[rows]
    fs = FeatureSet(NF, np.arange(K)).append(X, y)
    t = _Raw(*_init(K, NF), class_weight=inp["w"], alpha=0.0)
    try:
        assert t.set_dro(G, eta) == 0
        z = t.logits(X)
        q_before = t.logq()
        np.testing.assert_allclose(q_before, gc.uniform_logq(G), rtol=1e-15)
        status, d, l, qo, _ = t.stage(z, y, r, a, q_before, eta, G)
        assert status == 0
        assert t.logq().tobytes() == q_before.tobytes()                            # the stage left the trainer's own q alone
        status, avg = t.fit(fs, r, a)
        assert status == 0 and t.state()[1] == 1
        assert t.logq().tobytes() == qo.tobytes()
        total = float(np.sum(l.astype(np.float64)))
        bound = ((1.0 + gc.ULP) ** 3 - 1.0) * float(np.sum(np.abs(l.astype(np.float64))))
        print(f"K{K} eta {eta}: avg_loss {avg!r} sum of row losses {total!r} bound {bound:.3e}")
        assert abs(avg - total) <= bound
        assert total > 0
    finally:
        t.close()
        fs.close()


# ---- 6. resume -----------------------------------------------------------------------------------------------------------------------------
def test_resumed_trainer_continues_on_the_same_bits(sets):
    s, K, G = sets[5], 5, 3
    a = gc.row_groups(G)
    whole, first = _trainer(s, K, G, 0.5), _trainer(s, K, G, 0.5)
    resumed = None
    try:
        for _ in range(2):
            assert whole.fit(s["fs"], s["r"], a)[0] == 0
        assert first.fit(s["fs"], s["r"], a)[0] == 0
        ws, bs = first.params()
        resumed = _Raw(ws, bs, class_weight=s["w"])
        assert resumed.set_dro(G, 0.5) == 0
        for which in (0, 1):
            moments, step = first.adam(which)
            resumed.adam(which, new=moments, step=step)
        assert resumed.logq(first.logq()) == 0
        assert _same(resumed.state(), first.state())
        assert resumed.fit(s["fs"], s["r"], a)[0] == 0
        assert _same(resumed.state(), whole.state())
        # a state that is not normalised is renormalised; one that is not finite is refused
        assert resumed.logq(np.log([1.0, 2.0, 5.0])) == 0
        np.testing.assert_allclose(np.exp(resumed.logq()), [0.125, 0.25, 0.625], rtol=1e-14)
        before = resumed.logq()
        assert resumed.logq([0.0, np.nan, 0.0]) == resumed._lib.MMC_ERR_ARG and resumed.logq().tobytes() == before.tobytes()
    finally:
        for t in (whole, first, resumed):
            if t is not None:
                t.close()


# ---- 7. rejections ---------------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_change_nothing(sets):
    s, K, G = sets[5], 5, 3
    from mermaid_classifier_amd import _lib
    ERR = _lib.MMC_ERR_ARG
    a, r = gc.row_groups(G), s["r"]
    dro, plain, mate = _trainer(s, K, G, 0.5), _trainer(s, K), _trainer(s, K)
    try:
        assert dro.fit(s["fs"], r, a)[0] == 0 and plain.fit(s["fs"], r)[0] == 0       # not the initial state
        before, before_plain, before_mate = dro.state(), plain.state(), mate.state()

        def put(arr, pos, value):
            out = np.array(arr, copy=True)
            out[pos] = value
            return out
        dead = np.where(np.arange(gc.N_ROWS) // gc.MB == 1, 0.0, r).astype(np.float32)     # mini-batch 1 without mass
        bad_passes = [
            (dro, put(r, 3, -1.0), a, b"row_weight[3]"), (dro, put(r, 16, np.nan), a, b"row_weight[16]"),
            (dro, put(r, 8, np.inf), None, b"row_weight[8]"), (dro, r, put(a, 4, G), b"row_group[4]"),
            (dro, None, put(a, 0, -1), b"row_group[0]"), (dro, dead, None, b"zero total mass"),
            (dro, dead, a, b"no group of mini-batch 1 has mass"), (plain, r, a, b"mmc_trainer_set_group_dro"),
            (plain, put(r, 3, -1.0), None, b"row_weight[3]"),
        ]
        for t, w, g, word in bad_passes:
            status, avg = t.fit(s["fs"], w, g)
            assert status == ERR and word in t.lib.mmc_last_error(), (word, t.lib.mmc_last_error())
        for args in ((G, 10.5), (G, -0.1), (G, float("nan")), (1025, 0.5), (-1, 0.5)):
            assert dro.set_dro(*args) == ERR
        # in a group the rejected member keeps every member as it was
        count = 2
        handles = (C.c_void_p * count)(mate.h.value, dro.h.value)
        visit = (C.c_void_p * count)(None, None)
        neg, a32 = put(r, 3, -1.0), np.ascontiguousarray(a, np.int32)
        rw, rg = (C.c_void_p * count)(None, neg.ctypes.data), (C.c_void_p * count)(None, a32.ctypes.data)
        n, mb, avg = (C.c_int64 * count)(gc.N_ROWS, gc.N_ROWS), (C.c_int * count)(gc.MB, gc.MB), (C.c_double * count)(1.0, 1.0)
        assert dro.lib.mmc_trainer_group_partial_fit_set_weighted(handles, count, s["fs"]._handle(), visit, rw, rg, n, mb, avg, None) == ERR
        assert b"member 1" in dro.lib.mmc_last_error() and list(avg) == [0.0, 0.0]
        # the stage entry point: the same checks, and its own
        z, y = s["z"], s["y"]
        q0 = gc.uniform_logq(G)
        for kw, word in ((dict(rw=put(r, 3, -1.0), rg=a, logq=q0, eta=0.5, G=G), b"row_weight[3]"),
                         (dict(rw=r, rg=put(a, 4, G), logq=q0, eta=0.5, G=G), b"row_group[4]"),
                         (dict(rw=r, rg=a, logq=q0, eta=11.0, G=G), b"eta"), (dict(rw=r, rg=a, logq=q0, eta=0.5, G=1025), b"n_groups"),
                         (dict(rw=r, rg=a, logq=q0, eta=0.5, G=0), b"n_groups"), (dict(rw=r, rg=a, logq=None, eta=0.5, G=G), b"log_q_in"),
                         (dict(rw=np.zeros(gc.N_ROWS, np.float32)), b"zero total mass"),
                         (dict(rw=np.zeros(gc.N_ROWS, np.float32), rg=a, logq=q0, eta=0.5, G=G), b"no group")):
            status = dro.stage(z, y, **kw)[0]
            assert status == ERR and word in dro.lib.mmc_last_error(), (word, dro.lib.mmc_last_error())
        assert _same(dro.state(), before) and _same(plain.state(), before_plain) and _same(mate.state(), before_mate)
        # the plain entry point on a trainer with group DRO runs as ever and leaves q alone
        lq = dro.logq()
        assert dro.fit(s["fs"], weighted=False)[0] == 0 and dro.fit(s["fs"], r, None)[0] == 0
        assert dro.logq().tobytes() == lq.tobytes()
        fresh = _trainer(s, K, G, 0.5)
        assert dro.set_dro(G, 0.5) == 0 and dro.logq().tobytes() == fresh.logq().tobytes() != lq.tobytes()   # any call resets q
        fresh.close()
        assert dro.set_dro(0, 0.0) == 0 and dro.fit(s["fs"], None, a)[0] == ERR                            # off again
    finally:
        for t in (dro, plain, mate):
            t.close()


# ---- 8. a sweep of ERM, group-balanced and DRO members ---------------------------------------------------------------------------------
def _python_data():
    rng = np.random.default_rng(23)
    K, NF, n = 5, 16, 96
    y = np.concatenate([np.arange(K)] * 4 + [rng.integers(0, K, n - 4 * K)])
    X = (rng.normal(0, 1.0, (K, NF))[y] + rng.normal(0, 1.0, (n, NF))).astype(np.float32)
    src = rng.integers(0, 3, n).astype(np.int64)
    return K, NF, X, y, src


def test_train_sweep_with_erm_balanced_and_dro_members_equals_train_classifier():
    from mermaid_classifier_amd import FeatureSet, SweepConfig, train_classifier, train_sweep
    from mermaid_classifier_amd.sampling import group_balance_weights
    K, NF, X, y, src = _python_data()
    sets = [FeatureSet(NF, np.arange(K)).append(X[s], y[s]) for s in (slice(0, 56), slice(56, 76), slice(76, 96))]
    groups, weights = src[:56], group_balance_weights(src[:56])
    base = dict(hidden_layer_sizes=(HIDDEN,), learning_rate_init=3e-3, alpha=1e-3, random_state=0, batch_size=gc.MB)
    configs = [SweepConfig(**base), SweepConfig(**base, row_weight=weights),
               SweepConfig(**base, row_group=groups, n_groups=3, group_dro_eta=0.0),
               SweepConfig(**base, row_group=groups, row_weight=weights, n_groups=3, group_dro_eta=0.5)]
    try:
        got = train_sweep(*sets, configs, 2, batch_size=30, early_stopping_patience=2)
        for i, cfg in enumerate(configs):
            cal, info, ref_accs = train_classifier(*sets, 2, batch_size=30, early_stopping_patience=2, clf=cfg.classifier(sets[1].device),
                                                   row_weight=cfg.row_weight, row_group=cfg.row_group)
            mine, my_info, my_accs = got[i]
            assert my_info == info and my_accs == ref_accs
            for u, v in zip(mine.weights + mine.biases, cal.weights + cal.biases):
                assert np.array_equal(u, v)
            assert np.array_equal(mine.a_, cal.a_) and np.array_equal(mine.b_, cal.b_)
        for i in range(1, 4):
            assert not all(np.array_equal(u, v) for u, v in zip(got[0][0].weights, got[i][0].weights))
    finally:
        for s in sets:
            s.close()


def test_classifier_keeps_group_weights_through_a_pickle():
    from mermaid_classifier_amd import FeatureSet
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    K, NF, X, y, src = _python_data()
    fs = FeatureSet(NF, np.arange(K)).append(X, y)
    try:
        clf = TorchMLPClassifier(hidden_layer_sizes=(HIDDEN,), random_state=0, batch_size=gc.MB, n_groups=3, group_dro_eta=1.0)
        rows = np.arange(10, 60)
        clf.partial_fit_rows(fs, rows, row_group=src)
        q = clf.group_weights_.copy()
        assert q.shape == (3,) and abs(q.sum() - 1.0) < 1e-12 and not np.allclose(q, 1 / 3)
        twin = pickle.loads(pickle.dumps(clf))
        assert twin.get_params() == clf.get_params() and np.array_equal(twin.group_weights_, q)
        for c in (clf, twin):
            c.partial_fit_rows(fs, rows, row_group=src, row_weight=np.linspace(0.5, 2.0, len(fs)))
        assert np.array_equal(clf.group_weights_, twin.group_weights_) and not np.array_equal(clf.group_weights_, q)
        for u, v in zip(sum(clf.parameters(), []), sum(twin.parameters(), [])):
            assert np.array_equal(u, v)
        assert clf.loss_curve_ == twin.loss_curve_
        plain = TorchMLPClassifier(hidden_layer_sizes=(HIDDEN,), random_state=0, batch_size=gc.MB)
        plain.partial_fit_rows(fs, rows)
        assert not hasattr(plain, "group_weights_")
    finally:
        fs.close()
