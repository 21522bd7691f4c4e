"""-m gpu: one step of the MLP trainer (``csrc/trainer.hip``) against the float64 reference of ``oracle/mlp_step_ref.py``, element by
element: |got - ref| <= 2 x the bound derived from the error model stated at the top of that module.  No quantile, no excluded
element; the factor 2 is the only margin over the derived worst case (second-order terms), as in ``tests/test_gpu_local.py``.

How a step is observed through the C ABI as it is: a trainer created with ``beta1 = 0`` has ``om_beta1 == 1.0f``, so from zero
moments ``exp_avg = 0 + 1 (g - 0) = g`` exactly and ``mmc_trainer_adam_state(which=0)`` after a one-step pass returns the step's
``gW[l]`` / ``gb[l]`` bit for bit; ``mmc_trainer_logits`` runs the forward GEMMs; the ``avg_loss`` of a one-step pass is
``loss_finalize_kernel``'s output.

a. gradients, logits and loss at the tile / step / block edges (``mlp_step_ref.CASES``);
b. the ragged last mini-batch of a two-step pass (lr = 1e-30: the first step leaves the parameters in place), host-fed, through
   the device gather of ``mmc_trainer_partial_fit_ordered`` and over a resident ``FeatureSet`` with a visiting order;
c. the Adam update: moments bit-equal to ``adam_f32``, step count, parameters within ``adam_param_ref``'s bound;
d. a heterogeneous group in one ``mmc_trainer_group_partial_fit_set`` call, each member against its own float64 reference;
e. one trainer through passes that grow, reuse and add to its device buffers, bit for bit against a fresh trainer per pass.

Measured max |got - ref| / bound per case and tensor: ``profiles/trainer_step_parity.txt`` (written per test into the directory
``MMC_TRAINER_STEP_PARITY_OUT`` names)."""

import ctypes as C
import os

import numpy as np
import pytest

from oracle import mlp_step_ref as sr

pytestmark = pytest.mark.gpu

FACTOR = 2.0
V = sr.V


class _Trainer:
    """An ``mmc_trainer`` through the C ABI alone."""

    def __init__(self, ws, bs, cw=None, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, alpha=sr.ALPHA):
        from mermaid_classifier_amd import _lib
        from mermaid_classifier_amd.torch_classifier import _ptr_array
        self._lib, self.lib, self._pa = _lib, _lib.lib(), _ptr_array
        self.shapes = [w.shape for w in ws]
        dims = [ws[0].shape[1]] + [w.shape[0] for w in ws]
        self.L, self.K, self.dim = len(ws), dims[-1], dims[0]
        ws, bs = [np.ascontiguousarray(w, np.float32) for w in ws], [np.ascontiguousarray(b, np.float32) for b in bs]
        cw = None if cw is None else np.ascontiguousarray(cw, np.float32)
        self.h = C.c_void_p()
        _lib.check(self.lib.mmc_trainer_create(_ptr_array(ws), _ptr_array(bs), (C.c_int * len(dims))(*dims), len(ws), lr, beta1, beta2,
                                               eps, alpha, None if cw is None else cw.ctypes.data_as(C.POINTER(C.c_float)), 0,
                                               C.byref(self.h)))

    def _empty(self):
        return [np.empty(s, np.float32) for s in self.shapes], [np.empty(s[0], np.float32) for s in self.shapes]

    def logits(self, X):
        X = np.ascontiguousarray(X, np.float32)
        z = np.full((len(X), self.K), np.nan, np.float32)
        self._lib.check(self.lib.mmc_trainer_logits(self.h, X.ctypes.data, len(X), z.ctypes.data, None))
        return z

    def fit(self, X, y, batch_size, order=None):
        """``mmc_trainer_partial_fit`` (rows as given), or ``_ordered`` with a visiting order -> (status, avg_loss)."""
        X, y32 = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(y, np.int32)
        avg = C.c_double(np.nan)
        if order is None:
            status = self.lib.mmc_trainer_partial_fit(self.h, X.ctypes.data, y32.ctypes.data, len(y32), batch_size, C.byref(avg), None)
        else:
            order = np.ascontiguousarray(order, np.int64)
            status = self.lib.mmc_trainer_partial_fit_ordered(self.h, X.ctypes.data, y32.ctypes.data, order.ctypes.data, len(y32),
                                                              batch_size, C.byref(avg), None)
        return status, avg.value

    def fit_set(self, fs, visit, batch_size):
        from mermaid_classifier_amd.backbone import _current_stream_ptr
        visit = np.ascontiguousarray(visit, np.int64)
        avg = C.c_double(np.nan)
        self._lib.check(self.lib.mmc_trainer_partial_fit_set(self.h, fs._handle(), visit.ctypes.data, len(visit), batch_size,
                                                             C.byref(avg), _current_stream_ptr(0)))
        return avg.value

    def params(self):
        ws, bs = self._empty()
        self._lib.check(self.lib.mmc_trainer_get_params(self.h, self._pa(ws), self._pa(bs)))
        return ws, bs

    def moments(self, which):
        ws, bs = self._empty()
        step = C.c_longlong(-1)
        self._lib.check(self.lib.mmc_trainer_adam_state(self.h, which, 0, self._pa(ws), self._pa(bs), C.byref(step)))
        return ws, bs, int(step.value)

    def set_moments(self, which, ws, bs, step):
        ws, bs = [np.ascontiguousarray(w, np.float32) for w in ws], [np.ascontiguousarray(b, np.float32) for b in bs]
        self._lib.check(self.lib.mmc_trainer_adam_state(self.h, which, 1, self._pa(ws), self._pa(bs), C.byref(C.c_longlong(step))))

    def fit_set_mixed(self, fs, visit, partner, lam, batch_size):
        from mermaid_classifier_amd.backbone import _current_stream_ptr
        visit, partner = np.ascontiguousarray(visit, np.int64), np.ascontiguousarray(partner, np.int64)
        lam = np.ascontiguousarray(lam, np.float32)
        avg = C.c_double(np.nan)
        self._lib.check(self.lib.mmc_trainer_partial_fit_set_mixed(self.h, fs._handle(), visit.ctypes.data, partner.ctypes.data,
                                                                   lam.ctypes.data, len(visit), batch_size, C.byref(avg),
                                                                   _current_stream_ptr(0)))
        return avg.value

    def set_options(self, max_norm, ema_decay, p_hidden, seed):
        self._lib.check(self.lib.mmc_trainer_set_grad_clip(self.h, max_norm))
        self._lib.check(self.lib.mmc_trainer_set_ema(self.h, ema_decay))
        self._lib.check(self.lib.mmc_trainer_set_dropout(self.h, 0.0, p_hidden, seed))

    def grad_norms(self):
        """The pre-clip norms of the last pass's steps (empty when it did not clip)."""
        out, steps = np.full(64, np.nan, np.float32), C.c_int(-1)
        self._lib.check(self.lib.mmc_trainer_grad_norms(self.h, out.ctypes.data, len(out), C.byref(steps)))
        assert 0 <= steps.value <= len(out)
        return out[:steps.value]

    def shadow(self):
        ws, bs = self._empty()
        self._lib.check(self.lib.mmc_trainer_ema_state(self.h, 0, self._pa(ws), self._pa(bs)))
        return ws, bs

    def set_shadow(self, ws, bs):
        self._lib.check(self.lib.mmc_trainer_ema_state(self.h, 1, self._pa(ws), self._pa(bs)))

    def close(self):
        self.lib.mmc_trainer_destroy(self.h)


def _named(gw, gb):
    out = {}
    for l, (w, b) in enumerate(zip(gw, gb)):
        out[f"gW{l}"], out[f"gb{l}"] = w, b
    return out


def _hold(label, L, got, ref, bound, lines, failures):
    """Every tensor of ``got`` per element against ``ref`` within FACTOR x ``bound``; one line per tensor."""
    for k, g in got.items():
        g = np.asarray(g)
        assert g.shape == ref[k].shape == bound[k].shape and np.isfinite(g).all() and np.isfinite(bound[k]).all(), (label, k)
        ratio, idx = sr.worst_ratio(g, ref[k], bound[k])
        lines.append(f"{label:34s} {k:7s} max|got-ref|/bound {ratio:7.4f} at {idx}")
        rep = sr.exceed_report(k, L, g, ref[k], bound[k], FACTOR)
        if rep:
            failures.append(f"{label}: {rep}")


def _finish(name, lines, failures):
    print("\n".join(lines))
    out_dir = os.environ.get("MMC_TRAINER_STEP_PARITY_OUT")      # tools: keep the table (profiles/trainer_step_parity.txt)
    if out_dir:
        with open(os.path.join(out_dir, f"trainer_step_parity_{name}.txt"), "w") as f:
            f.write("\n".join(lines + failures) + "\n")
    assert not failures, f"{len(failures)} tensors exceed {FACTOR:g} x bound\n" + "\n".join(failures)


def _one_step(t, X, y):
    """Logits before, then a one-step pass on a ``beta1 = 0`` trainer -> {name: tensor} as ``step_ref`` names them."""
    got = {"logits": t.logits(X)}
    status, avg = t.fit(X, y, len(y))
    assert status == 0, t.lib.mmc_last_error()
    gw, gb, step = t.moments(0)
    assert step == 1
    got["loss"] = np.asarray(avg)
    got.update(_named(gw, gb))
    return got


# ---- a. the edges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sr.CASES, ids=[c.id for c in sr.CASES])
def test_step_at_the_edges_within_twice_the_bound(case):
    ws, bs, cw, X, y = sr.make_case(case)
    ref, bound = sr.step_ref(ws, bs, X, y, sr.ALPHA, cw)
    t = _Trainer(ws, bs, cw, beta1=0.0)
    try:
        got = _one_step(t, X, y)
    finally:
        t.close()
    assert set(got) == set(ref)
    lines, failures = [f"# {case.id}: {case.what}"], []
    _hold(case.id, len(ws), got, ref, bound, lines, failures)
    _finish("a_" + case.id, lines, failures)


# ---- b. the ragged last mini-batch of a pass -----------------------------------------------------------------------------------------

ROUTES = [("host-67", 67), ("set-visit-67", 67), ("ordered-68", 68), ("set-visit-68", 68)]


@pytest.mark.parametrize("route,dim", ROUTES, ids=[r for r, _ in ROUTES])
def test_ragged_last_minibatch_of_a_pass(route, dim):
    """77 rows in mini-batches of 64 at lr = 1e-30: after the pass ``exp_avg = g1 + 1 (g2 - g1)``, the second step's gradient up to
    the two roundings 2 v max(|g1|, |g2|), which is added to the bound.  The device gather of ``mmc_trainer_partial_fit_ordered``
    moves float4 rows, so it takes widths that are a multiple of 4 only: width 67 goes host-fed and over a resident set (dword
    gather), width 68 through both device gathers."""
    from mermaid_classifier_amd import FeatureSet, _lib
    ws, bs, cw, X, y, order = sr.ragged_pass(dim)
    assert not np.array_equal(order, np.arange(77))
    steps = [sr.step_ref(ws, bs, X[order[s]], y[order[s]], sr.ALPHA, cw) for s in (slice(0, 64), slice(64, 77))]
    (r1, b1), (r2, b2) = steps
    ref = {k: v for k, v in r2.items() if k != "logits"}
    bound = {k: b2[k] + 2.0 * V * np.maximum(np.abs(r1[k]), np.abs(r2[k])) for k in ref if k != "loss"}
    ref["loss"] = np.asarray((64.0 * r1["loss"] + 13.0 * r2["loss"]) / 77.0)
    bound["loss"] = np.asarray((64.0 * b1["loss"] + 13.0 * b2["loss"]) / 77.0)
    t = _Trainer(ws, bs, cw, lr=1e-30, beta1=0.0)
    fs = None
    try:
        if route.startswith("host"):
            assert t.fit(X, y, 64, order)[0] == _lib.MMC_ERR_ARG        # no device gather at this width; nothing ran
            assert t.moments(0)[2] == 0
            status, avg = t.fit(X[order], y[order], 64)
            assert status == 0, t.lib.mmc_last_error()
        elif route.startswith("ordered"):
            status, avg = t.fit(X, y, 64, order)
            assert status == 0, t.lib.mmc_last_error()
        else:
            fs = FeatureSet(dim, np.arange(7)).append(X, y)
            avg = t.fit_set(fs, order, 64)
        gw, gb, step = t.moments(0)
        pw, pb = t.params()
    finally:
        t.close()
        if fs is not None:
            fs.close()
    assert step == 2
    moved = max(float(np.abs(a - b).max()) for a, b in zip(pw + pb, ws + bs))
    assert moved <= 1e-29, moved                                     # two steps of at most 1e-30 |m / denom|
    got = {"loss": np.asarray(avg), **_named(gw, gb)}
    lines, failures = [f"# {route}: second step of 64 + 13 rows, mb 13"], []
    _hold(route, len(ws), got, ref, bound, lines, failures)
    _finish("b_" + route, lines, failures)


# ---- c. the Adam update, bit for bit ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def twin_gradient():
    """The gradient of one step on dims [67, 129, 18, 7], 77 rows, from a ``beta1 = 0`` twin: what any trainer on the same parameters
    and rows consumes, whatever its optimizer settings (a step is bit-reproducible)."""
    case = sr.CASES[4]
    assert case.dims == (67, 129, 18, 7) and all(int(np.prod(w.shape)) % 256 for w in sr.make_case(case)[0])
    ws, bs, cw, X, y = sr.make_case(case)
    t = _Trainer(ws, bs, cw, beta1=0.0)
    try:
        status, _ = t.fit(X, y, len(y))
        assert status == 0
        gw, gb, _ = t.moments(0)
    finally:
        t.close()
    return ws, bs, cw, X, y, gw + gb


@pytest.mark.parametrize("step0", [0, 1000])
def test_adam_update_bit_for_bit(twin_gradient, step0):
    ws, bs, cw, X, y, g = twin_gradient
    rng = np.random.default_rng([9, step0])
    p0 = ws + bs
    m0 = [(1e-3 * rng.standard_normal(p.shape)).astype(np.float32) for p in p0]
    v0 = [rng.uniform(1e-9, 1e-5, p.shape).astype(np.float32) for p in p0]
    for m, v in zip(m0, v0):                                         # exact zeros in each moment, some in both
        zm, zv = rng.random(m.shape) < 0.1, rng.random(m.shape) < 0.1
        zm.flat[:3], zv.flat[:3] = (True, False, True), (False, True, True)
        m[zm] = 0
        v[zv] = 0
        assert (v >= 0).all() and (v > 0).any() and (zm & zv).any() and (zm & ~zv).any() and (zv & ~zm).any()
    L = len(ws)
    t = _Trainer(ws, bs, cw)                                         # the defaults: 0.9, 0.999, 1e-8, lr 1e-3
    try:
        t.set_moments(0, m0[:L], m0[L:], step0)
        t.set_moments(1, v0[:L], v0[L:], step0)
        status, _ = t.fit(X, y, len(y))
        assert status == 0, t.lib.mmc_last_error()
        mw, mb_, step_m = t.moments(0)
        vw, vb, step_v = t.moments(1)
        pw, pb = t.params()
    finally:
        t.close()
    assert step_m == step_v == step0 + 1
    s = sr.adam_scalars(step0 + 1)
    names = [f"W{l}" for l in range(L)] + [f"b{l}" for l in range(L)]
    lines, failures = [f"# Adam from step {step0}: parameters, max |got - ref| / bound (bound: v |p'| + 7 v |step_size m' / denom|)"], []
    for name, gi, mi, vi, pi, m1, v1, p1 in zip(names, g, m0, v0, p0, mw + mb_, vw + vb, pw + pb):
        em, ev = sr.adam_f32(gi, mi, vi, s)
        assert np.array_equal(m1, em), f"exp_avg of {name}: {int((m1 != em).sum())} of {em.size} elements differ"
        assert np.array_equal(v1, ev), f"exp_avg_sq of {name}: {int((v1 != ev).sum())} of {ev.size} elements differ"
        ref, bound = sr.adam_param_ref(pi, em, ev, s)
        ratio, idx = sr.worst_ratio(p1, ref, bound)
        lines.append(f"adam-step{step0:<25d} {name:7s} max|got-ref|/bound {ratio:7.4f} at {idx}")
        over = np.abs(p1.astype(np.float64) - ref) > bound
        if over.any():
            failures.append(f"{name} [adam_kernel]: worst element {idx}: got {float(p1[idx]):.9g} ref {float(ref[idx]):.9g} bound "
                            f"{float(bound[idx]):.3g}; {int(over.sum())} of {over.size} elements over the bound")
    _finish(f"c_adam_step{step0}", lines, failures)


# ---- d. a heterogeneous group ------------------------------------------------------------------------------------------------------------

def test_heterogeneous_group_each_member_against_fp64():
    """Three members of depth 3, 1 and 2 with 77, 13 and 64 rows in one call: the grid is the largest member's, the shallow member
    sits out of the hidden-layer launches, and the members differ in M, N and K in every launch."""
    from mermaid_classifier_amd import FeatureSet, _lib
    from mermaid_classifier_amd.backbone import _current_stream_ptr
    X, y, members = sr.group_pass()
    assert [[w.shape[0] for w in m[0]] for m in members] == [[129, 18, 7], [7], [300, 7]] and [len(m[3]) for m in members] == [77, 13, 64]
    refs = [sr.step_ref(ws, bs, X[visit], y[visit], sr.ALPHA, cw) for ws, bs, cw, visit in members]
    fs = FeatureSet(67, np.arange(7)).append(X, y)
    ts = [_Trainer(ws, bs, cw, beta1=0.0) for ws, bs, cw, _ in members]
    try:
        got = [{"logits": t.logits(X[m[3]])} for t, m in zip(ts, members)]
        count = len(ts)
        visits = [np.ascontiguousarray(m[3], np.int64) for m in members]
        avg = (C.c_double * count)()
        _lib.check(_lib.lib().mmc_trainer_group_partial_fit_set(
            (C.c_void_p * count)(*[t.h.value for t in ts]), count, fs._handle(), (C.c_void_p * count)(*[v.ctypes.data for v in visits]),
            (C.c_int64 * count)(*[len(v) for v in visits]), (C.c_int * count)(*[len(v) for v in visits]), avg, _current_stream_ptr(0)))
        for i, t in enumerate(ts):
            gw, gb, step = t.moments(0)
            assert step == 1
            got[i]["loss"] = np.asarray(avg[i])
            got[i].update(_named(gw, gb))
    finally:
        for t in ts:
            t.close()
        fs.close()
    lines, failures = ["# one mmc_trainer_group_partial_fit_set call: dims [67,129,18,7] x 77 rows, [67,7] x 13, [67,300,7] x 64"], []
    for i, (ref, bound) in enumerate(refs):
        assert set(got[i]) == set(ref)
        _hold(f"group-member{i}", len(members[i][0]), got[i], ref, bound, lines, failures)
    _finish("d_group", lines, failures)


# ---- e. one trainer whose buffers grow, stay and gain the optional ones, against fresh trainers -------------------------------------

def test_one_trainer_through_growing_passes_matches_fresh_trainers(monkeypatch):
    """Handle A (8 -> 12 -> 5, class weights) takes five passes that grow its staging, activation and loss buffers, reuse them at a
    smaller size, and allocate the ordered pass's, the visiting order's, the mixing plan's, the clipping and the shadow buffers.
    Before each pass a fresh trainer B is made from A's parameters, moments, step count, options and shadow, and takes that pass
    alone: afterwards A and B agree bit for bit in parameters, both moments, step count, avg_loss, the gradient norms and the
    shadow -- what a buffer held before, or how large it once was, changes nothing."""
    from mermaid_classifier_amd import FeatureSet
    rng = np.random.default_rng(20261)
    dims = [8, 12, 5]
    ws = [(rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l])).astype(np.float32) for l in range(2)]
    bs = [(0.1 * rng.standard_normal(dims[l + 1])).astype(np.float32) for l in range(2)]
    cw = np.array([1.0, 0.5, 2.0, 1.5, 0.75], np.float32)
    X = rng.standard_normal((70, 8)).astype(np.float32)
    y = (np.arange(70) % 5).astype(np.int32)
    order = rng.permutation(70)
    visit9 = rng.permutation(40)[:9]
    visit40, partner40 = rng.permutation(40), rng.integers(0, 40, 40)
    lam = rng.uniform(0.2, 0.8, 3).astype(np.float32)                    # ceil(40 / 16) mini-batches
    opts = dict(max_norm=0.5, ema_decay=0.9, p_hidden=0.25, seed=77)
    fs = FeatureSet(8, np.arange(5)).append(X[:40], y[:40])

    def host6(t):
        status, avg = t.fit(X[:6], y[:6], 4)                            # 4 + 2 rows: a ragged last step
        assert status == 0, t.lib.mmc_last_error()
        return avg

    def ordered70(t):
        status, avg = t.fit(X, y, 32, order)
        assert status == 0, t.lib.mmc_last_error()
        return avg

    def set9(t):                                                        # chunks of 8 and 1 rows
        monkeypatch.setenv("MMC_TRAIN_CHUNK_ROWS", "8")
        try:
            return t.fit_set(fs, visit9, 4)
        finally:
            monkeypatch.delenv("MMC_TRAIN_CHUNK_ROWS")

    def mixed40(t):
        return t.fit_set_mixed(fs, visit40, partner40, lam, 16)

    def observe(t, with_options):
        mw, mb, step = t.moments(0)
        vw, vb, step2 = t.moments(1)
        assert step == step2
        state = {"params": t.params(), "m": (mw, mb), "v": (vw, vb), "step": step, "gnorm": t.grad_norms()}
        if with_options:
            state["shadow"] = t.shadow()
        return state

    def flat(v):
        return np.concatenate([np.ravel(a) for a in v[0] + v[1]]) if isinstance(v, tuple) else np.atleast_1d(np.asarray(v))

    a = _Trainer(ws, bs, cw)
    try:
        with_options = False
        for name, run, steps, turn_on in [("host-6", host6, 2, False), ("ordered-70", ordered70, 3, False), ("set-visit-9", set9, 3, False),
                                          ("mixed-40", mixed40, 3, True), ("host-6-again", host6, 2, False)]:
            if turn_on:
                a.set_options(**opts)
                with_options = True
            before = observe(a, with_options)
            b = _Trainer(*before["params"], cw)
            try:
                b.set_moments(0, *before["m"], before["step"])
                b.set_moments(1, *before["v"], before["step"])
                if with_options:
                    b.set_options(**opts)
                    b.set_shadow(*before["shadow"])
                got_b = {"avg_loss": run(b), **observe(b, with_options)}
            finally:
                b.close()
            got_a = {"avg_loss": run(a), **observe(a, with_options)}
            assert got_a["step"] == before["step"] + steps and np.isfinite(got_a["avg_loss"]), name
            assert len(got_a["gnorm"]) == (steps if with_options else 0), name
            assert not np.array_equal(flat(got_a["params"]), flat(before["params"])), name      # the pass did train
            for k in got_a:
                fa, fb = flat(got_a[k]), flat(got_b[k])
                assert fa.shape == fb.shape and fa.tobytes() == fb.tobytes(), (name, k, float(np.abs(fa - fb).max()))
    finally:
        a.close()
        fs.close()
