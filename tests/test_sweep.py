"""A sweep of MLP heads trained in one pass: ``mmc_trainer_group_partial_fit_set``, ``partial_fit_rows_group``, ``sweep_loop``
and ``train_sweep``.

CPU: C-ABI and Python argument errors that need no device; ``sweep_loop``'s bookkeeping with fake classifiers and scripted
validation losses, against ``epoch_loop`` on the same script.
GPU (-m gpu): every comparison is ``np.array_equal`` on parameters, both Adam moments, step count, ``loss_curve_`` and
``n_iter_`` against clones trained by the solo ``partial_fit_rows`` -- the solo call is a group of one in the same kernels, and no
reduction's decomposition depends on the group, so there is nothing to tolerate.  Data: tests/golden/trainer_fixture.npz (730 x 64,
7 classes; the weighted variant has one class of weight 0)."""

import ctypes as C
import pickle

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def fx():
    d = dict(np.load(GOLDEN / "trainer_fixture.npz"))
    d["y"] = d["classes"][d["y_idx"]]
    return d


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_group_c_abi_argument_errors_without_device():
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    vp = C.c_void_p
    assert _lib.MMC_TRAINER_GROUP_MAX == 16
    one = (vp * 1)(1234)          # never dereferenced: the calls below fail before a member is looked at
    visit, n, bs = (vp * 1)(None), (C.c_int64 * 1)(5), (C.c_int * 1)(2)
    avg = (C.c_double * 1)(7.0)
    for args in ((None, 1, None, visit, n, bs), (one, 1, None, None, n, bs), (one, 1, None, visit, None, bs),
                 (one, 1, None, visit, n, None)):
        avg[0] = 7.0
        assert lib.mmc_trainer_group_partial_fit_set(*args, avg, None) == _lib.MMC_ERR_ARG
        assert b"NULL" in lib.mmc_last_error() and avg[0] == 0.0          # zeroed on failure
    big = (vp * 17)(*[1234] * 17)
    for count in (0, -3, 17):
        assert lib.mmc_trainer_group_partial_fit_set(big, count, None, (vp * 17)(), (C.c_int64 * 17)(), (C.c_int * 17)(), None,
                                                     None) == _lib.MMC_ERR_ARG
        assert b"count" in lib.mmc_last_error()
    members = (vp * 3)(None, None, None)
    avg3 = (C.c_double * 3)(1.0, 2.0, 3.0)
    assert lib.mmc_trainer_group_partial_fit_set(members, 3, None, (vp * 3)(), (C.c_int64 * 3)(1, 1, 1), (C.c_int * 3)(1, 1, 1), avg3,
                                                 None) == _lib.MMC_ERR_ARG
    assert b"member 0" in lib.mmc_last_error() and list(avg3) == [0.0, 0.0, 0.0]
    same = (vp * 2)(1234, 1234)
    assert lib.mmc_trainer_group_partial_fit_set(same, 2, None, (vp * 2)(), (C.c_int64 * 2)(1, 1), (C.c_int * 2)(1, 1), None,
                                                 None) == _lib.MMC_ERR_ARG
    assert b"same trainer" in lib.mmc_last_error()
    assert lib.mmc_trainer_group_partial_fit_set(one, 1, None, visit, n, bs, avg, None) == _lib.MMC_ERR_ARG    # no feature set
    assert b"feature set" in lib.mmc_last_error()


def test_group_python_argument_errors_without_device():
    import mermaid_classifier_amd as pkg
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    assert pkg.partial_fit_rows_group is not None and pkg.train_sweep is not None and pkg.SweepConfig is not None
    fs = pkg.FeatureSet(4, ["a", "b", "c"])
    a, b = TorchMLPClassifier(), TorchMLPClassifier()
    with pytest.raises(ValueError, match="1 entries for 2 classifiers"):
        pkg.partial_fit_rows_group([a, b], fs, rows=[np.arange(3)])
    with pytest.raises(ValueError, match="3 entries for 2 classifiers"):
        pkg.partial_fit_rows_group([a, b], fs, rows=[None, np.arange(3), None])
    with pytest.raises(ValueError, match="twice"):
        pkg.partial_fit_rows_group([a, b, a], fs)
    with pytest.raises(ValueError, match="row indices"):
        pkg.partial_fit_rows_group([a, b], fs, rows=np.array([0.5, 1.0]))
    with pytest.raises(ValueError, match="row indices"):
        pkg.partial_fit_rows_group([a, b], fs, rows=[np.arange(3), np.zeros((2, 2), np.int64)])
    with pytest.raises(ValueError, match="classifier 1 is on device 1"):
        pkg.partial_fit_rows_group([a, TorchMLPClassifier(device="cuda:1")], fs)
    assert not a._fitted() and not b._fitted()                      # nothing was initialised on the way to those errors
    cfg = pkg.SweepConfig(hidden_layer_sizes=[8, 4], learning_rate_init=0.5, alpha=0.0, class_weight={"a": 1.0}, random_state=None,
                          batch_size=32, beta_1=0.8, beta_2=0.9, epsilon=1e-6)
    clf = cfg.classifier(device="cuda:0")
    assert clf.get_params() == dict(TorchMLPClassifier().get_params(), hidden_layer_sizes=(8, 4), learning_rate_init=0.5, alpha=0.0,
                                    class_weight={"a": 1.0}, random_state=None, batch_size=32, beta_1=0.8, beta_2=0.9, epsilon=1e-6)
    prod = pkg.SweepConfig().classifier()
    assert prod.hidden_layer_sizes == (500, 300, 100) and prod.learning_rate_init == 1e-4 and prod.random_state == 0
    with pytest.raises(ValueError, match="configs is empty"):
        pkg.train_sweep(fs, fs, fs, [], 3, batch_size=10)
    with pytest.raises(ValueError, match="empty"):
        pkg.train_sweep(fs, fs, fs, [cfg], 3, batch_size=10)
    with pytest.raises(ValueError, match="batch_size"):
        pkg.train_sweep(fs, fs, fs, [cfg], 3, batch_size=0)


class _Fake:
    """A 'classifier' that counts its passes."""

    def __init__(self, name):
        self.name = name
        self.count = 0
        self.loss_curve_ = []


def _scripted(script):
    """Device steps over fakes: a pass counts; the validation loss of a model's k-th evaluation is script[name][k]."""
    evals = {name: 0 for name in script}
    log = []

    def fit_group(models, rows):
        log.append(([m.name for m in models], list(rows)))
        for m in models:
            m.count += 1
            m.loss_curve_.append(10.0 - m.count)

    def eval_val(m):
        evals[m.name] += 1
        return 0.5 + 0.01 * m.count, script[m.name][evals[m.name] - 1]

    return fit_group, (lambda m: 0.25 * m.count), eval_val, log


_SCRIPT = {"early": [.90, .80, .85, .80, .70, .10],                 # best at epoch 2, out of patience after 4
           "nan": [.9, float("nan"), .5, .6, float("nan"), .1],     # a NaN is no improvement; best at 3, stops after 5
           "late": [.9, .8, .7, .6, .5, .4]}                        # improves to the end of the budget


def test_sweep_loop_bookkeeping_is_epoch_loops_per_model():
    from mermaid_classifier_amd.sweep import sweep_loop
    from mermaid_classifier_amd.training import epoch_loop
    names = list(_SCRIPT)
    passes = {"early": 2, "nan": 1, "late": 3}                       # outer batches per epoch
    batches = [lambda epoch, nm=nm: [(nm, epoch, p) for p in range(passes[nm])] for nm in names]
    fit_group, eval_ref, eval_val, log = _scripted(_SCRIPT)
    seen = []
    got = sweep_loop([_Fake(nm) for nm in names], batches, fit_group, eval_ref, eval_val, 6, early_stopping_patience=2,
                     on_epoch_end=seen.append)
    # one group call per outer batch position, over the models that have a batch there and are still running
    want_log = []
    for epoch in range(6):
        running = [nm for nm in names if epoch < {"early": 4, "nan": 5, "late": 6}[nm]]
        for p in range(3):
            group = [nm for nm in running if p < passes[nm]]
            if group:
                want_log.append((group, [(nm, epoch, p) for nm in group]))
    assert log == want_log
    assert [(m["config"], m["epoch"]) for m in seen] == [(i, e) for e in range(6) for i, nm in enumerate(names)
                                                         if e < {"early": 4, "nan": 5, "late": 6}[nm]]
    # per model: exactly what epoch_loop makes of the same script
    for i, nm in enumerate(names):
        f, r, v, _ = _scripted({nm: _SCRIPT[nm]})
        solo_seen = []

        def train_epoch(clf, epoch, nm=nm, f=f):
            for p in range(passes[nm]):
                f([clf], [None])
        want_clf, want_info = epoch_loop(_Fake(nm), train_epoch, r, v, 6, early_stopping_patience=2, on_epoch_end=solo_seen.append)
        clf, info = got[i]
        assert info == want_info
        assert (clf.name, clf.count, clf.loss_curve_) == (nm, want_clf.count, want_clf.loss_curve_)   # the restore is per model
        mine = [{k: v for k, v in m.items() if k not in ("cumulative_seconds", "config")} for m in seen if m["config"] == i]
        assert mine == [{k: v for k, v in m.items() if k != "cumulative_seconds"} for m in solo_seen]
    assert [info["final_epoch"] for _, info in got] == [4, 5, 6]
    assert [info["best_val_epoch"] for _, info in got] == [2, 3, 6]
    assert [clf.count for clf, _ in got] == [2 * 2, 3 * 1, 6 * 3]
    assert got[0][1]["stop_reason"] == got[1][1]["stop_reason"] == "early_stopping" and got[2][1]["stop_reason"] == "budget_exhausted"


def test_sweep_loop_without_patience_and_bad_arguments():
    from mermaid_classifier_amd.sweep import sweep_loop
    fit_group, eval_ref, eval_val, log = _scripted({"a": [.5, .9, .95], "b": [.1, .2, .3]})
    got = sweep_loop([_Fake("a"), _Fake("b")], [lambda e: [0]] * 2, fit_group, eval_ref, eval_val, 3)
    assert [clf.count for clf, _ in got] == [3, 3] and len(log) == 3
    assert got[0][1] == {"enabled": False, "patience": None, "stop_reason": "budget_exhausted", "final_epoch": 3,
                         "best_val_epoch": None, "best_val_loss": None}
    with pytest.raises(ValueError, match="early_stopping_patience"):
        sweep_loop([_Fake("a")], [lambda e: [0]], fit_group, eval_ref, eval_val, 3, early_stopping_patience=0)
    with pytest.raises(ValueError, match="nbr_epochs"):
        sweep_loop([_Fake("a")], [lambda e: [0]], fit_group, eval_ref, eval_val, 0)
    with pytest.raises(ValueError, match="batch callables"):
        sweep_loop([_Fake("a")], [], fit_group, eval_ref, eval_val, 3)


# ---- GPU --------------------------------------------------------------------------------------------------------------------
def _weights(fx):
    return {c: float(w) for c, w in zip(fx["classes"], fx["class_weight"])}


def _clf(fx, hidden=(48, 32), weighted=False, **kw):
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    args = dict(hidden_layer_sizes=hidden, learning_rate_init=1e-3, alpha=1e-3, random_state=0,
                class_weight=_weights(fx) if weighted else None)
    args.update(kw)
    return TorchMLPClassifier(**args)


def _fill(fx):
    from mermaid_classifier_amd import FeatureSet
    return FeatureSet(64, fx["classes"], reserve=730).append(fx["X"], fx["y"])


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


def _heterogeneous(fx):
    """The five members of the issue's first GPU test, with their rows: depths 1 to 4, widths that are no multiple of 16,
    4 / 6 / 1 / 1 / 4 steps a pass, weighted and plain, with and without a visiting order."""
    return [(_clf(fx, (48, 32), weighted=True, batch_size=200), None),
            (_clf(fx, (70,), learning_rate_init=3e-3, alpha=0.0, batch_size=64), np.arange(729, -1, -2)),
            (_clf(fx, (), batch_size="auto"), np.arange(0, 97 * 7, 7)),
            (_clf(fx, (33, 17, 9), random_state=3, batch_size=730), None),
            (_clf(fx, (48, 32), shuffle=False), None)]


@pytest.fixture(scope="module")
def solo_heterogeneous(fx):
    """Three solo passes per member: what the group passes must reproduce bit for bit (computed once, left unchanged)."""
    fs = _fill(fx)
    out = []
    for clf, rows in _heterogeneous(fx):
        for _ in range(3):
            clf.partial_fit_rows(fs, rows, classes=fx["classes"].tolist())
        out.append(_state(clf))
    fs.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_rows", ["256", None])
def test_heterogeneous_group_has_the_bits_of_the_solo_passes(fx, solo_heterogeneous, monkeypatch, chunk_rows):
    """At MMC_TRAIN_CHUNK_ROWS=256 the members' chunks are 200, 256, 194, 730 and 200 rows: chunk boundaries fall at different
    steps per member (every step; after four steps; never); the default takes every pass in one chunk."""
    from mermaid_classifier_amd import partial_fit_rows_group
    if chunk_rows is None:
        monkeypatch.delenv("MMC_TRAIN_CHUNK_ROWS", raising=False)
    else:
        monkeypatch.setenv("MMC_TRAIN_CHUNK_ROWS", chunk_rows)
    fs = _fill(fx)
    members = _heterogeneous(fx)
    clfs, rows = [c for c, _ in members], [r for _, r in members]
    for _ in range(3):
        assert partial_fit_rows_group(clfs, fs, rows, classes=fx["classes"].tolist()) == clfs
    assert [c._adam_state()["step"] for c in clfs] == [12, 18, 3, 3, 12]
    for clf, want in zip(clfs, solo_heterogeneous):
        _assert_same_state(clf, want)
    fs.close()


@pytest.fixture(scope="module")
def solo_plain(fx):
    fs = _fill(fx)
    clf = _clf(fx)
    for _ in range(2):
        clf.partial_fit_rows(fs, classes=fx["classes"].tolist())
    fs.close()
    return _state(clf)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 16, 17])
def test_identical_members_do_not_interfere(fx, solo_plain, count):
    """A group of one; sixteen identical members in one call (any cross-member mix-up shows); seventeen split into 16 + 1."""
    from mermaid_classifier_amd import partial_fit_rows_group
    fs = _fill(fx)
    clfs = [_clf(fx) for _ in range(count)]
    for _ in range(2):
        partial_fit_rows_group(clfs, fs, classes=fx["classes"].tolist())
    for clf in clfs:
        _assert_same_state(clf, solo_plain)
    fs.close()


@pytest.mark.gpu
def test_group_odd_feature_width():
    """Width 10: rows are neither 16-byte sized nor aligned, the gather moves dwords."""
    from mermaid_classifier_amd import FeatureSet, partial_fit_rows_group
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    rng = np.random.default_rng(2)
    k, nf, n = 5, 10, 333
    yi = rng.integers(0, k, size=n)
    X = (rng.normal(0, 1, size=(k, nf))[yi] + rng.normal(0, 1, size=(n, nf))).astype(np.float32)
    fs = FeatureSet(nf, np.arange(k)).append(X[:100], yi[:100]).append(X[100:], yi[100:])
    make = lambda: [TorchMLPClassifier(hidden_layer_sizes=(16,), batch_size=50, random_state=1),
                    TorchMLPClassifier(hidden_layer_sizes=(21, 5), batch_size=64, random_state=2)]
    group, solo = make(), make()
    rows = [None, np.arange(0, n, 3)]
    for _ in range(2):
        partial_fit_rows_group(group, fs, rows, classes=list(range(k)))
        for clf, r in zip(solo, rows):
            clf.partial_fit_rows(fs, r, classes=list(range(k)))
    for a, b in zip(group, solo):
        _assert_same_state(a, b)
    fs.close()


def _c_group_call(clfs, fs, visits, ns, batch_sizes):
    from mermaid_classifier_amd import _lib
    count = len(clfs)
    visits = [None if v is None else np.ascontiguousarray(v, dtype=np.int64) for v in visits]
    avg = (C.c_double * count)(*[7.0] * count)
    status = _lib.lib().mmc_trainer_group_partial_fit_set(
        (C.c_void_p * count)(*[c._h.value for c in clfs]), count, fs._handle(),
        (C.c_void_p * count)(*[None if v is None else v.ctypes.data for v in visits]), (C.c_int64 * count)(*ns),
        (C.c_int * count)(*batch_sizes), avg, None)
    return status, list(avg), _lib.lib().mmc_last_error()


@pytest.mark.gpu
def test_rejected_group_calls_leave_every_member_untouched(fx):
    from mermaid_classifier_amd import FeatureSet, _lib, partial_fit_rows_group
    fs = _fill(fx)
    classes = fx["classes"].tolist()
    make = lambda: [_clf(fx, (48, 32), weighted=True), _clf(fx, (70,)), _clf(fx, (33, 17), weighted=True, random_state=3)]
    group, solo = make(), make()
    partial_fit_rows_group(group, fs, classes=classes)
    for clf in solo:
        clf.partial_fit_rows(fs, classes=classes)
    before = [_state(c) for c in group]
    zero = fx["classes"][np.flatnonzero(fx["class_weight"] == 0)[0]]
    dead = np.flatnonzero(fx["y"] == zero)
    assert dead.size > 0
    order = np.arange(730)
    other = FeatureSet(64, np.arange(5)).append(fx["X"][:50], np.arange(50) % 5)
    five = _clf(fx, (8,), learning_rate_init=1e-3)                       # a trainer with five classes
    five.partial_fit_rows(other)
    five_before = _state(five)
    cases = [
        ("zero weight", group, [dead, order, order], [dead.size, 730, 730], b"member 0: mini-batch 0 has zero total class weight"),
        ("visit out of range in the last member", group, [order, order, np.array([3, 730])], [730, 730, 2], b"member 2: visit[1] = 730 outside"),
        ("same handle twice", [group[0], group[1], group[0]], [order] * 3, [730] * 3, b"member 2 is the same trainer as member 0"),
        ("another class count", [group[0], five, group[2]], [order] * 3, [730] * 3, b"member 1: feature set has 7 classes, trainer 5"),
    ]
    for what, members, visits, ns, message in cases:
        status, avg, err = _c_group_call(members, fs, visits, ns, [200] * 3)
        assert status == _lib.MMC_ERR_ARG and message in err and avg == [0.0, 0.0, 0.0], (what, status, err, avg)
        for clf, want in zip(group, before):
            _assert_same_state(clf, want)
        _assert_same_state(five, five_before)
    with pytest.raises(ValueError, match="member 0: mini-batch 0 has zero total class weight"):
        partial_fit_rows_group(group, fs, [dead, None, None])
    assert [c.n_iter_ for c in group] == [1, 1, 1]
    partial_fit_rows_group(group, fs)
    for a, b in zip(group, solo):
        b.partial_fit_rows(fs)
        _assert_same_state(a, b)
    fs.close()
    other.close()


@pytest.mark.gpu
def test_solo_and_group_passes_mix(fx):
    """solo, group, solo equals three solo passes; a pickled and restored member carries on in a group like the original."""
    from mermaid_classifier_amd import partial_fit_rows_group
    fs = _fill(fx)
    classes = fx["classes"].tolist()
    rows = np.arange(729, -1, -2)
    a, want, mate = _clf(fx, weighted=True), _clf(fx, weighted=True), _clf(fx, (70,))
    for _ in range(3):
        want.partial_fit_rows(fs, rows, classes=classes)
    a.partial_fit_rows(fs, rows, classes=classes)
    partial_fit_rows_group([mate, a], fs, [None, rows], classes=classes)
    a.partial_fit_rows(fs, rows)
    _assert_same_state(a, want)
    b = pickle.loads(pickle.dumps(a))
    _assert_same_state(b, want)
    partial_fit_rows_group([a, mate, b], fs, [rows, None, rows])
    want.partial_fit_rows(fs, rows)
    _assert_same_state(a, want)
    _assert_same_state(b, want)
    fs.close()


def _subsample(epoch):
    """A row-subset hook: three uneven batches of a per-epoch permutation of the 500 train rows."""
    order = np.random.default_rng(100 + epoch).permutation(500)
    return [order[:150], order[150:290], order[290:400]]


@pytest.mark.gpu
def test_train_sweep_equals_train_classifier_per_config(fx):
    """Three configurations chosen with the CPU restatement oracle/mlp_train_ref.py on this split (patience 2, 12 epochs): the
    slow one improves to the end of the budget, lr 3e-2 on one hidden layer overfits at once (best epoch 1, stop after 3), and the
    class-weighted one on a per-epoch subsample (the `batches` hook: fewer rows, three outer batches instead of two) stops in
    between (best epoch 5, stop after 7 there)."""
    from mermaid_classifier_amd import FeatureSet, SweepConfig, train_classifier, train_sweep
    X, y, classes = fx["X"], fx["y"], fx["classes"].tolist()
    sets = [FeatureSet(64, classes).append(X[s], y[s]) for s in (slice(0, 500), slice(500, 630), slice(630, 730))]
    configs = [SweepConfig(hidden_layer_sizes=(48, 32), learning_rate_init=1e-3, alpha=1e-3, random_state=0),
               SweepConfig(hidden_layer_sizes=(70,), learning_rate_init=3e-2, alpha=0.0, random_state=1, batch_size=50),
               SweepConfig(hidden_layer_sizes=(48, 32), learning_rate_init=3e-3, alpha=1e-3, random_state=0, batch_size=50,
                           class_weight=_weights(fx), batches=_subsample)]
    seen = []
    got = train_sweep(*sets, configs, 12, batch_size=300, early_stopping_patience=2, on_epoch_end=seen.append)
    assert len(got) == 3
    finals = []
    for i, cfg in enumerate(configs):
        solo_seen = []
        cal, info, ref_accs = train_classifier(*sets, 12, batch_size=300, early_stopping_patience=2, on_epoch_end=solo_seen.append,
                                               batches=cfg.batches, clf=cfg.classifier(sets[1].device))
        print("config", i, "info", info, "val losses", [m["val_loss"] for m in solo_seen])
        finals.append(info["final_epoch"])
        mine, my_info, my_accs = got[i]
        assert my_info == info and my_accs == ref_accs and len(ref_accs) == info["final_epoch"]
        assert len(mine.weights) == len(cal.weights)
        for u, v in zip(mine.weights + mine.biases, cal.weights + cal.biases):
            assert np.array_equal(u, v)
        assert np.array_equal(mine.a_, cal.a_) and np.array_equal(mine.b_, cal.b_)
        strip = lambda ms: [{k: v for k, v in m.items() if k not in ("cumulative_seconds", "config")} for m in ms]
        assert strip(m for m in seen if m["config"] == i) == strip(solo_seen)
    assert len(set(finals)) > 1, finals          # the precondition: the solo runs do not all stop at the same epoch
    for s in sets:
        s.close()
