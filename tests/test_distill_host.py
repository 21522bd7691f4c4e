"""Distillation without a device: the ABI's declarations, the Python-side argument checks, the fp32 emulation of the stage against
the bounds of tests/distill_checker.py, wrong kernels against the same bounds, Gibbs' inequality, and the float64 training evidence
that the README's entry quotes."""

import dataclasses
import re
from pathlib import Path

import numpy as np
import pytest

import distill_checker as dc
import loss_checker as lc

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ["mmc_targetset_create", "mmc_targetset_rows", "mmc_targetset_num_classes", "mmc_targetset_append",
               "mmc_targetset_read", "mmc_ensemble_predict_set", "mmc_trainer_set_distillation", "mmc_trainer_partial_fit_set_distill",
               "mmc_trainer_group_partial_fit_set_distill", "mmc_trainer_loss_gradient_distill",
               "mmc_trainer_loss_gradient_distill_weighted"]
KINDS, _opts, _peak = dc.KINDS, dc.kind_options, dc.peak


def test_header_declares_and_symbols_list_every_entry_point():
    header = (ROOT / "include" / "mmc.h").read_text()
    binding = (ROOT / "mermaid_classifier_amd" / "_lib.py").read_text()
    listed = re.search(r"SYMBOLS = \[(.*?)\n\]", binding, re.S).group(1)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b(int|int64_t) {name}\(", header), name
        assert f'"{name}"' in listed, name
        assert f"lib.{name}.argtypes" in binding, name
    assert re.search(r"\bvoid mmc_targetset_destroy\(", header) and '"mmc_targetset_destroy"' in listed
    assert re.search(r"#define MMC_TARGETSET_MAX_CELLS 1073741824LL\b", header)
    assert "distillation" in header
    csrc = ROOT / "mermaid_classifier_amd" / "csrc"
    for unit, kernel in (("trainer.hip", "ce_grad_distill_kernel"), ("targets.hip", "target_rows_kernel")):
        assert re.search(rf"__global__ [^\n]*void {kernel}\(", (csrc / unit).read_text()), kernel
    assert re.search(r"\bvoid ce_grad_rows_distill\(", (csrc / "trainer.hip").read_text())       # its two instantiations' body
    build = (ROOT / "mermaid_classifier_amd" / "build.py").read_text()
    assert '"targets.hip": [' in build


# ---- argument checks on the Python side (none of these reaches the library) ---------------------------------------------------------
def _clf(**kw):
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    return TorchMLPClassifier(hidden_layer_sizes=(9,), **kw)


def test_constructor_ranges_params_and_config():
    from mermaid_classifier_amd.sweep import SweepConfig
    for bad in (dict(distill_alpha=-0.1), dict(distill_alpha=1.5), dict(distill_alpha=float("nan")), dict(distill_alpha=True),
                dict(distill_alpha="0.5"), dict(distill_temperature=0.2), dict(distill_temperature=65.0),
                dict(distill_temperature=float("nan")), dict(distill_temperature=None)):
        with pytest.raises(ValueError, match="distill_"):
            _clf(**bad)
    clf = _clf(distill_alpha=0.5, distill_temperature=2.0)
    params = clf.get_params()
    assert params["distill_alpha"] == 0.5 and params["distill_temperature"] == 2.0
    assert _clf().get_params()["distill_alpha"] == 0.0 and _clf().get_params()["distill_temperature"] == 1.0
    twin = _clf(**{k: v for k, v in params.items() if k != "hidden_layer_sizes"})
    assert twin.get_params() == params
    clf.set_params(distill_alpha=1.0, distill_temperature=4.0)
    assert (clf.distill_alpha, clf.distill_temperature) == (1.0, 4.0)
    made = SweepConfig(hidden_layer_sizes=(9,), distill_alpha=0.7, distill_temperature=3.0).classifier()
    assert (made.distill_alpha, made.distill_temperature) == (0.7, 3.0)
    assert SweepConfig().classifier().distill_alpha == 0.0
    kw_only = {f.name for f in dataclasses.fields(SweepConfig) if f.kw_only}
    assert {"distill_alpha", "distill_temperature"} <= kw_only                                 # keyword only: no positional slot
    import pickle
    back = pickle.loads(pickle.dumps(_clf(distill_alpha=0.25, distill_temperature=8.0)))          # unfitted: no device
    assert (back.distill_alpha, back.distill_temperature) == (0.25, 8.0)
    old = _clf()
    state = old.__getstate__()
    del state["distill_alpha"], state["distill_temperature"]                                   # a pickle from before the options
    old.__setstate__(state)
    assert (old.distill_alpha, old.distill_temperature) == (0.0, 1.0)


class _FakeSet:
    """What the Python-side checks read of a FeatureSet / TargetSet: length and classes."""

    def __init__(self, n, classes):
        self.n, self.classes = n, np.asarray(classes)

    def __len__(self):
        return self.n


def test_python_side_argument_errors(monkeypatch):
    import importlib
    import mermaid_classifier_amd as m
    from mermaid_classifier_amd import _lib, training
    D = importlib.import_module("mermaid_classifier_amd.distill")      # the package's attribute of that name is the function
    from mermaid_classifier_amd.sweep import _targets_per_classifier
    from mermaid_classifier_amd.torch_classifier import check_targets

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    assert {"TargetSet", "teacher_targets", "distill"} <= set(m.__all__)
    with pytest.raises(ValueError, match="classes is empty"):
        D.TargetSet([])
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="reserve_rows"):
            D.TargetSet([0, 1, 2], reserve_rows=bad)
    with pytest.raises(ValueError, match="at most"):
        D.TargetSet(np.arange(108), reserve_rows=(1 << 30) // 108 + 1)
    ts = D.TargetSet([2, 0, 1])
    assert ts.classes.tolist() == [0, 1, 2] and len(ts) == 0
    with pytest.raises(ValueError, match=r"must be \(n, 3\)"):
        ts.append(np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError, match="outside the set's 0 rows"):
        ts.read(0, 1)
    fs = _FakeSet(6, [0, 1, 2])
    good = D.TargetSet([0, 1, 2])
    monkeypatch.setattr(D.TargetSet, "__len__", lambda self: 6)
    assert check_targets(_clf(), fs, None) is None
    assert check_targets(_clf(distill_alpha=0.5), fs, good) is good
    with pytest.raises(ValueError, match="must be a TargetSet"):
        check_targets(_clf(distill_alpha=0.5), fs, np.zeros((6, 3)))
    with pytest.raises(ValueError, match="distill_alpha > 0"):
        check_targets(_clf(), fs, good)
    with pytest.raises(ValueError, match="mixup_alpha"):
        check_targets(_clf(distill_alpha=0.5, mixup_alpha=0.2), fs, good)
    with pytest.raises(ValueError, match="taxonomy"):
        check_targets(_clf(distill_alpha=0.5, class_levels={0: [0], 1: [0], 2: [1]}, level_weights=[1.0]), fs, good)
    with pytest.raises(ValueError, match="hold 6 rows, the feature set 5"):
        check_targets(_clf(distill_alpha=0.5), _FakeSet(5, [0, 1, 2]), good)
    with pytest.raises(ValueError, match="classes differ"):
        check_targets(_clf(distill_alpha=0.5), _FakeSet(6, [0, 1, 3]), good)
    with pytest.raises(ValueError, match="targets or teacher, not both"):
        training.resolve_targets(good, object(), fs)
    assert training.resolve_targets(good, None, fs) is good and training.resolve_targets(None, None, fs) is None
    with pytest.raises(ValueError, match="2 entries for 3 classifiers"):
        _targets_per_classifier([good, None], 3)
    assert _targets_per_classifier(good, 2) == [good, good] and _targets_per_classifier(None, 2) == [None, None]
    with pytest.raises(ValueError, match="must be a CalibratedMLP or a Predictor"):
        D.as_teacher(object())
    with pytest.raises(ValueError, match="fs must be a FeatureSet"):
        D.check_teacher(_FakeSet(6, [0, 1, 2]), object())
    for bad in (dict(alpha=0.0), dict(alpha=1.5), dict(alpha=0.5, temperature=0.1)):
        with pytest.raises(ValueError):
            D.distill(object(), None, None, None, 1, batch_size=10, **bad)
    with pytest.raises(ValueError, match="clf has distill_alpha"):
        D.distill(object(), None, None, None, 1, batch_size=10, alpha=0.5, clf=_clf(distill_alpha=0.25))


# ---- the stage's arithmetic against the bounds ------------------------------------------------------------------------------------
def _case(K, weighted, seed=7):
    rng = np.random.default_rng([K, int(weighted), seed])
    w = lc.class_weights(rng, K) if weighted else None
    prior = lc.dirichlet_prior(rng, K)
    z, y = lc.logit_rows(rng, 205, K, 4.0)
    q = dc.teacher_rows(rng, y, K)
    return rng, w, prior, z, y, q


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [3, 65, 108, 130])
def test_fp32_emulation_stays_within_the_bounds(K, weighted):
    rng, w, prior, z, y, q = _case(K, weighted)
    for name, kind in KINDS:
        alpha, tau, o = _opts(kind, prior)
        grad, rows, k = dc.checker(z, y, q, alpha, tau, w, **o)
        bd, bl = dc.bounds(z, y, q, alpha, tau, w, rows, k, prior=o.get("prior"))
        d, l = dc.emulate(z, y, q, alpha, tau, w, **o)
        assert np.isfinite(d).all() and np.isfinite(l).all()
        ed, el = _peak(d - grad, bd), _peak(l - rows, bl)
        print(f"K {K} weighted {weighted} {name:26s}: dlogits {ed:.3f} of its bound, row_loss {el:.3f} of its bound")
        assert ed <= 1.0 and el <= 1.0, (name, ed, el)
    r = rng.uniform(1e-2, 1e2, len(y)).astype(np.float32)
    r[[2, 5]] = 0.0
    exact = dc.normaliser(y, w, r, exact=True)
    grad, rows, k = dc.checker(z, y, q, 0.3, 2.0, w, norm=exact)
    bd, bl = dc.bounds(z, y, q, 0.3, 2.0, w, rows, k, norm=exact)
    d, l = dc.emulate(z, y, q, 0.3, 2.0, w, norm=dc.normaliser(y, w, r))
    assert (d[2] == 0).all() and l[5] == 0
    assert _peak(d - grad, bd) <= 1.0 and _peak(l - rows, bl) <= 1.0


@pytest.mark.parametrize("K", [3, 108])
def test_wrong_kernels_miss_the_bounds_by_orders_of_magnitude(K):
    rng, w, prior, z, y, q = _case(K, True)
    alpha, tau = 0.3, 2.0
    grad, rows, k = dc.checker(z, y, q, alpha, tau, w)
    bd, bl = dc.bounds(z, y, q, alpha, tau, w, rows, k)
    for wrong in dc.WRONG:
        d, l = dc.emulate(z, y, q, alpha, tau, w, wrong=wrong)
        ed, el = _peak(d - grad, bd), _peak(l - rows, bl)
        print(f"K {K} wrong kernel {wrong:24s}: dlogits {ed:.3g} x its bound, row_loss {el:.3g} x its bound")
        worst = max(ed, el)
        assert worst >= 100.0, (wrong, ed, el)
        if wrong == "tau_for_tau2":
            assert el >= 100.0 and ed <= 1.0        # the loss alone is scaled wrongly
        if wrong == "no_tau_in_gradient":
            assert ed >= 100.0 and el <= 1.0        # and here the gradient alone


def test_gibbs_cross_entropy_is_at_least_the_teachers_entropy():
    for K in (3, 65, 130):
        rng, w, prior, z, y, q = _case(K, False)
        for tau in (1.0, 2.0, 0.5):
            _, _, k = dc.checker(z, y, q, 1.0, tau)
            qt = dc.soften(q, tau)
            # at tau = 1 the stored row is used as it is, sum S: k = S (-sum (q / S) log p) >= S H(q / S)
            sums = qt.sum(axis=1)
            h = dc.entropy(qt / sums[:, None]) * sums
            assert np.all(k >= h - 1e-12), (K, tau, float((k - h).min()))


# ---- evidence -------------------------------------------------------------------------------------------------------------------
def test_distilling_the_five_seed_ensemble_of_the_float64_recipe():
    """The recipe of tests/test_ensemble_host.py's last test: five seeds of one 12 -> 24 -> 5 head trained by oracle/mlp_train_ref.py
    (20 passes over 600 rows of five Gaussian classes, 25 % of the training labels replaced at random), 1000 clean held-out rows.  One
    more 12 -> 24 -> 5 student (``distill_checker.StudentRef``, float64, its own seed, 20 passes) is trained three ways: on the noisy
    labels alone, on the five-seed mean at alpha = 1, tau = 1, and at alpha = 0.5, tau = 2.  Printed, in favour or not (the README entry
    quotes them): held-out accuracy and log-loss of each against the ensemble and the mean member.  Asserted: everything is finite, and
    Gibbs on the training rows (the cross-entropy of every student against the softened teacher is at least the teacher's entropy)."""
    from oracle.mlp_train_ref import MLPTrainRef
    rng = np.random.default_rng(2024)
    K, dim, n_train, n_test = 5, 12, 600, 1000
    centres = rng.normal(0, 1.0, (K, dim))

    def draw(n):
        y = rng.integers(0, K, n)
        return (centres[y] + rng.normal(0, 1.2, (n, dim))).astype(np.float32), y
    Xtr, ytr = draw(n_train)
    Xte, yte = draw(n_test)
    noisy = ytr.copy()
    flip = rng.random(n_train) < 0.25
    noisy[flip] = rng.integers(0, K, int(flip.sum()))
    dims = (dim, 24, K)

    def init(seed):
        r = np.random.default_rng(100 + seed)
        W = [r.uniform(-1, 1, (dims[i + 1], dims[i])).astype(np.float32) * np.float32(np.sqrt(6.0 / (dims[i] + dims[i + 1]))) for i in range(2)]
        return W, [np.zeros(dims[i + 1], np.float32) for i in range(2)]
    test_probs, train_probs = [], []
    for seed in range(5):
        net = MLPTrainRef(*init(seed), lr=3e-3)
        for epoch in range(20):
            net.partial_fit(Xtr, noisy, 100, random_state=seed * 1000 + epoch)
        test_probs.append(net.predict_proba(Xte))
        train_probs.append(net.predict_proba(Xtr))
    teacher_train = np.mean(train_probs, axis=0).astype(np.float32)          # what a target set would store
    assert dc.valid_rows(teacher_train).all()
    e = np.mean(test_probs, axis=0)
    rows = np.arange(n_test)

    def score(p):
        return float((p.argmax(1) == yte).mean()), float(-np.log(np.clip(p[rows, yte], 1e-15, 1)).mean())
    acc_e, nll_e = score(e)
    members = [score(p) for p in test_probs]
    acc_m, nll_m = float(np.mean([a for a, _ in members])), float(np.mean([b for _, b in members]))
    report = [f"ensemble accuracy {acc_e:.4f} log-loss {nll_e:.4f}", f"mean member accuracy {acc_m:.4f} log-loss {nll_m:.4f}"]
    X64 = Xtr.astype(np.float64)
    for name, alpha, tau in (("labels alone", 0.0, 1.0), ("alpha=1 tau=1", 1.0, 1.0), ("alpha=0.5 tau=2", 0.5, 2.0)):
        qt = dc.soften(teacher_train, tau)
        student = dc.StudentRef(*init(5), lr=3e-3, alpha=alpha, tau=tau)
        for epoch in range(20):
            student.partial_fit(X64, noisy, qt if alpha else None, 100, random_state=5000 + epoch)
        p = student.predict_proba(Xte.astype(np.float64))
        assert np.isfinite(p).all()
        acc, nll = score(p)
        report.append(f"student {name} accuracy {acc:.4f} log-loss {nll:.4f}")
        logpt = student._log_softmax(student.logits(X64) / tau)
        k = -np.where(qt > 0, qt * logpt, 0.0).sum(axis=1)
        sums = qt.sum(axis=1)
        h = dc.entropy(qt / sums[:, None]) * sums
        assert np.isfinite(k).all() and np.all(k >= h - 1e-12)
    print("distillation evidence: " + "; ".join(report))
