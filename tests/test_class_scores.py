"""``ClassScores`` against tests/golden/balancing_fixture.json -- the reference's ``compute_precision_recall_f1`` and
``compute_balanced_accuracy_mcc`` (sklearn underneath) on the pairs tests/golden/make_balancing_golden.py lists -- and the
``class_scores=True`` bookkeeping of ``sweep_loop`` / ``epoch_loop`` with stub device steps.  Supports compare with ``==``; scores
within relative 1e-12 (the means may be summed in another order: a bound on rounding, not a measured tolerance).  Host only."""

import json

import numpy as np
import pytest

from conftest import GOLDEN

REL = 1e-12


@pytest.fixture(scope="module")
def fx():
    return json.loads((GOLDEN / "balancing_fixture.json").read_text())


def _confusion(K, gt, est):
    c = np.zeros((K, K), np.int64)
    np.add.at(c, (np.asarray(gt), np.asarray(est)), 1)
    return c


def _close(got, want):
    return abs(got - want) <= REL * abs(want)


def test_class_scores_match_the_reference(fx):
    from mermaid_classifier_amd import ClassScores
    assert len(fx["scores"]) >= 3
    for case in fx["scores"]:
        K = case["n_classes"]
        cs = ClassScores(_confusion(K, case["gt"], case["est"]), [f"c{i}" for i in range(K)])
        per = cs.per_class()
        assert per["support"].dtype == np.int64 and per["support"].tolist() == case["support"], case["name"]
        for name in ("precision", "recall", "f1"):
            assert per[name].dtype == np.float64 and per[name].shape == (K,)
            for k in range(K):
                assert _close(per[name][k], case[name][k]), (case["name"], name, k, per[name][k], case[name][k])
        for name in ("precision_macro", "recall_macro", "f1_macro", "balanced_accuracy", "mcc", "accuracy"):
            assert _close(getattr(cs, name), case[name]), (case["name"], name, getattr(cs, name), case[name])
        assert cs.scalars() == {k: getattr(cs, k) for k in ("precision_macro", "recall_macro", "f1_macro", "balanced_accuracy", "mcc",
                                                            "accuracy")}
        assert cs.n == len(case["gt"])


def test_the_fixture_holds_the_cases_that_separate_the_conventions(fx):
    """The six-class pair has a class only in est (3), one only in gt (4) and one in neither (5); there the macro averages run
    over five classes, balanced accuracy over four, and f1_macro is not the mean of the per-class f1."""
    from mermaid_classifier_amd import ClassScores
    case = next(c for c in fx["scores"] if c["name"] == "six classes, partial presence")
    gt, est = set(case["gt"]), set(case["est"])
    assert 3 in est - gt and 4 in gt - est and 5 not in gt | est
    cs = ClassScores(_confusion(6, case["gt"], case["est"]), list(range(6)))
    per = cs.per_class()
    assert per["precision"][3] == 0 and per["recall"][3] == 0 and per["f1"][3] == 0 and per["support"][3] == 0
    assert per["recall"][4] == 0 and per["precision"][4] == 0 and per["support"][4] > 0
    assert _close(cs.recall_macro, per["recall"][:5].sum() / 5) and _close(cs.balanced_accuracy, per["recall"][[0, 1, 2, 4]].sum() / 4)
    assert abs(cs.f1_macro - per["f1"][:5].mean()) > 1e-4
    one = next(c for c in fx["scores"] if c["name"] == "one class, all correct")
    assert one["mcc"] == 0.0 and ClassScores(_confusion(3, one["gt"], one["est"]), "abc").mcc == 0.0
    allc = next(c for c in fx["scores"] if c["name"] == "all correct")
    assert allc["mcc"] == 1.0 and allc["balanced_accuracy"] == 1.0 and allc["f1_macro"] == 1.0


def test_class_scores_arguments_and_validation_hook():
    from mermaid_classifier_amd import ClassScores, Validation
    with pytest.raises(ValueError, match="shape"):
        ClassScores(np.zeros((2, 3), np.int64), ["a", "b"])
    with pytest.raises(ValueError, match="integers"):
        ClassScores(np.zeros((2, 2)), ["a", "b"])
    with pytest.raises(ValueError, match="negative"):
        ClassScores(np.array([[1, -1], [0, 0]]), ["a", "b"])
    empty = ClassScores(np.zeros((3, 3), np.int64), "abc")
    assert empty.mcc == 0.0 and empty.f1_macro == 0.0 and np.isnan(empty.accuracy) and np.isnan(empty.balanced_accuracy)
    conf = np.array([[5, 1, 0], [2, 3, 0], [0, 0, 0]], np.int64)
    v = Validation(["a", "b", "c"], None, None, None, None, None, conf, np.array([8, 3, 0]), 11, 8, 0, 0, 0)
    cs = v.class_scores()
    assert isinstance(cs, ClassScores) and np.array_equal(cs.confusion, conf) and cs.classes == ["a", "b", "c"]
    assert cs.accuracy == 8 / 11 and cs.balanced_accuracy == (5 / 6 + 3 / 5) / 2


class _Fake:
    def __init__(self, name):
        self.name, self.count, self.loss_curve_ = name, 0, []


class _Scores:
    def __init__(self, ba, f1):
        self.balanced_accuracy, self.f1_macro = ba, f1


_SCRIPT = {"early": [.90, .80, .85, .80, .70, .10], "late": [.9, .8, .7, .6, .5, .4]}


def _steps(class_scores):
    evals = {name: 0 for name in _SCRIPT}

    def fit_group(models, rows):
        for m in models:
            m.count += 1
            m.loss_curve_.append(10.0 - m.count)

    def eval_val(m):
        evals[m.name] += 1
        pair = (0.5 + 0.01 * m.count, _SCRIPT[m.name][evals[m.name] - 1])
        return pair + (_Scores(0.3 + 0.02 * m.count, 0.2 + 0.03 * m.count),) if class_scores else pair

    return fit_group, (lambda m: 0.25 * m.count), eval_val


def _strip(ms, drop=()):
    return [{k: v for k, v in m.items() if k not in ("cumulative_seconds",) + tuple(drop)} for m in ms]


def test_sweep_loop_class_scores_adds_two_keys_and_changes_nothing_else():
    from mermaid_classifier_amd.sweep import sweep_loop
    runs = {}
    for flag in (False, True):
        fit_group, eval_ref, eval_val = _steps(flag)
        seen = []
        got = sweep_loop([_Fake(n) for n in _SCRIPT], [lambda e: [0, 1]] * 2, fit_group, eval_ref, eval_val, 6, early_stopping_patience=2,
                         on_epoch_end=seen.append, class_scores=flag)
        runs[flag] = (seen, [(clf.name, clf.count, info) for clf, info in got])
    plain, scored = runs[False][0], runs[True][0]
    assert len(plain) == len(scored) == 4 + 6 and runs[False][1] == runs[True][1]          # "early" stops after 4 epochs
    extra = ("val_balanced_accuracy", "val_f1_macro")
    assert all(not set(extra) & set(m) for m in plain)
    assert all(set(m) - set(p) == set(extra) for m, p in zip(scored, plain))
    assert _strip(scored, extra) == _strip(plain)
    for m in scored:
        passes = 2 * (m["epoch"] + 1)
        assert m["val_balanced_accuracy"] == 0.3 + 0.02 * passes and m["val_f1_macro"] == 0.2 + 0.03 * passes


def test_epoch_loop_class_scores_and_the_early_stopping_keyword():
    from mermaid_classifier_amd.training import EarlyStopping, epoch_loop
    runs = {}
    for flag in (False, True):
        fit_group, eval_ref, eval_val = _steps(flag)
        seen = []
        clf, info = epoch_loop(_Fake("early"), lambda c, e: fit_group([c], [None]), eval_ref, eval_val, 6, early_stopping_patience=2,
                               on_epoch_end=seen.append, class_scores=flag)
        runs[flag] = (seen, clf.count, info)
    assert runs[False][1:] == runs[True][1:] and runs[True][2]["final_epoch"] == 4
    assert _strip(runs[True][0], ("val_balanced_accuracy", "val_f1_macro")) == _strip(runs[False][0])
    assert all("val_f1_macro" in m for m in runs[True][0])
    state = EarlyStopping(3, None)
    base = state.epoch_done(_Fake("a"), 0, 0.1, 0.2, 0.3)                                   # the positional signature stays
    more = EarlyStopping(3, None).epoch_done(_Fake("a"), 0, 0.1, 0.2, 0.3, extra={"val_f1_macro": 0.5})
    assert set(more) - set(base) == {"val_f1_macro"} and more["val_f1_macro"] == 0.5
