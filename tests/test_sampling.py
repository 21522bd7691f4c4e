"""``sampling.py`` -- effective-number class weights, per-class subsample targets, the rows of a subsample and its batch hook --
against tests/golden/balancing_fixture.json: the reference's ``compute_class_weights`` and ``compute_per_class_targets`` on the
cases tests/golden/make_balancing_golden.py lists.  Targets compare with ``==``; weights within relative 1e-12, a bound on the
rounding of ``beta**n`` between libm builds, not a measured tolerance.  Host only."""

import json

import numpy as np
import pytest

from conftest import GOLDEN

REL = 1e-12


@pytest.fixture(scope="module")
def fx():
    return json.loads((GOLDEN / "balancing_fixture.json").read_text())


def test_effective_number_weights_match_the_reference(fx):
    from mermaid_classifier_amd.sampling import effective_number_weights
    names = [c["name"] for c in fx["weights"]]
    assert {"single class", "counts 0 and 1", "imbalance, no cap", "imbalance, cap 5", "imbalance, cap 5000", "empty"} <= set(names)
    assert fx["beta"] == 0.9999
    for case in fx["weights"]:
        got = effective_number_weights(case["counts"], weight_ratio_cap=case["weight_ratio_cap"])
        want = case["weights"]
        assert list(got) == list(want), case["name"]                    # same keys, in the input's order
        for k in want:
            assert abs(got[k] - want[k]) <= REL * abs(want[k]), (case["name"], k, got[k], want[k])
        assert all(w > 0 for w in got.values())
    by = {c["name"]: c["weights"] for c in fx["weights"]}
    # the fixture does what its names say: cap 5 lowers the rare class to 5 x the smallest weight and leaves "mid" (3.9 x) alone,
    # cap 5000 lowers nothing
    assert by["imbalance, cap 5"]["rare"] == by["imbalance, no cap"]["big"] * 5.0
    assert by["imbalance, cap 5"]["mid"] == by["imbalance, no cap"]["mid"] < by["imbalance, cap 5"]["rare"]
    assert by["imbalance, cap 5000"] == by["imbalance, no cap"]
    assert by["imbalance, no cap"]["rare"] / by["imbalance, no cap"]["big"] > 400
    assert by["counts 0 and 1"]["a"] == by["counts 0 and 1"]["b"]       # n = max(count, 1)
    assert by["empty"] == {}


def test_effective_number_weights_arguments():
    from mermaid_classifier_amd.sampling import effective_number_weights
    assert effective_number_weights({}) == {}
    flat = effective_number_weights({"a": 10, "b": 1000}, beta=0.0)
    assert flat == {"a": 1.0, "b": 1.0}                                 # beta = 0: uniform
    with pytest.raises(ValueError, match="weight_ratio_cap"):
        effective_number_weights({"a": 1}, weight_ratio_cap=0.5)
    with pytest.raises(ValueError, match="beta"):
        effective_number_weights({"a": 1}, beta=1.0)


def test_subsample_targets_match_the_reference(fx):
    from mermaid_classifier_amd.sampling import subsample_targets
    for case in fx["targets"]:
        got = subsample_targets(case["counts"], case["strategy"], case["total_annotations"], case["min_per_class"])
        assert got == case["targets"], case["name"]
        assert all(type(v) is int for v in got.values())
        assert list(got) == list(case["counts"])
    by = {c["name"]: c["targets"] for c in fx["targets"]}
    assert by["5-25-1 stratified floor 1"] == {"a": 2, "b": 7, "c": 1}
    assert by["5-25-1 balanced floor 2"] == {"a": 3, "b": 3, "c": 2}
    assert by["half to even 2.5 / 7.5"] == {"a": 2, "b": 8} and by["half to even 0.5 / 1.5"] == {"a": 0, "b": 2}
    assert sum(by["floor blocks the whole trim"].values()) > 3          # the overshoot stays
    assert by["equal counts: trim by key"] == {"b": 2, "a": 1, "c": 2}  # "a" sorts first and absorbs the trim
    assert by["all counts zero, stratified"] == {"a": 0, "b": 0}


def test_subsample_targets_rejects_what_the_reference_rejects(fx):
    from mermaid_classifier_amd.sampling import subsample_targets
    assert len(fx["rejected"]) == 4
    for kwargs in fx["rejected"]:
        with pytest.raises(ValueError):
            subsample_targets({"a": 3, "b": 4}, kwargs["strategy"], kwargs["total_annotations"], kwargs.get("min_per_class", 0))
    with pytest.raises(ValueError, match="strategy"):
        subsample_targets({}, "sqrt", 5)


def _rows_by_loop(labels, targets, order):
    """dataset.py:292-310 as a plain loop: walk the rows in primary-key order, number them within their class, keep _rn <= target."""
    seen, keep = {}, []
    for row in (range(len(labels)) if order is None else order):
        k = int(labels[row])
        seen[k] = seen.get(k, 0) + 1
        if seen[k] <= targets.get(k, 0):
            keep.append(int(row))
    return sorted(keep)


def test_subsample_rows_equals_the_plain_loop():
    from mermaid_classifier_amd.sampling import class_counts, subsample_rows, subsample_targets
    rng = np.random.default_rng(5)
    labels = rng.choice(6, 400, p=[0.5, 0.2, 0.15, 0.1, 0.05, 0.0])      # class 5 is empty
    counts = class_counts(labels, 6)
    assert counts.dtype == np.int64 and counts.tolist() == np.bincount(labels, minlength=6).tolist() and counts[5] == 0
    perm = rng.permutation(400)
    for targets in ({0: 30, 1: 30, 2: 30, 3: 30, 4: int(counts[4])},     # class 5 has no target: dropped
                    {0: 0, 1: int(counts[1]), 5: 0},                      # a zero target, a whole class, an empty class
                    {k: int(v) for k, v in subsample_targets(dict(enumerate(counts.tolist())), "balanced", 120).items()},
                    {k: int(v) for k, v in subsample_targets(dict(enumerate(counts.tolist())), "stratified", 97).items()}):
        for order in (None, perm):
            got = subsample_rows(labels, targets, order)
            assert got.dtype == np.int64 and got.tolist() == _rows_by_loop(labels, targets, None if order is None else order.tolist())
            kept = np.bincount(labels[got], minlength=6)
            assert all(kept[k] == targets.get(k, 0) for k in range(6))
    assert subsample_rows(labels, {0: 30}, perm).tolist() != subsample_rows(labels, {0: 30}).tolist()   # the order matters
    with pytest.raises(ValueError, match="no oversampling"):
        subsample_rows(labels, {4: int(counts[4]) + 1})
    with pytest.raises(ValueError, match="no oversampling"):
        subsample_rows(labels, {5: 1})
    with pytest.raises(ValueError, match="permutation"):
        subsample_rows(labels, {0: 1}, order=np.zeros(400, np.int64))
    with pytest.raises(ValueError, match="permutation"):
        subsample_rows(labels, {0: 1}, order=np.arange(399))
    assert subsample_rows(np.zeros(0, np.int64), {}).tolist() == []
    with pytest.raises(ValueError, match="outside"):
        class_counts(np.array([0, 6]), 6)
    with pytest.raises(ValueError, match="n_classes"):
        class_counts(labels)


def test_row_batches_yields_contiguous_slices_every_epoch():
    from mermaid_classifier_amd.sampling import row_batches
    rows = np.array([3, 4, 9, 11, 20, 21, 22], np.int64)
    hook = row_batches(rows, 3)
    for epoch in (0, 1, 7):
        got = list(hook(epoch))
        assert [b.tolist() for b in got] == [[3, 4, 9], [11, 20, 21], [22]] and all(b.dtype == np.int64 for b in got)
    assert [b.tolist() for b in row_batches(rows, 7)(0)] == [rows.tolist()]
    assert list(row_batches([], 4)(0)) == []
    with pytest.raises(ValueError, match="batch_size"):
        row_batches(rows, 0)


def test_package_exports():
    import mermaid_classifier_amd as pkg
    for name in ("class_counts", "effective_number_weights", "subsample_targets", "subsample_rows", "row_batches", "rank_sweep",
                 "evaluate_classes", "ClassScores"):
        assert getattr(pkg, name) is not None and name in pkg.__all__
