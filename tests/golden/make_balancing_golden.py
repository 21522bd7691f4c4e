"""Generate tests/golden/balancing_fixture.json: the reference's own ``compute_class_weights`` (training/sample_weighting/
effective_number.py), ``compute_per_class_targets`` (training/subsample/registry.py) and the two confusion-matrix groups
``compute_precision_recall_f1`` / ``compute_balanced_accuracy_mcc`` (pyspacer/metrics/classification.py) on small cases.

    python tests/golden/make_balancing_golden.py /path/to/mermaid-classifier     (needs pandas, scikit-learn, scipy, matplotlib)

The metrics package imports ``spacer.data_classes``, ``mlflow`` and ``duckdb`` at module level; none is used by the two groups, so
stand-in modules go into ``sys.modules`` first, as in make_metrics_golden.py.  The file holds data only: the inputs and what the
reference returned (floats as JSON numbers: ``repr`` round-trips a float64).

Cases
  weights: one class; counts 0 and 1; a 10^4 : 1 imbalance with cap None, 5 and 5000; an empty input.
  targets: {5, 25, 1} with total 10 (stratified, floor 1; balanced, floor 2); proportional shares of exactly x.5 (half to even, both
           ways); an overshoot the floor keeps from being trimmed (fully, and in part); equal counts, so the trim order falls to the
           key; counts that are all zero.  ``SubsampleOptions`` itself rejects a total_annotations of 0: recorded under "rejected".
  scores:  6 classes with class 3 only in est, class 4 only in gt and class 5 in neither; an all-correct pair; one-class pairs (the
           MCC denominator is 0)."""

import dataclasses
import json
import sys
import types
import warnings
from pathlib import Path

import numpy as np


class _Dummy(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


@dataclasses.dataclass
class ValResults:
    scores: list
    gt: list
    est: list
    classes: list


class _Library:
    def bagf_id_to_name(self, bagf_id, gf_library):
        return "name of " + bagf_id


def _stand_ins():
    for name in ("mlflow", "duckdb", "spacer", "spacer.data_classes"):
        sys.modules.setdefault(name, _Dummy(name))
    sys.modules["spacer.data_classes"].ValResults = ValResults


WEIGHT_CASES = [
    ("single class", {"a": 500}, None),
    ("counts 0 and 1", {"a": 0, "b": 1}, None),
    ("counts 0 and 1, cap 1", {"a": 0, "b": 1, "c": 40}, 1.0),
    ("imbalance, no cap", {"big": 200000, "mid": 3000, "rare": 20}, None),
    ("imbalance, cap 5", {"big": 200000, "mid": 3000, "rare": 20}, 5.0),
    ("imbalance, cap 5000", {"big": 200000, "mid": 3000, "rare": 20}, 5000.0),
    ("one class with a cap", {"a": 7}, 5.0),
    ("empty", {}, None),
]

TARGET_CASES = [
    ("5-25-1 stratified floor 1", {"a": 5, "b": 25, "c": 1}, "stratified", 10, 1),
    ("5-25-1 balanced floor 2", {"a": 5, "b": 25, "c": 1}, "balanced", 10, 2),
    ("half to even 0.5 / 1.5", {"a": 1, "b": 3}, "stratified", 2, 0),
    ("half to even 2.5 / 7.5", {"a": 5, "b": 15}, "stratified", 10, 0),
    ("half to even 1.5 / 2.5", {"a": 3, "b": 5}, "stratified", 4, 0),
    ("floor blocks the whole trim", {"a": 2, "b": 2, "c": 9}, "stratified", 3, 2),
    ("floor blocks part of the trim", {"a": 1, "b": 1, "c": 1, "d": 10}, "stratified", 3, 1),
    ("equal counts: trim by key", {"b": 4, "a": 4, "c": 4}, "stratified", 5, 0),
    ("equal counts: trim two by key", {"z": 6, "m": 6, "k": 6, "y": 6}, "stratified", 6, 1),
    ("all counts zero, stratified", {"a": 0, "b": 0}, "stratified", 5, 0),
    ("all counts zero, balanced", {"a": 0, "b": 0}, "balanced", 5, 0),
    ("balanced caps the large class", {"a": 100, "b": 3, "c": 40}, "balanced", 90, 0),
    ("undershoot is accepted", {"a": 1, "b": 1, "c": 1, "d": 1, "e": 1, "f": 1, "g": 1}, "stratified", 3, 0),
    ("empty", {}, "balanced", 4, 0),
]


def score_inputs():
    rng = np.random.default_rng(20250519)
    gt = rng.choice([0, 1, 2, 4], 240, p=[0.55, 0.25, 0.15, 0.05])
    est = np.where(rng.random(240) < 0.65, gt, rng.choice([0, 1, 2, 3], 240))
    est = np.where(est == 4, 3, est)            # class 4 is never predicted, class 3 never true, class 5 in neither
    assert set(gt.tolist()) == {0, 1, 2, 4} and set(est.tolist()) == {0, 1, 2, 3}
    g2 = rng.integers(0, 4, 50)
    return [("six classes, partial presence", 6, gt.tolist(), est.tolist()),
            ("all correct", 4, g2.tolist(), g2.tolist()),
            ("one class, all correct", 3, [2] * 7, [2] * 7),
            ("one true class, two predicted", 3, [1] * 6, [1, 1, 0, 1, 0, 1]),
            ("two true classes, one predicted", 3, [0, 0, 1, 2, 2, 2], [2] * 6)]


def main(reference_root):
    _stand_ins()
    sys.path.insert(0, str(reference_root))
    import matplotlib
    matplotlib.use("Agg")
    from sklearn.metrics import accuracy_score

    from mermaid_classifier.pyspacer.metrics._context import MetricsContext
    from mermaid_classifier.pyspacer.metrics.classification import compute_balanced_accuracy_mcc, compute_precision_recall_f1
    from mermaid_classifier.training.sample_weighting.effective_number import BETA, compute_class_weights
    from mermaid_classifier.training.sample_weighting.options import SampleWeightingOptions
    from mermaid_classifier.training.subsample.options import SubsampleOptions
    from mermaid_classifier.training.subsample.registry import compute_per_class_targets

    out = {"beta": BETA, "weights": [], "targets": [], "rejected": [], "scores": []}
    for name, counts, cap in WEIGHT_CASES:
        got = compute_class_weights(dict(counts), SampleWeightingOptions(enabled=True, weight_ratio_cap=cap))
        out["weights"].append({"name": name, "counts": counts, "weight_ratio_cap": cap, "weights": got})
    assert compute_class_weights({"a": 3}, SampleWeightingOptions(enabled=False)) == {}

    for name, counts, strategy, total, floor in TARGET_CASES:
        got = compute_per_class_targets(SubsampleOptions(strategy=strategy, total_annotations=total, min_per_class=floor), dict(counts))
        assert all(isinstance(v, int) for v in got.values())
        out["targets"].append({"name": name, "counts": counts, "strategy": strategy, "total_annotations": total,
                               "min_per_class": floor, "targets": got})
    by_name = {c["name"]: c["targets"] for c in out["targets"]}
    assert by_name["5-25-1 stratified floor 1"] == {"a": 2, "b": 7, "c": 1}
    assert by_name["5-25-1 balanced floor 2"] == {"a": 3, "b": 3, "c": 2}
    for kwargs in ({"strategy": "stratified", "total_annotations": 0}, {"strategy": "balanced", "total_annotations": None},
                   {"strategy": "inverse", "total_annotations": 5}, {"strategy": "balanced", "total_annotations": 5, "min_per_class": -1}):
        try:
            SubsampleOptions(**kwargs)
        except ValueError:
            out["rejected"].append(kwargs)
        else:
            raise AssertionError(f"the reference accepts {kwargs}")

    for name, K, gt, est in score_inputs():
        classes = [f"c{i}::g" for i in range(K)]
        ctx = MetricsContext(val_results=ValResults(scores=[1.0] * len(gt), gt=gt, est=est, classes=classes), ba_library=_Library(),
                             gf_library=None, format_func=float, dataset=None, ba_paths={})
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            prf = compute_precision_recall_f1(ctx)
            bam = compute_balanced_accuracy_mcc(ctx)
            acc = float(accuracy_score(gt, est))
        df = prf.dataframes[0].df
        assert df["bagf_id"].tolist() == classes
        case = {"name": name, "n_classes": K, "gt": gt, "est": est, "accuracy": acc,
                "precision": [float(v) for v in df["precision"]], "recall": [float(v) for v in df["recall"]],
                "f1": [float(v) for v in df["f1_score"]], "support": [int(v) for v in df["n_samples"]]}
        for s in list(prf.scalars) + list(bam.scalars):
            case[s.name] = float(s.value)
        out["scores"].append(case)

    path = Path(__file__).resolve().parent / "balancing_fixture.json"
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main(Path(sys.argv[1]))
