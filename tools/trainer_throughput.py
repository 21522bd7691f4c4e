#!/usr/bin/env python3
"""GPU box: samples/s of TorchMLPClassifier.partial_fit on the MI355X (production shape 1280 -> 500 -> 300 -> 100 -> 108,
mini-batches of 200 = the reference's "auto") next to the numpy oracle of the same arithmetic on the host cores.

--resident: instead, one 20 000-row training pass and one evaluate of the same rows at the production shape, each host-fed
(partial_fit / evaluate on host arrays) and from a device-resident FeatureSet (partial_fit_rows / evaluate on the set)."""
import sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
from oracle.mlp_train_ref import MLPTrainRef
rng = np.random.default_rng(0)
k, nf, n = 108, 1280, 20000
yi = rng.integers(0, k, size=n)
X = np.abs(rng.normal(0.4, 0.4, size=(n, nf))).astype(np.float32)
clf = TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), learning_rate_init=1e-4, random_state=0)
clf.partial_fit(X, yi, classes=list(range(k)))


if "--resident" in sys.argv:
    from mermaid_classifier_amd import FeatureSet, evaluate
    t = time.perf_counter()
    fs = FeatureSet(nf, np.arange(k), reserve=n).append(X, yi)
    print(f"FeatureSet fill: {n} x {nf} fp32 ({X.nbytes/1e6:.0f} MB) uploaded once in {(time.perf_counter() - t)*1e3:.1f} ms")
    clf.partial_fit_rows(fs)          # warm-up: staging buffers
    evaluate(clf, fs)
    evaluate(clf, (X, yi))
    rows = [("training pass, host-fed   (partial_fit)", lambda: clf.partial_fit(X, yi)),
            ("training pass, resident   (partial_fit_rows)", lambda: clf.partial_fit_rows(fs)),
            ("evaluate, host-fed        (evaluate(clf, (X, y)))", lambda: evaluate(clf, (X, yi))),
            ("evaluate, resident        (evaluate(clf, fs))", lambda: evaluate(clf, fs))]
    reps = 7
    print(f"{n} rows, 1280 -> 500 -> 300 -> 100 -> {k}, mini-batches of 200 ({n//200} Adam steps per pass); wall clock around calls that end in a "
          f"stream synchronise, the four variants taken in turn {reps} times: best / median")
    times = {name: [] for name, _ in rows}
    for _ in range(reps):
        for name, fn in rows:
            t = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t) * 1e3)
    for name, _ in rows:
        lo, med = min(times[name]), sorted(times[name])[reps // 2]
        print(f"  {name:<52s} {lo:8.2f} ms / {med:8.2f} ms   {n/lo*1e3:10.0f} rows/s")
    assert evaluate(clf, fs) == evaluate(clf, (X, yi))
    sys.exit(0)
t0 = time.perf_counter()
for _ in range(3):
    clf.partial_fit(X, yi)
dt = (time.perf_counter() - t0) / 3
print(f"HIP partial_fit: {n/dt:.0f} samples/s ({dt*1e3:.1f} ms per pass of {n}, {n//200} Adam steps, incl. host shuffle + H2D of {X.nbytes/1e6:.0f} MB)")
clf2 = TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), random_state=0)
clf2.classes_, clf2.n_features_in_ = np.arange(k), nf
ref = MLPTrainRef(*clf2._initial_parameters(), lr=1e-4)
t0 = time.perf_counter()
ref.partial_fit(X[:4000], yi[:4000], "auto")
dt2 = time.perf_counter() - t0
print(f"numpy oracle on the host: {4000/dt2:.0f} samples/s")
