#!/usr/bin/env python3
"""GPU box: the per-epoch validation pass of the production head (1280 -> 500 -> 300 -> 100 -> 108) over a resident set of 200 000
rows, as mmc_trainer_evaluate_set_q32 (two totals) and as mmc_trainer_evaluate_classes_set (the totals and the 108 x 108 table).

Wall clock around calls that end in their stream synchronise; one warm-up per route, then the routes in turn, five times each;
median and spread (min .. max) per route.  The two routes' totals are compared, and the table's trace and row sums checked, before
anything is timed.

--plain-only: the plain leg alone.  It needs nothing this script's commit added to the library, so with --package-root pointing at a
checkout of an older commit (its sources and its built library) it gives that commit's figure.
--rows N: a smaller run."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--package-root", default=str(Path(__file__).resolve().parent.parent))
ap.add_argument("--rows", type=int, default=200000)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, args.package_root)
from mermaid_classifier_amd import FeatureSet, _lib  # noqa: E402
from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier  # noqa: E402

k, nf, n = 108, 1280, args.rows
rng = np.random.default_rng(0)
yi = rng.integers(0, k, size=n)
X = np.abs(rng.standard_normal((n, nf), dtype=np.float32) * np.float32(0.4) + np.float32(0.4))
fs = FeatureSet(nf, np.arange(k), reserve=n).append(X, yi)
del X
lib = _lib.lib()
clf = TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), learning_rate_init=1e-4, random_state=0)
clf.classes_, clf.n_features_in_, clf.n_iter_, clf.loss_curve_ = np.arange(k), nf, 0, []
clf._class_weight_vector = None
clf._create_trainer(*clf._initial_parameters())
table = np.zeros((k, k), np.int64)


def plain():
    nc, q = C.c_int64(0), C.c_int64(0)
    _lib.check(lib.mmc_trainer_evaluate_set_q32(clf._h, fs._handle(), 0, n, C.byref(nc), C.byref(q), None))
    return nc.value, q.value


def classes():
    nc, q = C.c_int64(0), C.c_int64(0)
    _lib.check(lib.mmc_trainer_evaluate_classes_set(clf._h, fs._handle(), 0, n, C.byref(nc), C.byref(q), table.ctypes.data, None))
    return nc.value, q.value


def stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


routes = [("mmc_trainer_evaluate_set_q32    ", plain)] if args.plain_only else [("mmc_trainer_evaluate_set_q32    ", plain),
                                                                               ("mmc_trainer_evaluate_classes_set", classes)]
print(f"{n} resident rows x {nf}, {k} classes, 1280 -> 500 -> 300 -> 100 -> {k}: {-(-n // 16384)} chunks of at most 16384 rows per call")
print(f"host clock around calls that end in a stream synchronise; one warm-up per route, then the routes in turn, {args.repeats} times "
      "each; median (min .. max) in ms")
first = [fn() for _, fn in routes]
if not args.plain_only:
    assert first[0] == first[1], first
    assert int(np.trace(table)) == first[1][0] and np.array_equal(table.sum(1), np.bincount(yi, minlength=k))
    print(f"totals equal: n_correct {first[0][0]}, sum_log_loss_q32 {first[0][1]}; trace and row sums of the table check")
times = {name: [] for name, _ in routes}
for _ in range(args.repeats):
    for name, fn in routes:
        t = time.perf_counter()
        fn()
        times[name].append((time.perf_counter() - t) * 1e3)
for name, _ in routes:
    med, lo, hi = stats(times[name])
    print(f"{name} {med:8.2f} ({lo:8.2f} .. {hi:8.2f})  {n / med * 1e3 / 1e6:6.2f} M rows/s", flush=True)
if not args.plain_only:
    (p_med, p_lo, p_hi), (c_med, c_lo, c_hi) = (stats(times[name]) for name, _ in routes)
    print(f"class-wise / plain = {c_med / p_med:.4f} (of the medians; {c_lo / p_hi:.4f} .. {c_hi / p_lo:.4f} over the spreads)")
