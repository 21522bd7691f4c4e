#!/usr/bin/env python3
"""GPU box: what dropout and mixup cost in a training pass (profiles/regularizers.txt).

One pass of the production head (1280 -> 500 -> 300 -> 100 -> 108, mini-batches of 200) over a resident set of 200 000 rows, as
mmc_trainer_partial_fit_set(_mixed) calls: plain, dropout 0.2, dropout 0.2 + input dropout 0.1, and those two + mixup (alpha 0.2; the
plan is made once, outside the clock).  Then the eight-head sweep of tools/sweep_throughput.py as one grouped call, plain and with
every member dropping.

Wall clock around calls that end in their stream synchronise; every variant is warmed up once, then the variants are taken in turn,
five times each; median and spread (min .. max) per variant.

--plain-only: the plain solo leg alone.  It needs nothing this script's commit added to the library or the package, so it runs on a
checkout of the parent commit too: that is how the plain pass is compared with the earlier code's, alternating the two processes.
--rows N / --repeats R: smaller runs."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from mermaid_classifier_amd import FeatureSet, _lib  # noqa: E402
from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--rows", type=int, default=200000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--sweep", type=int, default=8)
args = ap.parse_args()
k, nf, n, mb = 108, 1280, args.rows, 200

rng = np.random.default_rng(0)
yi = rng.integers(0, k, size=n)
X = np.abs(rng.standard_normal((n, nf), dtype=np.float32) * np.float32(0.4) + np.float32(0.4))
fs = FeatureSet(nf, np.arange(k), reserve=n).append(X, yi)
del X
lib = _lib.lib()


def member(seed, **kw):
    clf = TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), learning_rate_init=1e-4, random_state=seed, **kw)
    clf.classes_, clf.n_features_in_, clf.n_iter_, clf.loss_curve_ = np.arange(k), nf, 0, []
    clf._class_weight_vector = None
    clf._create_trainer(*clf._initial_parameters())
    return clf, np.ascontiguousarray(np.random.default_rng(seed).permutation(n).astype(np.int64))


def solo_pass(clf, visit, plan=None):
    avg = C.c_double(0.0)
    if plan is None:
        _lib.check(lib.mmc_trainer_partial_fit_set(clf._h, fs._handle(), visit.ctypes.data, n, mb, C.byref(avg), None))
    else:
        _lib.check(lib.mmc_trainer_partial_fit_set_mixed(clf._h, fs._handle(), visit.ctypes.data, plan[0].ctypes.data, plan[1].ctypes.data,
                                                         n, mb, C.byref(avg), None))
    return avg.value


def group_pass(members):
    count = len(members)
    handles = (C.c_void_p * count)(*[clf._h.value for clf, _ in members])
    visits = (C.c_void_p * count)(*[v.ctypes.data for _, v in members])
    avg = (C.c_double * count)()
    _lib.check(lib.mmc_trainer_group_partial_fit_set(handles, count, fs._handle(), visits, (C.c_int64 * count)(*[n] * count),
                                                     (C.c_int * count)(*[mb] * count), avg, None))
    return list(avg)


def measure(routes):
    """routes: [(name, callable)] -> {name: (median, min, max) in ms}; one warm-up each, then in turn."""
    for _, fn in routes:
        fn()
    times = {name: [] for name, _ in routes}
    for _ in range(args.repeats):
        for name, fn in routes:
            t = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t) * 1e3)
    return {name: (sorted(ms)[len(ms) // 2], min(ms), max(ms)) for name, ms in times.items()}


steps = -(-n // mb)
print(f"{n} resident rows x {nf}, {k} classes, 1280 -> 500 -> 300 -> 100 -> {k}, mini-batches of {mb}: {steps} Adam steps per model and pass")
print(f"host clock around calls that end in a stream synchronise; one warm-up per variant, then the variants in turn, {args.repeats} times "
      "each; median (min .. max) in ms")
if args.plain_only:
    clf, visit = member(0)
    med, lo, hi = measure([("plain", lambda: solo_pass(clf, visit))])["plain"]
    print(f"solo  plain                                  {med:9.1f} ({lo:9.1f} .. {hi:9.1f})")
    sys.exit(0)

from mermaid_classifier_amd.sampling import mixup_plan  # noqa: E402

variants = [("plain", {}, False), ("dropout 0.2", dict(dropout=0.2), False),
            ("dropout 0.2 + input dropout 0.1", dict(dropout=0.2, input_dropout=0.1), False),
            ("dropout 0.2 + input dropout 0.1 + mixup", dict(dropout=0.2, input_dropout=0.1), True),
            ("mixup alone", {}, True)]
routes = []
for name, kw, mixed in variants:
    clf, visit = member(0, **kw)
    plan = mixup_plan(visit, mb, 0.2, np.random.default_rng(1)) if mixed else None
    routes.append((name, lambda clf=clf, visit=visit, plan=plan: solo_pass(clf, visit, plan)))
got = measure(routes)
base = got["plain"][0]
for name, _, _ in variants:
    med, lo, hi = got[name]
    print(f"solo  {name:40s} {med:9.1f} ({lo:9.1f} .. {hi:9.1f})   {med / base:6.3f} x plain")

S = args.sweep
plain = [member(m) for m in range(S)]
drop = [member(m, dropout=0.2) for m in range(S)]
got = measure([("plain", lambda: group_pass(plain)), ("dropout 0.2", lambda: group_pass(drop))])
base = got["plain"][0]
for name in ("plain", "dropout 0.2"):
    med, lo, hi = got[name]
    print(f"group of {S}, every member {name:20s}   {med:9.1f} ({lo:9.1f} .. {hi:9.1f})   {S * steps / med * 1e3:8.0f} model-steps/s   "
          f"{med / base:6.3f} x plain")
