#!/usr/bin/env python3
"""GPU box: what batch normalisation costs in a training pass (profiles/batch_norm.txt).

One pass of the production head (1280 -> 500 -> 300 -> 100 -> 108, mini-batches of 200) over a resident set of 200 000 rows: plain,
then with mmc_trainer_set_batch_norm on the trainer (per step: three bn_forward_kernel and three bn_backward_kernel launches and one
more adam_kernel launch; three colsum launches fewer).  Then the same two as one grouped call of eight heads in which every member
carries the option, and a mixed group of four plain and four normalised heads.  Last, the eval-mode forward of 16 384 rows on a
trainer whose fold is stale (the first call after a step launches bn_fold_kernel) and on one whose fold is current.

Wall clock around calls that end in their stream synchronise; every variant is warmed up once, then the variants are taken in turn,
five times each; median and spread (min .. max) per variant.  The plain pass against the parent commit is
tools/regularizer_cost.py --plain-only, which runs on either checkout.

--rows N / --repeats R / --sweep S: smaller runs."""
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
ap.add_argument("--rows", type=int, default=200000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--sweep", type=int, default=8)
args = ap.parse_args()
k, nf, n, mb = 108, 1280, args.rows, 200
steps = -(-n // mb)

rng = np.random.default_rng(0)
yi = rng.integers(0, k, size=n)
X = np.abs(rng.standard_normal((n, nf), dtype=np.float32) * np.float32(0.4) + np.float32(0.4))
fs = FeatureSet(nf, np.arange(k), reserve=n).append(X, yi)
Xe = np.ascontiguousarray(X[:16384])
del X
lib = _lib.lib()
variants = [("plain", False), ("batch normalisation", True)]


def member(seed, bn):
    clf = TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), learning_rate_init=1e-4, random_state=seed, batch_norm=bn)
    clf.classes_, clf.n_features_in_, clf.n_iter_, clf.loss_curve_ = np.arange(k), nf, 0, []
    clf._class_weight_vector = None
    clf._create_trainer(*clf._initial_parameters())
    return clf, np.ascontiguousarray(np.random.default_rng(seed).permutation(n).astype(np.int64))


def solo_pass(clf, visit):
    avg = C.c_double(0.0)
    _lib.check(lib.mmc_trainer_partial_fit_set(clf._h, fs._handle(), visit.ctypes.data, n, mb, C.byref(avg), None))
    return avg.value


def group_pass(members):
    count = len(members)
    handles = (C.c_void_p * count)(*[clf._h.value for clf, _ in members])
    visits = (C.c_void_p * count)(*[v.ctypes.data for _, v in members])
    avg = (C.c_double * count)()
    ns, mbs = (C.c_int64 * count)(*[n] * count), (C.c_int * count)(*[mb] * count)
    _lib.check(lib.mmc_trainer_group_partial_fit_set(handles, count, fs._handle(), visits, ns, mbs, avg, None))
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


print(f"{n} resident rows x {nf}, {k} classes, 1280 -> 500 -> 300 -> 100 -> {k}, mini-batches of {mb}: {steps} Adam steps per model and pass")
print(f"host clock around calls that end in a stream synchronise; one warm-up per variant, then the variants in turn, {args.repeats} times "
      "each; median (min .. max) in ms")
solo = {name: member(0, bn) for name, bn in variants}
got = measure([(name, lambda m=m: solo_pass(*m)) for name, m in solo.items()])
base = got["plain"][0]
for name, _ in variants:
    med, lo, hi = got[name]
    print(f"solo  {name:30s} {med:9.1f} ({lo:9.1f} .. {hi:9.1f})   {med / base:6.3f} x plain   {(med - base) / steps * 1e3:6.2f} us a step")

S = args.sweep
sweeps = [(name, [member(m, bn) for m in range(S)]) for name, bn in variants]
sweeps.append((f"{S // 2} plain + {S - S // 2} normalised", [member(m, m >= S // 2) for m in range(S)]))
got = measure([(name, lambda g=g: group_pass(g)) for name, g in sweeps])
base = got["plain"][0]
for name, _ in sweeps:
    med, lo, hi = got[name]
    print(f"group of {S}: {name:30s} {med:9.1f} ({lo:9.1f} .. {hi:9.1f})   {S * steps / med * 1e3:8.0f} model-steps/s   "
          f"{med / base:6.3f} x plain   {(med - base) / steps * 1e3:6.2f} us a step")

# the eval-mode forward: a one-mini-batch step makes the fold stale, so the forward after it launches bn_fold_kernel first
clf, _ = solo["batch normalisation"]
plain, _ = solo["plain"]
out = np.empty((len(Xe), k), np.float32)
two = np.ascontiguousarray(np.arange(mb, dtype=np.int64))


def forward(c, stale):
    if stale:
        avg = C.c_double(0.0)
        _lib.check(lib.mmc_trainer_partial_fit_set(c._h, fs._handle(), two.ctypes.data, mb, mb, C.byref(avg), None))
    t = time.perf_counter()
    _lib.check(lib.mmc_trainer_logits(c._h, Xe.ctypes.data, len(Xe), out.ctypes.data, None))
    return (time.perf_counter() - t) * 1e3


for name, c, stale in (("plain", plain, True), ("normalised, fold current", clf, False), ("normalised, fold stale", clf, True)):
    forward(c, stale)
    ms = sorted(forward(c, stale) for _ in range(2 * args.repeats + 1))
    print(f"eval forward of {len(Xe)} rows, upload and download included: {name:26s} {ms[len(ms) // 2]:7.2f} ({ms[0]:7.2f} .. {ms[-1]:7.2f})")
