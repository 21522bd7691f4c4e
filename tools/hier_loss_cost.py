#!/usr/bin/env python3
"""GPU box: what the taxonomy-aware loss costs in a training pass (profiles/hier_loss.txt).

One pass of the production head (1280 -> 500 -> 300 -> 100 -> 108, mini-batches of 200) over a resident set of 200 000 rows: plain
(ce_grad_kernel), then with mmc_trainer_set_hierarchy on the trainer (ce_grad_hier_kernel): one level, four levels, soft targets and
four levels.  Then the same four as one grouped call of eight heads in which every member carries the option.

The levels: 108 classes in 6 / 18 / 36 / 54 contiguous nodes (every tenth class has no node at the second level); T puts 0.7 on the
class and spreads 0.3 over its 17 siblings at the first level.

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
del X
lib = _lib.lib()

c = np.arange(k)
ids = np.stack([c // 18 * 18, c // 6 * 6, c // 3 * 3, c // 2 * 2]).astype(np.int32)
ids[1, c % 10 == 9] = -1
T = np.where(ids[0][None, :] == ids[0][:, None], 0.3 / 17.0, 0.0)
T[c, c] = 0.7
T = np.ascontiguousarray(T, np.float32)
LAM = np.array([1.0, 0.5, 0.25, 0.25])
variants = [("plain", 0, False), ("one level", 1, False), ("four levels", 4, False), ("soft targets + four levels", 4, True)]


def member(seed, n_levels, soft):
    clf = TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), learning_rate_init=1e-4, random_state=seed)
    clf.classes_, clf.n_features_in_, clf.n_iter_, clf.loss_curve_ = np.arange(k), nf, 0, []
    clf._class_weight_vector = None
    clf._hierarchy_arrays = None if not (n_levels or soft) else (np.ascontiguousarray(ids[:n_levels]), LAM[:n_levels].copy(), T if soft else None)
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
routes = []
for name, n_levels, soft in variants:
    clf, visit = member(0, n_levels, soft)
    routes.append((name, lambda clf=clf, visit=visit: solo_pass(clf, visit)))
got = measure(routes)
base = got[variants[0][0]][0]
for name, *_ in variants:
    med, lo, hi = got[name]
    print(f"solo  {name:30s} {med:9.1f} ({lo:9.1f} .. {hi:9.1f})   {med / base:6.3f} x plain   {(med - base) / steps * 1e3:6.2f} us a step")

S = args.sweep
sweeps = [(name, [member(m, n_levels, soft) for m in range(S)]) for name, n_levels, soft in variants]
got = measure([(name, lambda g=g: group_pass(g)) for name, g in sweeps])
base = got[variants[0][0]][0]
for name, *_ in variants:
    med, lo, hi = got[name]
    print(f"group of {S}, every member: {name:30s} {med:9.1f} ({lo:9.1f} .. {hi:9.1f})   {S * steps / med * 1e3:8.0f} model-steps/s   "
          f"{med / base:6.3f} x plain   {(med - base) / steps * 1e3:6.2f} us a step")
