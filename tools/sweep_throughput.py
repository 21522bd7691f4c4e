#!/usr/bin/env python3
"""GPU box: one training pass of S production heads (1280 -> 500 -> 300 -> 100 -> 108, mini-batches of 200) over a resident set of
200 000 rows, as one mmc_trainer_group_partial_fit_set call and as S mmc_trainer_partial_fit_set calls one after the other.

Wall clock around calls that end in their stream synchronise; every shape is warmed up once, then the two routes are taken in
turn, five times each; median and spread (min .. max) per route.  S in 1, 4, 8, 16.  Every member has its own initial weights
(seed) and visiting order, as the members of a sweep do.

--solo-only: the solo leg alone.  It needs nothing this script's commit added to the library, so it runs on an older checkout
too: that is how the solo figure is checked to be the earlier code's.
--loss KIND: the members' loss formulation (mmc_trainer_set_loss): plain (the default: no option is passed, so the leg runs on a
checkout from before the options too), smooth (label smoothing 0.1), focal (gamma 2), prior (0.7 log of a Dirichlet draw), all
(the three together), mixed (member m takes plain, smooth, focal, prior, all in turn: one group launch runs both instantiations).
--rows N / --sizes 1,4: smaller runs."""
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
ap.add_argument("--solo-only", action="store_true")
ap.add_argument("--rows", type=int, default=200000)
ap.add_argument("--sizes", default="1,4,8,16")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--loss", choices=["plain", "smooth", "focal", "prior", "all", "mixed"], default="plain")
args = ap.parse_args()
sizes = [int(s) for s in args.sizes.split(",")]
k, nf, n, mb = 108, 1280, args.rows, 200

rng = np.random.default_rng(0)
yi = rng.integers(0, k, size=n)
X = np.abs(rng.standard_normal((n, nf), dtype=np.float32) * np.float32(0.4) + np.float32(0.4))
fs = FeatureSet(nf, np.arange(k), reserve=n).append(X, yi)
del X
lib = _lib.lib()
prior = (0.7 * np.log(np.random.default_rng(1).dirichlet(np.ones(k)))).astype(np.float32)
LOSSES = {"plain": {}, "smooth": {"label_smoothing": 0.1}, "focal": {"focal_gamma": 2.0}, "prior": {},
          "all": {"label_smoothing": 0.1, "focal_gamma": 2.0}}
members = []
for m in range(max(sizes)):
    kind = list(LOSSES)[m % len(LOSSES)] if args.loss == "mixed" else args.loss
    clf = TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), learning_rate_init=1e-4, random_state=m, **LOSSES[kind])
    clf.classes_, clf.n_features_in_, clf.n_iter_, clf.loss_curve_ = np.arange(k), nf, 0, []
    clf._class_weight_vector = None
    if kind in ("prior", "all"):
        clf._logit_prior_vector = prior
    clf._create_trainer(*clf._initial_parameters())
    members.append((clf, np.ascontiguousarray(np.random.default_rng(m).permutation(n).astype(np.int64))))


def solo(count):
    avg = C.c_double(0.0)
    for clf, visit in members[:count]:
        _lib.check(lib.mmc_trainer_partial_fit_set(clf._h, fs._handle(), visit.ctypes.data, n, mb, C.byref(avg), None))


def group(count):
    handles = (C.c_void_p * count)(*[clf._h.value for clf, _ in members[:count]])
    visits = (C.c_void_p * count)(*[v.ctypes.data for _, v in members[:count]])
    avg = (C.c_double * count)()
    _lib.check(lib.mmc_trainer_group_partial_fit_set(handles, count, fs._handle(), visits, (C.c_int64 * count)(*[n] * count),
                                                     (C.c_int * count)(*[mb] * count), avg, None))


def stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


steps = -(-n // mb)
print(f"{n} resident rows x {nf}, {k} classes, 1280 -> 500 -> 300 -> 100 -> {k}, mini-batches of {mb}: {steps} Adam steps per model and pass")
print(f"loss formulation of the members: {args.loss}")
print(f"host clock around calls that end in a stream synchronise; one warm-up per shape, then the routes in turn, {args.repeats} times each; "
      "median (min .. max) in ms")
routes = [("solo", solo)] if args.solo_only else [("solo", solo), ("group", group)]
for count in sizes:
    for _, fn in routes:
        fn(count)
    times = {name: [] for name, _ in routes}
    for _ in range(args.repeats):
        for name, fn in routes:
            t = time.perf_counter()
            fn(count)
            times[name].append((time.perf_counter() - t) * 1e3)
    line = f"S = {count:2d}:"
    for name, _ in routes:
        med, lo, hi = stats(times[name])
        what = f"{count} solo calls" if name == "solo" else "1 group call "
        line += f"  {what} {med:9.1f} ({lo:9.1f} .. {hi:9.1f})  {count * steps / med * 1e3:8.0f} model-steps/s;"
    if not args.solo_only:
        s_med, s_lo, s_hi = stats(times["solo"])
        g_med, g_lo, g_hi = stats(times["group"])
        line += f"  solo / group = {s_med / g_med:.2f}x (of the medians; {s_lo / g_hi:.2f} .. {s_hi / g_lo:.2f} over the spreads)"
    print(line, flush=True)
