#!/usr/bin/env python3
"""GPU box: what distillation costs (profiles/distillation.txt).

One pass of the production head (1280 -> 500 -> 300 -> 100 -> 108, mini-batches of 200) over a resident set of 200 000 rows: plain
(ce_grad_kernel), then with a target set and mmc_trainer_set_distillation on the trainer (ce_grad_distill_kernel) at alpha = 0.5,
tau = 1 and tau = 2.  Then the same three as one grouped call of eight heads in which every member carries the option and all read one
shared target set.  Before that, the fill: teacher_targets for an ensemble of eight production heads against mmc_ensemble_topk with
proba (device outputs) on the same rows.

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
import torch  # noqa: E402
from mermaid_classifier_amd import CalibratedMLP, FeatureSet, HeadEnsemble, _lib, teacher_targets  # noqa: E402
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
Xd = torch.from_numpy(X).cuda()
del X
lib = _lib.lib()


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

# ---- the fill: eight production heads with Xavier weights and a Platt slope of -1 ---------------------------------------------------
dims = (nf, 500, 300, 100, k)
teachers = []
for seed in range(8):
    r = np.random.default_rng(100 + seed)
    W = [(r.uniform(-1, 1, (dims[i + 1], dims[i])) * np.sqrt(6.0 / (dims[i] + dims[i + 1]))).astype(np.float32) for i in range(4)]
    teachers.append(CalibratedMLP(W, [np.zeros(dims[i + 1], np.float32) for i in range(4)], np.arange(k), np.full(k, -1.0), np.zeros(k)))
ens = HeadEnsemble(teachers)


def fill():
    ts = teacher_targets(ens, fs)
    torch.cuda.synchronize()
    return ts


def topk_proba():
    out = ens.topk(Xd, 1, want_proba=True)
    torch.cuda.synchronize()
    return out


def fill_and_free():
    fill().close()


got = measure([("teacher_targets (mmc_ensemble_predict_set)", fill_and_free), ("mmc_ensemble_topk with proba, device outputs", topk_proba)])
base = got["mmc_ensemble_topk with proba, device outputs"][0]
for name, (med, lo, hi) in got.items():
    print(f"fill  {name:46s} {med:9.1f} ({lo:9.1f} .. {hi:9.1f})   {med / base:6.3f} x topk   {n / med * 1e3:10.0f} rows/s")
targets = fill()
del Xd

# ---- the passes ------------------------------------------------------------------------------------------------------------------------
variants = [("plain", 0.0, 1.0), ("distilled alpha 0.5 tau 1", 0.5, 1.0), ("distilled alpha 0.5 tau 2", 0.5, 2.0)]


def member(seed, alpha, tau):
    clf = TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), learning_rate_init=1e-4, random_state=seed, distill_alpha=alpha,
                             distill_temperature=tau)
    clf.classes_, clf.n_features_in_, clf.n_iter_, clf.loss_curve_ = np.arange(k), nf, 0, []
    clf._class_weight_vector = None
    clf._create_trainer(*clf._initial_parameters())
    return clf, np.ascontiguousarray(np.random.default_rng(seed).permutation(n).astype(np.int64))


def solo_pass(clf, visit):
    avg = C.c_double(0.0)
    if clf.distill_alpha:
        _lib.check(lib.mmc_trainer_partial_fit_set_distill(clf._h, fs._handle(), targets._handle(), visit.ctypes.data, None, None, n, mb,
                                                           C.byref(avg), None))
    else:
        _lib.check(lib.mmc_trainer_partial_fit_set(clf._h, fs._handle(), visit.ctypes.data, n, mb, C.byref(avg), None))
    return avg.value


def group_pass(members):
    count = len(members)
    handles = (C.c_void_p * count)(*[clf._h.value for clf, _ in members])
    visits = (C.c_void_p * count)(*[v.ctypes.data for _, v in members])
    avg = (C.c_double * count)()
    ns, mbs = (C.c_int64 * count)(*[n] * count), (C.c_int * count)(*[mb] * count)
    if members[0][0].distill_alpha:
        ts = (C.c_void_p * count)(*[targets._handle().value] * count)
        _lib.check(lib.mmc_trainer_group_partial_fit_set_distill(handles, count, fs._handle(), ts, visits, None, None, ns, mbs, avg, None))
    else:
        _lib.check(lib.mmc_trainer_group_partial_fit_set(handles, count, fs._handle(), visits, ns, mbs, avg, None))
    return list(avg)


routes = []
for name, alpha, tau in variants:
    clf, visit = member(0, alpha, tau)
    routes.append((name, lambda clf=clf, visit=visit: solo_pass(clf, visit)))
got = measure(routes)
base = got[variants[0][0]][0]
for name, *_ in variants:
    med, lo, hi = got[name]
    print(f"solo  {name:30s} {med:9.1f} ({lo:9.1f} .. {hi:9.1f})   {med / base:6.3f} x plain   {(med - base) / steps * 1e3:6.2f} us a step")

S = args.sweep
sweeps = [(name, [member(m, alpha, tau) for m in range(S)]) for name, alpha, tau in variants]
got = measure([(name, lambda g=g: group_pass(g)) for name, g in sweeps])
base = got[variants[0][0]][0]
for name, *_ in variants:
    med, lo, hi = got[name]
    print(f"group of {S}, every member: {name:30s} {med:9.1f} ({lo:9.1f} .. {hi:9.1f})   {S * steps / med * 1e3:8.0f} model-steps/s   "
          f"{med / base:6.3f} x plain   {(med - base) / steps * 1e3:6.2f} us a step")
