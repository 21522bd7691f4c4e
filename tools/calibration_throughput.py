#!/usr/bin/env python3
"""GPU box: throughput of the device-side evaluation and Platt calibration (mermaid_classifier_amd/calibration.py,
csrc/calib.hip) at K = 108 classes.

    python tools/calibration_throughput.py                 fit / calibrate / evaluate timings (+ host sklearn fit at 1e5)
    python tools/calibration_throughput.py --features-only the calibrate-from-features and evaluate lines alone (the trainer's forward
                                                           at 16384 rows a call; no score matrices, no host sklearn fit)
    python tools/calibration_throughput.py --fit-only N    one warm-up fit and one fit at N rows (for a rocprofv3 run)
    python tools/calibration_throughput.py --summarize kernel_trace.csv N
                                                           platt_pass_kernel launches of that rocprofv3 trace: bytes of F read
                                                           per launch (active classes x N x 4) over kernel time
"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

K, D = 108, 1280
COPY_TBPS = 6.3   # measured HBM copy rate of the MI355X (MI355X_MICROARCH.md)


def scores(n, seed=0):
    rng = np.random.default_rng(seed)
    z = rng.normal(0.0, 2.0, size=(n, K)).astype(np.float32)
    z -= z.max(1, keepdims=True)
    np.exp(z, out=z)
    z /= z.sum(1, keepdims=True)
    y = rng.integers(0, K, size=n).astype(np.int32)
    return z.astype(np.float64), y


def device_fit(S, y):
    from mermaid_classifier_amd.calibration import _Calibrator
    cal = _Calibrator(K, 0)
    cal.add_scores(S, y)
    cal.fit()                                   # warm-up (first launches, module load)
    t0 = time.perf_counter()
    a, b, it = cal.fit()                        # synchronous: returns after the last pass's counter is read
    dt = time.perf_counter() - t0
    cal.close()
    return dt, it


def main(features_only=False):
    import torch  # noqa: F401  (HIP runtime of torch first, as the package does)
    from mermaid_classifier_amd.calibration import calibrate, evaluate
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    for n in () if features_only else (100_000, 1_000_000):
        S, y = scores(n)
        dt, it = device_fit(S, y)
        print(f"fit N={n} K={K}: {dt * 1e3:.2f} ms wall (device-synchronised), Newton trial points per class max {it.max()} "
              f"mean {it.mean():.2f}; F = {n * K * 4 / 1e6:.0f} MB fp32 per full pass")
        if n == 100_000:
            S1e5, y1e5 = S, y
        del S
    rng = np.random.default_rng(1)
    X = rng.normal(0.0, 1.0, size=(20_000, D)).astype(np.float32)
    yl = rng.integers(0, K, size=20_000)
    clf = TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), random_state=0)
    clf.partial_fit(X[:4000], yl[:4000], classes=list(range(K)))
    for n in (100_000, 1_000_000):
        reps = n // len(yl)
        evaluate(clf, (X[:1000], yl[:1000]))
        t0 = time.perf_counter()
        cm = calibrate(clf, ((X, yl) for _ in range(reps)))
        dt = time.perf_counter() - t0
        print(f"calibrate N={n} from features (1280 -> 500 -> 300 -> 100 -> 108, batches of 20000 incl. H2D of "
              f"{n * D * 4 / 1e9:.2f} GB + forward + fit): {n / dt:,.0f} rows/s ({dt:.2f} s); trial points max {cm.iterations_.max()}")
        t0 = time.perf_counter()
        evaluate(clf, ((X, yl) for _ in range(reps)))
        dt = time.perf_counter() - t0
        print(f"evaluate N={n}: {n / dt:,.0f} rows/s ({dt:.2f} s)")
    if features_only:
        return
    try:
        from sklearn.calibration import _SigmoidCalibration
    except ImportError:
        print("host sklearn fit: sklearn not importable")
        return
    import sklearn
    t0 = time.perf_counter()
    for k in range(K):
        _SigmoidCalibration().fit(S1e5[:, k], (y1e5 == k).astype(np.int64))
    dt = time.perf_counter() - t0
    print(f"host sklearn {sklearn.__version__} _SigmoidCalibration x {K} at N=100000: {dt:.2f} s")


def fit_only(n):
    import torch  # noqa: F401
    S, y = scores(n)
    dt, it = device_fit(S, y)
    print(f"fit N={n}: {dt * 1e3:.2f} ms, trial points max {it.max()}")


def summarize(csv_path, n):
    import csv
    rows = list(csv.DictReader(open(csv_path)))
    passes = [r for r in rows if "platt_pass_kernel" in r.get("Kernel_Name", "")]
    if not passes:
        print("no platt_pass_kernel launches in", csv_path)
        return
    out = []
    for r in passes:
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        active = int(r["Grid_Size_X"]) // int(r.get("Workgroup_Size_X", 256))
        out.append((active, ns))
    for label, sel in (("all classes active", [o for o in out if o[0] == K]), ("every launch", out)):
        if not sel:
            continue
        byts = np.array([a * n * 4 for a, _ in sel], np.float64)
        ns = np.array([t for _, t in sel], np.float64)
        tbps = byts / ns / 1e3
        print(f"platt_pass_kernel N={n}, {label}: {len(sel)} launches, median {np.median(ns) / 1e3:.1f} us, "
              f"F bytes / kernel time median {np.median(tbps):.2f} TB/s = {np.median(tbps) / COPY_TBPS:.1%} of the {COPY_TBPS} TB/s copy rate")
    tot = sum(t for _, t in out)
    print(f"platt_pass_kernel total {tot / 1e6:.2f} ms over {len(out)} launches (two fits: warm-up + timed)")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--fit-only":
        fit_only(int(sys.argv[2]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], int(sys.argv[3]))
    else:
        main(features_only="--features-only" in sys.argv[1:])
