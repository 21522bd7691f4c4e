#!/usr/bin/env python3
"""GPU box: scoring a resident validation split, validation.validate against the route a user composes from the pieces.

    python tools/validation_throughput.py [--rows 1000000] [--repeats 3] [--out profiles/validation_throughput.txt] [--commit ID]

The production head 1280 -> 500 -> 300 -> 100 -> 108 (seeded weights and Platt parameters) and a FeatureSet of `rows` seeded rows.
  rows      validate(model, set): mmc_head_evaluate_set with calibrate_eval_kernel; per row est, score, rank, p_true come back (16 B)
  totals    validate(model, set, rows=False): only the integer totals, the rank histogram and the confusion table come back
  composed  FeatureSet.read (rows to the host) -> CalibratedMLP.predict_proba (rows up again, N x K probabilities down, float64) ->
            numpy argmax, stable argsort of -P, the rank of the true class, bincount of ranks and of (gt, est)
Every variant ends with its results on the host (each call synchronises), so the host clock around a call is the figure.  The
variants are taken in turn, `repeats` times after one warm-up round; the figure per variant is the median.  The three routes'
est / ranks / tables are compared for identity first.  Needs nothing but the package.
"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DIMS = (1280, 500, 300, 100, 108)
FILL = 65536   # rows per append while the set is filled


def commit_id():
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown (not a git checkout)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "validation_throughput.txt"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    if args.rows < 1 or args.repeats < 1:
        ap.error("--rows and --repeats must be positive")
    import torch
    if not torch.cuda.is_available():
        sys.exit("validation_throughput.py measures on the GPU: no HIP device visible")
    from mermaid_classifier_amd import CalibratedMLP, FeatureSet, validate

    rng = np.random.default_rng(0)
    K, N = DIMS[-1], args.rows
    weights = [(rng.normal(0, 1, (o, i)) * np.sqrt(2.0 / i)).astype(np.float32) for i, o in zip(DIMS[:-1], DIMS[1:])]
    biases = [rng.normal(0, 0.05, o).astype(np.float32) for o in DIMS[1:]]
    classes = [f"class {i:03d}" for i in range(K)]
    model = CalibratedMLP(weights, biases, classes, rng.uniform(-12, -4, K), rng.uniform(0.5, 3, K))
    fs = FeatureSet(DIMS[0], classes, reserve=N)
    block = rng.normal(0.3, 0.6, (min(FILL, N), DIMS[0])).astype(np.float32)
    for first in range(0, N, FILL):   # the same seeded block, shifted per append: distinct rows without N x 1280 host floats
        cur = min(FILL, N - first)
        fs.append(block[:cur] + np.float32(1e-3 * (first // FILL)), np.asarray(classes)[rng.integers(0, K, cur)])

    def composed():
        X, y = fs.read()
        P = model.predict_proba(X)
        gt = np.searchsorted(np.asarray(classes), y)
        est = P.argmax(1)
        order = np.argsort(-P, axis=1, kind="stable")
        ranks = 1 + np.argmax(order == gt[:, None], axis=1)
        return est, ranks, np.bincount(ranks - 1, minlength=K), np.bincount(gt * K + est, minlength=K * K).reshape(K, K)

    variants = {"rows": lambda: validate(model, fs), "totals": lambda: validate(model, fs, rows=False), "composed": composed}
    warm = {name: fn() for name, fn in variants.items()}   # warm-up: module load, staging growth
    est, ranks, hist, conf = warm["composed"]
    v, t = warm["rows"], warm["totals"]
    same = bool(np.array_equal(v.est, est) and np.array_equal(v.ranks, ranks) and np.array_equal(v.rank_hist, hist)
                and np.array_equal(v.confusion, conf) and np.array_equal(t.rank_hist, hist) and np.array_equal(t.confusion, conf)
                and t.n_correct == v.n_correct == int((est == v.gt).sum()) and t.nll_q32 == v.nll_q32)
    times = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    med = {k: statistics.median(x) for k, x in times.items()}
    lines = [
        "# " + " ".join(["python", "tools/validation_throughput.py"] + sys.argv[1:]),
        f"# commit {args.commit or commit_id()}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
        f"# head {' -> '.join(map(str, DIMS))}, a resident set of {N:,} rows; variants in turn, {args.repeats} repeats after a warm-up round, "
        "host clock around calls that end in a synchronise, median",
        f"est, ranks, rank histogram, confusion, n_correct of the routes identical: {same}",
    ]
    for name in variants:
        s = [f"{x:.3f}" for x in times[name]]
        lines.append(f"{name:9s} median {med[name]:8.3f} s = {N / med[name]:12,.0f} rows/s   (repeats {' '.join(s)} s)")
    lines.append(f"ratio composed / rows = {med['composed'] / med['rows']:.2f}; composed / totals = {med['composed'] / med['totals']:.2f}")
    lines.append(f"bytes to the host per pass: rows {N * 16 + (K * K + K + 5) * 8:,}; totals {(K * K + K + 5) * 8:,}; composed "
                 f"{N * DIMS[0] * 4 + N * K * 4:,} (features + probabilities), plus {N * DIMS[0] * 4:,} back up for the head")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)
    if not same:
        sys.exit("the routes disagree")


if __name__ == "__main__":
    main()
