#!/usr/bin/env python3
"""GPU box: the ranking tables of a resident split, ranking.ranking_validate against the host route it replaces.

    python tools/ranking_validation_throughput.py [--rows 1000000] [--max-k 10] [--repeats 3]
                                                  [--out profiles/ranking_validation_throughput.txt] [--commit ID]

The production head 1280 -> 500 -> 300 -> 100 -> 108 (seeded weights and Platt parameters), a FeatureSet of `rows` seeded rows, a
seeded similarity matrix over four categories with the values 0, 1/3, 1/2, 2/3 and 1.
  ranked    ranking_validate(model, set, similarity=S): mmc_head_evaluate_ranked_set with rank_rows_kernel; two tables come back
  validate  validate(model, set, rows=False), for scale: the evaluation without the ranking pass
  host      the route this replaces: FeatureSet.read -> predict_proba -> np.argsort(-proba, kind="stable") (in blocks of 65 536 rows,
            so the host holds one block of features) and the same two tables in numpy.  The stable sort makes the host order the
            device's (equal probabilities in class order; the reference's default sort leaves it open), so the tables must agree
Every variant ends with its results on the host (each call synchronises), so the host clock around a call is the figure.  The
variants are taken in turn, `repeats` times after one warm-up round; the figure per variant is the median.  The tables of the two
routes are compared first: class_rank_hist and hier_hist must be identical.  Needs nothing but the package.
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
FILL = 65536   # rows per append while the set is filled, and per block of the host route


def commit_id():
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown (not a git checkout)"


def host_tables(model, fs, levels, n_levels, kmax):
    """The reference's route (metrics/coordinator.py:59-76, ranking.py:55-61, :176-184) with the table sums in numpy.
    -> (class_rank_hist, hier_hist)."""
    K = len(model.classes_)
    where = {c: i for i, c in enumerate(np.asarray(model.classes_).tolist())}
    class_hist, hier = np.zeros(K * K, np.int64), np.zeros((kmax, n_levels), np.int64)
    for first in range(0, len(fs), FILL):
        X, labels = fs.read(first, min(FILL, len(fs) - first))
        proba = model.predict_proba(X)
        g = np.array([where[c] for c in labels.tolist()], np.int64)
        order = np.argsort(-proba, axis=1, kind="stable")
        rank = np.argmax(order == g[:, None], axis=1)
        class_hist += np.bincount(g * K + rank, minlength=K * K)
        m = np.maximum.accumulate(levels[g[:, None], order[:, :kmax]], axis=1)
        for j in range(kmax):
            hier[j] += np.bincount(m[:, j], minlength=n_levels)
    return class_hist.reshape(K, K), hier


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--max-k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ranking_validation_throughput.txt"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    if args.rows < 1 or args.repeats < 1 or not 1 <= args.max_k <= 16:
        ap.error("--rows and --repeats must be positive, --max-k in [1, 16]")
    import torch
    if not torch.cuda.is_available():
        sys.exit("ranking_validation_throughput.py measures on the GPU: no HIP device visible")
    from mermaid_classifier_amd import CalibratedMLP, FeatureSet, ranking_validate, similarity_levels, validate

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
    category = np.arange(K) // 27
    S = np.array([1 / 3, 1 / 2, 2 / 3])[rng.integers(0, 3, (K, K))]
    S = np.where(category[:, None] == category[None, :], np.maximum(S, S.T), 0.0)
    np.fill_diagonal(S, 1.0)
    levels, values = similarity_levels(S)
    kmax = min(args.max_k, K)

    variants = {"ranked": lambda: ranking_validate(model, fs, similarity=S, max_k=kmax),
                "validate": lambda: validate(model, fs, rows=False),
                "host": lambda: host_tables(model, fs, levels, len(values), kmax)}
    warm = {name: fn() for name, fn in variants.items()}   # warm-up: module load, scratch growth
    rv, (want_class, want_hier) = warm["ranked"], warm["host"]
    same = bool(np.array_equal(rv.class_rank_hist, want_class) and np.array_equal(rv.hier_hist, want_hier))
    times = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    med = {k: statistics.median(x) for k, x in times.items()}
    lines = [
        "# " + " ".join(["python", "tools/ranking_validation_throughput.py"] + sys.argv[1:]),
        f"# commit {args.commit or commit_id()}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
        f"# head {' -> '.join(map(str, DIMS))}, a resident set of {N:,} rows, kmax {kmax}, {len(values)} similarity levels; variants in turn, "
        f"{args.repeats} repeats after a warm-up round, host clock around calls that end in a synchronise, median",
        f"class_rank_hist and hier_hist of the two routes identical: {same}",
    ]
    for name in variants:
        s = [f"{x:.4f}" for x in times[name]]
        lines.append(f"{name:9s} median {med[name]:8.4f} s = {N / med[name]:12,.0f} rows/s   (repeats {' '.join(s)} s)")
    lines.append(f"ratio host / ranked = {med['host'] / med['ranked']:.2f}")
    lines.append(f"the ranking pass adds {med['ranked'] - med['validate']:.4f} s to validate(rows=False) "
                 f"({(med['ranked'] - med['validate']) / N * 1e9:.1f} ns per row)")
    lines.append(f"bytes to the host per pass: ranked {(2 * K * K + K + 5 + kmax * len(values)) * 8:,} (and {K * K:,} of levels to the device); "
                 f"host {N * DIMS[0] * 4 + N * 4:,} of features and labels, {N * K * 4:,} of probabilities")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)
    if not same:
        sys.exit("the routes disagree")
    if med["ranked"] >= med["host"]:
        sys.exit("the ranked call is not faster than the host route")


if __name__ == "__main__":
    main()
