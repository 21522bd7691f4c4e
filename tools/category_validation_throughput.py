#!/usr/bin/env python3
"""GPU box: per-category reliability tables of a resident split, metrics.grouped_validate(..., category_of_class=...) against the
same call without categories and against validate(rows=True) plus one argsort per category on the host.

    python tools/category_validation_throughput.py [--rows 1000000] [--images 40000] [--categories 12] [--repeats 3]
                                                   [--out profiles/category_validation_throughput.txt] [--commit ID]

The production head 1280 -> 500 -> 300 -> 100 -> 108 (seeded weights and Platt parameters), a FeatureSet of `rows` seeded rows in
`images` images of seeded sizes, 20 global bins, the classes dealt round-robin to `categories` categories.
  categories  grouped_validate(model, set, sizes, category_of_class=...): mmc_head_evaluate_categories_set; the tables come back, no
              row does
  grouped     grouped_validate(model, set, sizes): mmc_head_evaluate_grouped_set, the same call without the category pass: the baseline
              the category pass is measured against
  host        validate(model, set) (16 B per row to the host) and then, per category, in numpy: a stable argsort by (score, correct)
              and the per-bin sums
Every variant ends with its results on the host (each call synchronises), so the host clock around a call is the figure.  The
variants are taken in turn, `repeats` times after one warm-up round; the figure per variant is the median.  The category tables of
the two routes are compared for identity first.  Needs nothing but the package.
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
N_BINS = 20
KERNELS_PER_CATEGORY, MEMSETS_PER_CATEGORY = 9, 4   # mask, init, 3 x (histogram, scan), binned sums; a clear before each histogram and
                                                    # before the sums (metrics.hip: launch_group_select_category)


def commit_id():
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown (not a git checkout)"


def host_tables(v, cat, C):
    """The category tables from a Validation with rows, in numpy: per category count / n_correct / conf_q32 per bin."""
    from mermaid_classifier_amd import category_bins
    ok = (v.gt >= 0) & np.isfinite(v.scores)
    g, e, score = v.gt[ok].astype(np.int64), v.est[ok].astype(np.int64), v.scores[ok]
    correct = e == g
    sq = np.rint(score * 2.0 ** 32).astype(np.int64)
    row_cat = cat[g]
    out = {}
    for c in range(C):
        rows = np.flatnonzero(row_cat == c)
        if len(rows) == 0:
            continue
        nb = category_bins(len(rows))
        rows = rows[np.lexsort((correct[rows], score[rows]))]
        edges = np.arange(nb + 1) * len(rows) // nb
        keep = np.diff(edges) > 0
        cnt, cor, cq = np.zeros(nb, np.int64), np.zeros(nb, np.int64), np.zeros(nb, np.int64)
        cnt[:] = np.diff(edges)
        cor[keep] = np.add.reduceat(correct[rows].astype(np.int64), edges[:-1][keep])
        cq[keep] = np.add.reduceat(sq[rows], edges[:-1][keep])
        out[c] = (cnt, cor, cq)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--images", type=int, default=40000)
    ap.add_argument("--categories", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "category_validation_throughput.txt"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    if args.rows < N_BINS or args.repeats < 1 or not 1 <= args.images <= args.rows or not 1 <= args.categories <= 64:
        ap.error("--rows, --images (<= rows), --categories (<= 64) and --repeats must be positive")
    import torch
    if not torch.cuda.is_available():
        sys.exit("category_validation_throughput.py measures on the GPU: no HIP device visible")
    from mermaid_classifier_amd import CalibratedMLP, FeatureSet, grouped_validate, validate

    rng = np.random.default_rng(0)
    K, N, C = DIMS[-1], args.rows, args.categories
    weights = [(rng.normal(0, 1, (o, i)) * np.sqrt(2.0 / i)).astype(np.float32) for i, o in zip(DIMS[:-1], DIMS[1:])]
    biases = [rng.normal(0, 0.05, o).astype(np.float32) for o in DIMS[1:]]
    classes = [f"class {i:03d}" for i in range(K)]
    model = CalibratedMLP(weights, biases, classes, rng.uniform(-12, -4, K), rng.uniform(0.5, 3, K))
    fs = FeatureSet(DIMS[0], classes, reserve=N)
    block = rng.normal(0.3, 0.6, (min(FILL, N), DIMS[0])).astype(np.float32)
    for first in range(0, N, FILL):   # the same seeded block, shifted per append: distinct rows without N x 1280 host floats
        cur = min(FILL, N - first)
        fs.append(block[:cur] + np.float32(1e-3 * (first // FILL)), np.asarray(classes)[rng.integers(0, K, cur)])
    cuts = np.sort(rng.choice(np.arange(1, N), args.images - 1, replace=False)) if args.images > 1 else np.zeros(0, np.int64)
    sizes = np.diff(np.concatenate([[0], cuts, [N]])).astype(np.int64)
    cat = (np.arange(K) % C).astype(np.int64)

    phases = {}

    def host():
        t0 = time.perf_counter()
        v = validate(model, fs)
        t1 = time.perf_counter()
        tables = host_tables(v, cat, C)
        phases["validate(rows=True)"], phases["argsort per category"] = t1 - t0, time.perf_counter() - t1
        return tables

    variants = {"categories": lambda: grouped_validate(model, fs, sizes, n_bins=N_BINS, category_of_class=cat),
                "grouped": lambda: grouped_validate(model, fs, sizes, n_bins=N_BINS), "host": host}
    warm = {name: fn() for name, fn in variants.items()}   # warm-up: module load, scratch growth
    gv, plain, want = warm["categories"], warm["grouped"], warm["host"]
    same = sorted(gv.category_reliability) == sorted(want)
    for c, (cnt, cor, cq) in want.items():
        rel = gv.category_reliability.get(c)
        same = bool(same and rel is not None and np.array_equal(rel.count, cnt) and np.array_equal(rel.n_correct, cor)
                    and np.array_equal(rel.conf_q32, cq))
    kept = all(getattr(gv.reliability, k).tobytes() == getattr(plain.reliability, k).tobytes() for k in ("count", "n_correct", "conf_q32",
                                                                                                         "conf_min", "conf_max"))
    kept = bool(kept and gv.cover.sums.tobytes() == plain.cover.sums.tobytes() and np.array_equal(gv.support, plain.support)
                and np.array_equal(gv.nll_q32, plain.nll_q32) and np.array_equal(gv.score_q32, plain.score_q32))
    times = {name: [] for name in variants}
    split = {"validate(rows=True)": [], "argsort per category": []}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
            if name == "host":
                for k in split:
                    split[k].append(phases[k])
    med = {k: statistics.median(x) for k, x in times.items()}
    added = med["categories"] - med["grouped"]
    lines = [
        f"# python tools/category_validation_throughput.py --rows {N} --images {args.images} --categories {C} --repeats {args.repeats}",
        f"# commit {args.commit or commit_id()}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
        f"# head {' -> '.join(map(str, DIMS))}, a resident set of {N:,} rows in {args.images:,} images, {C} categories, {N_BINS} global "
        f"bins; variants in turn, {args.repeats} repeats after a warm-up round, host clock around calls that end in a synchronise, median",
        f"category tables of the device and the host route identical: {same}; grouped outputs of the two device calls identical: {kept}",
        f"rows per category: {[int(r.count.sum()) for _, r in sorted(gv.category_reliability.items())]}",
    ]
    for name in variants:
        s = [f"{x:.4f}" for x in times[name]]
        lines.append(f"{name:10s} median {med[name]:8.4f} s = {N / med[name]:12,.0f} rows/s   (repeats {' '.join(s)} s)")
    for k, x in split.items():
        lines.append(f"  host, {k}: median {statistics.median(x):.4f} s")
    lines.append(f"the category pass adds {added * 1e3:.2f} ms to the grouped call ({added / med['grouped'] * 100:.1f} % of it): {C} categories x "
                 f"({KERNELS_PER_CATEGORY} kernels + {MEMSETS_PER_CATEGORY} memsets), {added / C * 1e3:.3f} ms per category")
    lines.append(f"ratio host / categories = {med['host'] / med['categories']:.2f}")
    lines.append(f"bytes to the host for the category tables: device route {C * (8 + 4 + 20 * (3 * 8 + 2 * 4)):,}; host route {N * 16 + N * 4:,}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)
    if not same or not kept:
        sys.exit("the routes disagree")


if __name__ == "__main__":
    main()
