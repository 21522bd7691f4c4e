#!/usr/bin/env python3
"""GPU box: the grouped validation tables of a resident split, metrics.grouped_validate against validate(rows=True) plus the
reductions on the host.

    python tools/grouped_validation_throughput.py [--rows 1000000] [--images 40000] [--sources 50] [--repeats 3]
                                                  [--out profiles/grouped_validation_throughput.txt] [--commit ID]

The production head 1280 -> 500 -> 300 -> 100 -> 108 (seeded weights and Platt parameters), a FeatureSet of `rows` seeded rows in
`images` images of seeded sizes, `sources` sources, 20 bins.
  grouped   grouped_validate(model, set, sizes, source_of_image=...): mmc_head_evaluate_grouped_set; the tables come back, no row does
  baseline  validate(model, set) (16 B per row to the host) and then, in numpy: per-image class counts and the eight cover sums, one
            confusion table per source, the per-class sums, a lexsort by (score, correct) and the per-bin sums
  validate  validate(model, set, rows=False), for scale: what the evaluation without any grouped table costs
Every variant ends with its results on the host (each call synchronises), so the host clock around a call is the figure.  The
variants are taken in turn, `repeats` times after one warm-up round; the figure per variant is the median.  The integer tables of
the two routes are compared for identity first, the cover sums to 1e-12 of the sum of their absolute terms.  Needs nothing but the
package.
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


def commit_id():
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown (not a git checkout)"


def host_tables(v, sizes, source, S, K):
    """The grouped tables from a Validation with rows, in numpy."""
    ok = (v.gt >= 0) & np.isfinite(v.scores)
    image = np.repeat(np.arange(len(sizes)), sizes)[ok]
    g, e = v.gt[ok].astype(np.int64), v.est[ok].astype(np.int64)
    score, p_true = v.scores[ok], v.p_true[ok].astype(np.float64)
    nll = np.rint(-np.log(np.clip(p_true, 1e-15, 1.0)) * 2.0 ** 32).astype(np.int64)
    sq = np.rint(score * 2.0 ** 32).astype(np.int64)
    out = dict(support=np.bincount(g, minlength=K),
               source_confusion=np.bincount((source[image] * K + g) * K + e, minlength=S * K * K).reshape(S, K, K))
    by_class = np.argsort(g, kind="stable")
    starts = np.searchsorted(g[by_class], np.arange(K + 1))
    out["nll_q32"] = np.array([nll[by_class[a:b]].sum() for a, b in zip(starts[:-1], starts[1:])], np.int64)
    out["score_q32"] = np.array([sq[by_class[a:b]].sum() for a, b in zip(starts[:-1], starts[1:])], np.int64)
    n_images = len(sizes)
    true_cnt = np.bincount(image * K + g, minlength=n_images * K).reshape(n_images, K)
    pred_cnt = np.bincount(image * K + e, minlength=n_images * K).reshape(n_images, K)
    points = np.bincount(image, minlength=n_images)
    used = points > 0
    t, p = true_cnt[used] / points[used, None], pred_cnt[used] / points[used, None]
    d = p - t
    dev = t - t.sum(0) / used.sum()
    out["cover"] = np.stack([t.sum(0), p.sum(0), d.sum(0), (d * d).sum(0), np.abs(d).sum(0), t.min(0), t.max(0), (dev * dev).sum(0)], 1)
    out["cover_abs"] = np.stack([t.sum(0), p.sum(0), np.abs(d).sum(0), (d * d).sum(0), np.abs(d).sum(0), t.min(0), t.max(0), (dev * dev).sum(0)], 1)
    correct = e == g
    order = np.lexsort((correct, score))
    edges = np.arange(N_BINS + 1) * len(order) // N_BINS
    out["bin_count"] = np.diff(edges)
    out["bin_correct"] = np.add.reduceat(correct[order].astype(np.int64), edges[:-1])
    out["bin_conf_q32"] = np.add.reduceat(sq[order], edges[:-1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--images", type=int, default=40000)
    ap.add_argument("--sources", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "grouped_validation_throughput.txt"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    if args.rows < N_BINS or args.repeats < 1 or not 1 <= args.images <= args.rows or args.sources < 1:
        ap.error("--rows, --images (<= rows), --sources and --repeats must be positive")
    import torch
    if not torch.cuda.is_available():
        sys.exit("grouped_validation_throughput.py measures on the GPU: no HIP device visible")
    from mermaid_classifier_amd import CalibratedMLP, FeatureSet, grouped_validate, validate

    rng = np.random.default_rng(0)
    K, N, S = DIMS[-1], args.rows, args.sources
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
    source = rng.integers(0, S, args.images).astype(np.int64)

    phases = {}

    def baseline():
        t0 = time.perf_counter()
        v = validate(model, fs)
        t1 = time.perf_counter()
        tables = host_tables(v, sizes, source, S, K)
        phases["validate(rows=True)"], phases["host reductions"] = t1 - t0, time.perf_counter() - t1
        return tables

    variants = {"grouped": lambda: grouped_validate(model, fs, sizes, source_of_image=source, n_bins=N_BINS), "baseline": baseline,
                "validate": lambda: validate(model, fs, rows=False)}
    warm = {name: fn() for name, fn in variants.items()}   # warm-up: module load, scratch growth
    gv, want = warm["grouped"], warm["baseline"]
    same = bool(np.array_equal(gv.support, want["support"]) and np.array_equal(gv.score_q32, want["score_q32"])
                and np.array_equal(gv.sources.confusion, want["source_confusion"])
                and np.array_equal(gv.reliability.count, want["bin_count"]) and np.array_equal(gv.reliability.n_correct, want["bin_correct"])
                and np.array_equal(gv.reliability.conf_q32, want["bin_conf_q32"]))
    nll_gap = int(np.abs(gv.nll_q32 - want["nll_q32"]).sum())   # device log against host log: at most one 2^-32 unit per row
    scale = np.where(want["cover_abs"] > 0, want["cover_abs"], 1.0)
    cover_gap = float((np.abs(gv.cover.sums - want["cover"]) / scale).max())
    times = {name: [] for name in variants}
    split = {"validate(rows=True)": [], "host reductions": []}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
            if name == "baseline":
                for k in split:
                    split[k].append(phases[k])
    med = {k: statistics.median(x) for k, x in times.items()}
    lines = [
        "# " + " ".join(["python", "tools/grouped_validation_throughput.py"] + sys.argv[1:]),
        f"# commit {args.commit or commit_id()}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
        f"# head {' -> '.join(map(str, DIMS))}, a resident set of {N:,} rows in {args.images:,} images, {S} sources, {N_BINS} bins; variants in "
        f"turn, {args.repeats} repeats after a warm-up round, host clock around calls that end in a synchronise, median",
        f"integer tables of the two routes identical: {same}; per-class loss sums differ by {nll_gap} units of 2^-32 in all (device log "
        f"against host log); cover sums within {cover_gap:.3g} relative to the sum of absolute terms",
    ]
    for name in variants:
        s = [f"{x:.3f}" for x in times[name]]
        lines.append(f"{name:9s} median {med[name]:8.3f} s = {N / med[name]:12,.0f} rows/s   (repeats {' '.join(s)} s)")
    for k, x in split.items():
        lines.append(f"  baseline, {k}: median {statistics.median(x):.3f} s")
    ratio = med["baseline"] / med["grouped"]
    lines.append(f"ratio baseline / grouped = {ratio:.2f}" + ("" if ratio >= 1 else
                 f": the grouped call is {1 / ratio:.2f}x slower; its passes over the evaluation cost {med['grouped'] - med['validate']:.3f} s"))
    lines.append(f"the grouped pass adds {med['grouped'] - med['validate']:.3f} s to validate(rows=False)")
    lines.append(f"bytes to the host per pass: grouped {(S * K * K + K * K + 4 * K + 5 + 8 * K + 3 * N_BINS) * 8 + 2 * N_BINS * 4:,}; "
                 f"baseline {N * 16 + N * 4 + (K * K + K + 5) * 8:,}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)
    if not same or cover_gap > 1e-12 or nll_gap > N:
        sys.exit("the routes disagree")


if __name__ == "__main__":
    main()
