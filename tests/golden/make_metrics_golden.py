"""Generate tests/golden/metrics_fixture.npz: the reference's own ``_adaptive_ece`` (metrics/calibration.py), ``compute_cover``
(metrics/cover.py) and ``compute_per_source`` (metrics/per_source.py) on seeded validation results.

    python tests/golden/make_metrics_golden.py /path/to/mermaid-classifier     (needs pandas, scikit-learn, matplotlib)

The reference's metrics package imports ``spacer.data_classes``, ``mlflow`` and ``duckdb`` at module level; none of them is used by
the three functions, so stand-in modules go into ``sys.modules`` first (a ``ValResults`` dataclass and attribute-answering dummies).

Data: 300 images of 1-40 points (about 6 000 rows), 9 classes ``b<i>::`` / ``b<i>::g`` whose top-level ancestor is ``t<i // 3>``
(class 7 never occurs in gt, class 8 neither in gt nor in est), 4 sources, fp32 scores in [0.2, 1] of which about 5 % are exactly 1.0
on correct rows (a tie group across bin edges), ``n_bins`` 20 and 7.  The file holds data only: the inputs and what the reference
returned.  The generator asserts the conditions under which the reference is well defined, so the tests need no escape hatch:
  - no equal-score group of mixed correctness straddles a bin edge (np.argsort leaves that order open);
  - no per-source value lies within 1e-9 of a 4-decimal rounding boundary;
  - every class with max t > min t has sum (t - mean t)^2 >= 1e-3 (R^2 is well conditioned)."""

import dataclasses
import sys
import types
import warnings
from pathlib import Path

import numpy as np

K, N_IMAGES, N_SOURCES = 9, 300, 4


class _Dummy(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


@dataclasses.dataclass
class ValResults:
    scores: list
    gt: list
    est: list
    classes: list


def _stand_ins():
    for name in ("mlflow", "duckdb", "spacer", "spacer.data_classes"):
        sys.modules.setdefault(name, _Dummy(name))
    sys.modules["spacer.data_classes"].ValResults = ValResults


class _Labels(dict):
    """dataset.labels.val: feature location -> the image's point annotations."""


class _Library:
    def bagf_id_to_name(self, bagf_id, gf_library):
        return "name of " + bagf_id


def make_inputs():
    rng = np.random.default_rng(20240611)
    sizes = rng.integers(1, 41, N_IMAGES)
    n = int(sizes.sum())
    source = rng.choice(N_SOURCES, N_IMAGES, p=[0.5, 0.25, 0.15, 0.1])
    gt = rng.choice(7, n, p=[0.3, 0.25, 0.2, 0.1, 0.08, 0.05, 0.02])
    est = np.where(rng.random(n) < 0.7, gt, rng.integers(0, 8, n))
    scores = rng.uniform(0.2, 1.0, n).astype(np.float32)
    scores[(rng.random(n) < 0.05) & (est == gt)] = 1.0
    scores[est != gt] = np.minimum(scores[est != gt], np.float32(0.999))
    return sizes.astype(np.int64), source.astype(np.int32), gt.astype(np.int32), est.astype(np.int32), scores


def main(reference_root):
    _stand_ins()
    sys.path.insert(0, str(reference_root))
    import matplotlib
    matplotlib.use("Agg")
    from sklearn.metrics import accuracy_score, balanced_accuracy_score, precision_recall_fscore_support

    from mermaid_classifier.pyspacer.metrics._context import MetricsContext
    from mermaid_classifier.pyspacer.metrics.calibration import _adaptive_ece
    from mermaid_classifier.pyspacer.metrics.cover import compute_cover
    from mermaid_classifier.pyspacer.metrics.per_source import compute_per_source

    sizes, source, gt, est, scores = make_inputs()
    n = len(gt)
    classes = [f"b{i}::" if i % 2 else f"b{i}::g" for i in range(K)]
    top = np.arange(K) // 3
    ba_paths = {f"b{i}": [f"t{top[i]}", f"b{i}"] for i in range(K)}
    source_keys = [f"site{s % 2}:{100 + s}" for s in range(N_SOURCES)]
    labels = _Labels()
    loc_source = {}
    for i, m in enumerate(sizes.tolist()):
        loc = f"img{i:04d}"
        labels[loc] = [None] * m
        loc_source[loc] = tuple(source_keys[source[i]].split(":"))
    dataset = types.SimpleNamespace(labels=types.SimpleNamespace(val=labels), feature_loc_to_source=loc_source)
    ctx = MetricsContext(val_results=ValResults(scores=scores.astype(np.float64).tolist(), gt=gt.tolist(), est=est.tolist(), classes=classes),
                         ba_library=_Library(), gf_library=None, format_func=float, dataset=dataset, ba_paths=ba_paths)
    out = dict(image_sizes=sizes, source_of_image=source, gt=gt, est=est, scores=scores, classes=np.array(classes),
               top_of_class=top.astype(np.int32), source_keys=np.array(source_keys))

    # ---- reliability ----
    order = np.lexsort((est == gt, scores))
    s_sorted, c_sorted = scores[order], (est == gt)[order]
    for nb in (20, 7):
        assert np.array_equal(np.linspace(0, n, nb + 1, dtype=int), np.arange(nb + 1) * n // nb)
        for e in np.linspace(0, n, nb + 1, dtype=int)[1:-1]:
            if s_sorted[e - 1] == s_sorted[e]:
                grp = c_sorted[s_sorted == s_sorted[e]]
                assert grp.all() or not grp.any(), f"n_bins {nb}: a mixed tie group straddles position {e}"
        ece, bins = _adaptive_ece(ctx.val_results.scores, gt, est, n_bins=nb)
        out[f"ece{nb}"] = np.float64(ece)
        for k in ("avg_confidence", "avg_accuracy", "count", "conf_min", "conf_max"):
            out[f"bins{nb}_{k}"] = np.array([b[k] for b in bins])

    # ---- cover ----
    res = compute_cover(ctx)
    df = res.dataframes[0].df
    out["cover_class"] = np.array([classes.index(c) for c in df["bagf_id"]], np.int32)
    for k in ("mean_true_cover_pct", "bias_pct", "rmse_pct", "mae_pct", "r_squared"):
        out[f"cover_{k}"] = df[k].to_numpy(np.float64)
    for s in res.scalars:
        out[f"scalar_{s.name}"] = np.float64(s.value)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    t = np.stack([np.bincount(gt[a:b], minlength=K) / (b - a) for a, b in zip(offs[:-1], offs[1:])])
    for c in range(K):
        if t[:, c].max() > t[:, c].min():
            assert ((t[:, c] - t[:, c].mean()) ** 2).sum() >= 1e-3, c
    assert len(set(np.round(df["mean_true_cover_pct"], 9))) == len(df), "equal mean covers: the table order would be open"

    # ---- per source ----
    res = compute_per_source(ctx)
    df = res.dataframes[0].df
    out["source_index"] = np.array([source_keys.index(k) for k in df["source_key"]], np.int32)
    for k in ("num_val_images", "num_val_annotations"):
        out[f"source_{k}"] = df[k].to_numpy(np.int64)
    for k in ("accuracy", "balanced_accuracy", "f1_macro", "precision_macro", "recall_macro", "cross_branch_error_rate"):
        out[f"source_{k}"] = df[k].to_numpy(np.float64)
    assert len(set(df["num_val_annotations"])) == len(df), "equal annotation counts: the table order would be open"
    for s in res.scalars:
        out["scalar_" + s.name.replace("/", "_")] = np.float64(s.value)
    row_source = np.repeat(source, sizes)
    for s in range(N_SOURCES):
        g, e = gt[row_source == s], est[row_source == s]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            p, r, f, _ = precision_recall_fscore_support(g, e, average="macro", zero_division=0)
            vals = [accuracy_score(g, e), balanced_accuracy_score(g, e), p, r, f]
        wrong = g != e
        vals.append((top[g[wrong]] != top[e[wrong]]).mean())
        for v in vals:
            frac = (float(v) * 1e4) % 1.0
            assert abs(frac - 0.5) > 1e-5, f"source {s}: {v} lies on a rounding boundary"

    path = Path(__file__).resolve().parent / "metrics_fixture.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes;", n, "rows")


if __name__ == "__main__":
    main(Path(sys.argv[1]))
