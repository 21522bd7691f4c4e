"""Generate tests/golden/ranking_fixture.npz: the reference's own ``compute_ranking`` (metrics/ranking.py) and
``taxonomic_similarity`` (metrics/_taxonomy_helpers.py) on seeded validation probabilities.

    python tests/golden/make_ranking_golden.py /path/to/mermaid-classifier     (needs pandas, scikit-learn, matplotlib)

The reference's metrics package imports ``spacer.data_classes``, ``mlflow`` and ``duckdb`` at module level; none of them is used by
the two functions, so stand-in modules go into ``sys.modules`` first (as in make_metrics_golden.py).  The taxonomy is a small fake
``ba_library`` with what ``build_ba_to_top`` / ``build_ba_paths`` / ``taxonomic_similarity`` / ``group_by_top_level`` call:
``get_ancestor_ids`` and ``id_to_name``.

Data: 3 000 rows, 12 classes ``b<i>::`` / ``b<i>::g`` under four top-level categories ``t0 .. t3`` in a tree of depth 3:

    t0 - m0 - b0, b1      t1 - m1 - b3, b4      t2 - m2 - b7, b8      t3 - b10, b11
       - b2                  - b5, b6              - b9

so the similarities are 1 (same class), 2/3 (b0 / b1), 1/2 (b5 / b6), 1/3 (b0 / b2) and 0 (different categories).  Category t3 holds
fewer than 30 rows (the ``min_samples`` rule).  The probabilities are fp32 softmax rows that favour the true class, then its category.
The file holds data only: the inputs and what the reference returned.  The generator asserts the conditions under which the
reference is well defined, so the tests need no escape hatch:
  - no two equal probabilities among a row's eleven largest (np.argsort(-proba) leaves ties open);
  - no equal ``top_1`` between two categories (the table order would be open);
  - no similarity value within 1e-9 of a threshold without being equal to it."""

import sys
import types
from pathlib import Path

import numpy as np

from make_metrics_golden import ValResults, _stand_ins

K, N = 12, 3000
PARENT = {"m0": "t0", "m1": "t1", "m2": "t2",
          "b0": "m0", "b1": "m0", "b2": "t0",
          "b3": "m1", "b4": "m1", "b5": "t1", "b6": "t1",
          "b7": "m2", "b8": "m2", "b9": "t2",
          "b10": "t3", "b11": "t3"}
TOPS = ["t0", "t1", "t2", "t3"]


class _Library:
    def get_ancestor_ids(self, ba_id):
        """root first, without ``ba_id`` itself"""
        out = []
        while ba_id in PARENT:
            ba_id = PARENT[ba_id]
            out.append(ba_id)
        return out[::-1]

    def id_to_name(self, ba_id):
        return "name of " + ba_id

    def bagf_id_to_name(self, bagf_id, gf_library):
        return "name of " + bagf_id


def make_inputs(category_of_class):
    rng = np.random.default_rng(20240917)
    p_class = np.array([0.16, 0.12, 0.08, 0.14, 0.1, 0.07, 0.06, 0.1, 0.09, 0.072, 0.005, 0.003])
    gt = rng.choice(K, N, p=p_class / p_class.sum())
    logits = rng.normal(0.0, 1.5, (N, K))
    logits += 1.2 * (category_of_class[None, :] == category_of_class[gt][:, None])
    logits[np.arange(N), gt] += rng.normal(1.0, 1.5, N)
    e = np.exp(logits - logits.max(1, keepdims=True))
    proba = (e / e.sum(1, keepdims=True)).astype(np.float32)
    return gt.astype(np.int32), proba


def main(reference_root):
    _stand_ins()
    sys.path.insert(0, str(reference_root))
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    from mermaid_classifier.pyspacer.metrics._context import MetricsContext
    from mermaid_classifier.pyspacer.metrics._taxonomy_helpers import build_ba_paths, taxonomic_similarity
    from mermaid_classifier.pyspacer.metrics.ranking import compute_ranking

    lib = _Library()
    classes = [f"b{i}::" if i % 2 else f"b{i}::g" for i in range(K)]
    ba = [f"b{i}" for i in range(K)]
    category_of_class = np.array([TOPS.index((lib.get_ancestor_ids(b) + [b])[0]) for b in ba], np.int32)
    gt, proba = make_inputs(category_of_class)

    ba_paths = build_ba_paths(classes, lib)
    assert max(len(p) for p in ba_paths.values()) == 3
    similarity = np.array([[taxonomic_similarity(a, b, ba_paths, lib) for b in ba] for a in ba], np.float64)
    assert sorted(set(similarity.ravel().tolist())) == [0.0, 1 / 3, 1 / 2, 2 / 3, 1.0]
    for v in set(similarity.ravel().tolist()):
        for t in (1.0, 0.75, 0.5):
            assert v == t or abs(v - t) > 1e-9, (v, t)
    assert np.allclose(proba.sum(1), 1.0, atol=1e-6)
    top11 = -np.sort(-proba, axis=1)[:, :11]
    assert (top11[:, :-1] > top11[:, 1:]).all(), "equal probabilities among a row's eleven largest"
    per_cat = np.bincount(category_of_class[gt], minlength=len(TOPS))
    assert 0 < per_cat[3] < 30 and (per_cat[:3] >= 30).all(), per_cat

    ctx = MetricsContext(val_results=ValResults(scores=[], gt=gt.tolist(), est=proba.argmax(1).tolist(), classes=classes),
                         ba_library=lib, gf_library=None, format_func=float, clf=types.SimpleNamespace(classes_=np.array(classes)),
                         val_proba=proba, val_gt_labels=[classes[g] for g in gt])
    res = compute_ranking(ctx)
    plt.close("all")
    out = dict(proba=proba, gt=gt, classes=np.array(classes), category_of_class=category_of_class, similarity=similarity)
    cat, hier = res.dataframes
    assert cat.artifact_path == "ranking/per_category_topk" and hier.artifact_path == "ranking/hierarchical_topk"
    cat, hier = cat.df, hier.df
    assert len(set(cat["top_1"])) == len(cat) == 3, "equal top_1 between two categories: the table order would be open"
    out["cat_category"] = np.array([TOPS.index(name[len("name of "):]) for name in cat["category"]], np.int32)
    out["cat_n_samples"] = cat["n_samples"].to_numpy(np.int64)
    for k in ("mrr", "top_1", "top_3", "top_5", "top_10"):
        out[f"cat_{k}"] = cat[k].to_numpy(np.float64)
    out["hier_k"] = hier["k"].to_numpy(np.int64)
    for k in ("mean_max_similarity", "hit_exact", "hit_sibling_0.75", "hit_family_0.5"):
        out[f"hier_{k}"] = hier[k].to_numpy(np.float64)
    for s in res.scalars:
        out[f"scalar_{s.name}"] = np.float64(s.value)

    path = Path(__file__).resolve().parent / "ranking_fixture.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes;", N, "rows;", per_cat.tolist(), "rows per category")


if __name__ == "__main__":
    main(Path(sys.argv[1]))
