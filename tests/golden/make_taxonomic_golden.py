"""Generate tests/golden/taxonomic_fixture.npz: the reference's own ``compute_taxonomic`` (metrics/taxonomic.py) and
``compute_calibration`` (metrics/calibration.py, for its per-category ECE table) on seeded validation results.

    python tests/golden/make_taxonomic_golden.py /path/to/mermaid-classifier     (needs pandas, scikit-learn, matplotlib)

The reference's metrics package imports ``spacer.data_classes``, ``mlflow`` and ``duckdb`` at module level; none of them is used by
the two functions, so stand-in modules go into ``sys.modules`` first (as in make_metrics_golden.py).  The taxonomy is a small fake
``ba_library`` / ``gf_library`` with what the two functions call: ``get_ancestor_ids``, ``get_descendants``, ``id_to_name``, and
``id_to_name`` on the growth-form library.

Data: 4 000 rows, 15 classes ``b<i>::`` / ``b<i>::g<j>`` under six top-level categories in the depth-3 tree of
make_ranking_golden.py, extended:

    t0 - m0 - b0 (g0, g1), b1 (g0)    t1 - m1 - b3 (g1), b4 (g2)    t2 - m2 - b7 (g2), b8 (-)    t3 - b10 (g1), b11 (-)
       - b2 (-)                          - b5 (-, g0)                  - b9 (g3)                 t4 - b12 (g3)      t5 - b13 (g4)

Rows per true category: t0 2 200, t1 1 643, t2 100 (of which exactly 29 are predicted into t0: 29 / 100 * 100 is
28.999999999999996 in float64, so the reference's percent is 28), t3 35 (3 bins), t4 22 (below ``min_samples``), t5 none: its
class ``b13::g4`` is only ever predicted.  The file holds data only: the inputs and what the reference returned, data frames as
arrays of columns, the two percent matrices as the reference drew them (read back from the figures' image arrays and tick
labels).  Ids are stored as indices: LCA nodes into ``nodes``, categories into ``tops``, growth forms into ``gfs``; -1 stands
for the cross-branch row and for "(no GF)".  The generator asserts the conditions under which the reference is well defined, so the
tests need no escape hatch:
  - inside each category all scores are distinct (np.argsort leaves the order of equal scores open);
  - no two categories have equal ``ece``, no two top-level categories equal true frequency, no two growth forms equal support;
  - growth-form names are unique;
  - a top-level confusion cell hits the float floor; a category has fewer than 30 rows, one has 30-39;
  - a class has no growth form, a class is predicted only, and some errors are between two classes of one benthic attribute."""

import sys
from pathlib import Path

import numpy as np

from make_metrics_golden import ValResults, _stand_ins

PARENT = {"m0": "t0", "m1": "t1", "m2": "t2",
          "b0": "m0", "b1": "m0", "b2": "t0",
          "b3": "m1", "b4": "m1", "b5": "t1",
          "b7": "m2", "b8": "m2", "b9": "t2",
          "b10": "t3", "b11": "t3", "b12": "t4", "b13": "t5"}
CLASSES = ["b0::g0", "b0::g1", "b1::g0", "b2::", "b3::g1", "b4::g2", "b5::", "b5::g0", "b7::g2", "b8::", "b9::g3", "b10::g1", "b11::",
           "b12::g3", "b13::g4"]
TOPS = ["t0", "t1", "t2", "t3", "t4", "t5"]
GFS = ["g0", "g1", "g2", "g3", "g4"]
NODES = sorted(set(PARENT) | set(PARENT.values()))
ROWS_PER_TOP = [2200, 1643, 100, 35, 22, 0]
K = len(CLASSES)


class _Library:
    def get_ancestor_ids(self, ba_id):
        """root first, without ``ba_id`` itself"""
        out = []
        while ba_id in PARENT:
            ba_id = PARENT[ba_id]
            out.append(ba_id)
        return out[::-1]

    def get_descendants(self, ba_id):
        return [{"id": n} for n in NODES if ba_id in self.get_ancestor_ids(n)]

    def id_to_name(self, ba_id):
        return "name of " + ba_id

    def bagf_id_to_name(self, bagf_id, gf_library):
        return "name of " + bagf_id


class _GrowthForms:
    def id_to_name(self, gf_id):
        return "gf name of " + gf_id


def _unname(name, prefix="name of "):
    assert name.startswith(prefix), name
    return name[len(prefix):]


def make_inputs(top_of_class, ba_of_class):
    rng = np.random.default_rng(20241019)
    gt = []
    for t, m in enumerate(ROWS_PER_TOP):
        members = np.flatnonzero(top_of_class == t)
        members = members[members != K - 1]
        if m:
            gt.append(rng.choice(members, m, p=rng.dirichlet(np.full(len(members), 4.0))))
    gt = rng.permutation(np.concatenate(gt))
    n = len(gt)
    est = gt.copy()
    for i in np.flatnonzero(rng.random(n) > 0.62):
        g, u = gt[i], rng.random()
        same_ba = np.flatnonzero((ba_of_class == ba_of_class[g]) & (np.arange(K) != g))
        same_top = np.flatnonzero((top_of_class == top_of_class[g]) & (np.arange(K) != g))
        if u < 0.25 and len(same_ba):
            est[i] = rng.choice(same_ba)
        elif u < 0.7 and len(same_top):
            est[i] = rng.choice(same_top)
        elif u < 0.76:
            est[i] = K - 1
        else:
            est[i] = rng.choice(np.flatnonzero(top_of_class != top_of_class[g]))
    # category t2: exactly 29 of its 100 rows are predicted into t0
    rows = np.flatnonzero(top_of_class[gt] == 2)
    assert len(rows) == 100
    into = rows[top_of_class[est[rows]] == 0]
    for i in into[29:]:
        est[i] = gt[i]
    other = rows[top_of_class[est[rows]] != 0]
    for i in other[:max(0, 29 - len(into))]:
        est[i] = 3
    scores = np.where(est == gt, rng.beta(5, 1.6, n), rng.beta(2.2, 2.4, n))
    scores = (0.07 + 0.93 * scores).astype(np.float32)
    return gt.astype(np.int32), est.astype(np.int32), scores


def main(reference_root):
    _stand_ins()
    sys.path.insert(0, str(reference_root))
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    from mermaid_classifier.pyspacer.metrics._context import MetricsContext
    from mermaid_classifier.pyspacer.metrics._taxonomy_helpers import build_ba_paths
    from mermaid_classifier.pyspacer.metrics.calibration import compute_calibration
    from mermaid_classifier.pyspacer.metrics.taxonomic import compute_taxonomic

    lib, gfl = _Library(), _GrowthForms()
    ba = [c.split("::")[0] for c in CLASSES]
    gf = [c.split("::")[1] for c in CLASSES]
    ba_paths = build_ba_paths(CLASSES, lib)
    assert max(len(p) for p in ba_paths.values()) == 3
    top_of_class = np.array([TOPS.index(ba_paths[b][0]) for b in ba], np.int32)
    ba_of_class = np.array([NODES.index(b) for b in ba], np.int32)
    gt, est, scores = make_inputs(top_of_class, ba_of_class)
    n = len(gt)

    # ---- the conditions under which the reference is well defined ----
    per_top = np.bincount(top_of_class[gt], minlength=len(TOPS))
    assert per_top.tolist() == ROWS_PER_TOP and n == 4000
    assert len(set(per_top[per_top > 0].tolist())) == (per_top > 0).sum(), "equal true frequency of two categories"
    assert 0 < per_top[4] < 30 and 30 <= per_top[3] <= 39
    for t in range(len(TOPS)):
        s = scores[top_of_class[gt] == t]
        assert len(np.unique(s)) == len(s), f"equal scores inside category {t}"
    assert K - 1 not in gt and K - 1 in est, "no predicted-only class"
    assert any(g == "" for g in gf) and len(set(gfl.id_to_name(g) for g in GFS)) == len(GFS)
    wrong = gt != est
    assert (ba_of_class[gt[wrong]] == ba_of_class[est[wrong]]).sum() >= 20, "no errors inside one benthic attribute"
    gf_idx = np.array([GFS.index(g) if g else -1 for g in gf], np.int32)
    gf_support = np.bincount(gf_idx[gt][gf_idx[gt] >= 0], minlength=len(GFS))
    assert len(set(gf_support[gf_support > 0].tolist())) == (gf_support > 0).sum(), "equal support of two growth forms"
    top_cm = np.bincount(top_of_class[gt] * len(TOPS) + top_of_class[est], minlength=len(TOPS) ** 2).reshape(len(TOPS), len(TOPS))
    assert top_cm[2, 0] == 29 and top_cm[2].sum() == 100
    rs = np.maximum(top_cm.sum(1, keepdims=True), 1)
    assert (np.floor(top_cm / rs * 100).astype(np.int64) != top_cm * 100 // rs).any(), "no cell hits the float floor"

    ctx = MetricsContext(val_results=ValResults(scores=scores.astype(np.float64).tolist(), gt=gt.tolist(), est=est.tolist(), classes=CLASSES),
                         ba_library=lib, gf_library=gfl, format_func=float)
    out = dict(gt=gt, est=est, scores=scores, classes=np.array(CLASSES), nodes=np.array(NODES), tops=np.array(TOPS), gfs=np.array(GFS),
               top_of_class=top_of_class, gf_of_class=gf_idx)
    depth = max(len(p) for p in ba_paths.values())
    out["class_paths"] = np.array([[NODES.index(x) for x in ba_paths[b]] + [-1] * (depth - len(ba_paths[b])) for b in ba], np.int32)

    # ---- taxonomic ----
    res = compute_taxonomic(ctx)
    for s in res.scalars:
        out[f"scalar_{s.name}"] = np.float64(s.value)
    assert sorted(s.name for s in res.scalars) == ["cross_branch_error_rate", "gf_accuracy_gf_relevant", "within_ba_gf_accuracy",
                                                    "within_branch_error_rate"]
    frames = {d.artifact_path: d.df for d in res.dataframes}
    figures = {f.artifact_path: f.fig for f in res.figures}
    ea = frames["taxonomic/error_attribution"]
    out["ea_lca_node"] = np.array([-1 if v == "(cross-branch)" else NODES.index(v) for v in ea["lca_node"]], np.int32)
    out["ea_branch"] = np.array([-1 if v == "" else NODES.index(_unname(v)) for v in ea["branch"]], np.int32)
    out["ea_error_count"] = ea["error_count"].to_numpy(np.int64)
    out["ea_pct_of_errors"] = ea["pct_of_errors"].to_numpy(np.float64)
    out["ea_classes_in_subtree"] = ea["classes_in_subtree"].to_numpy(np.int64)
    assert -1 in out["ea_lca_node"] and len(ea) >= 6

    tl = frames["taxonomic/top_level_confusions"]
    out["tl_true"] = np.array([TOPS.index(_unname(v)) for v in tl["true"]], np.int32)
    out["tl_predicted"] = np.array([TOPS.index(_unname(v)) for v in tl["predicted"]], np.int32)
    out["tl_row_normalized_pct"] = tl["row_normalized_pct"].to_numpy(np.int64)
    out["tl_sample_count"] = tl["sample_count"].to_numpy(np.int64)
    ax = figures["taxonomic/top_level_confusion.png"].axes[0]
    out["tl_categories"] = np.array([TOPS.index(_unname(t.get_text())) for t in ax.get_yticklabels()], np.int32)
    out["tl_percent"] = np.asarray(ax.images[0].get_array()).astype(np.int64)
    assert out["tl_percent"].shape == (len(TOPS), len(TOPS)) and out["tl_categories"][-1] == 5, "t5 is seen only as a prediction"
    hit = (out["tl_true"] == 2) & (out["tl_predicted"] == 0)
    assert out["tl_row_normalized_pct"][hit].tolist() == [28] and out["tl_sample_count"][hit].tolist() == [29]

    prf = frames["taxonomic/gf_precision_recall_f1"]
    out["gf_growth_form"] = np.array([GFS.index(_unname(v, "gf name of ")) for v in prf["growth_form"]], np.int32)
    for k in ("precision", "recall", "f1"):
        out[f"gf_{k}"] = prf[k].to_numpy(np.float64)
    out["gf_support"] = prf["support"].to_numpy(np.int64)
    ax = figures["taxonomic/gf_confusion.png"].axes[0]
    out["gf_rows"] = np.array([GFS.index(_unname(t.get_text(), "gf name of ")) for t in ax.get_yticklabels()], np.int32)
    out["gf_columns"] = np.array([-1 if t.get_text() == "(no GF)" else GFS.index(_unname(t.get_text(), "gf name of "))
                                  for t in ax.get_xticklabels()], np.int32)
    out["gf_percent"] = np.asarray(ax.images[0].get_array()).astype(np.int64)
    assert out["gf_percent"].shape == (len(out["gf_rows"]), len(out["gf_rows"]) + 1) and 4 not in out["gf_rows"]

    # ---- per-category ECE ----
    res = compute_calibration(ctx)
    frames = {d.artifact_path: d.df for d in res.dataframes}
    pc = frames["calibration/per_category_ece"]
    out["pc_category"] = np.array([TOPS.index(_unname(v)) for v in pc["category"]], np.int32)
    for k in ("ece", "accuracy", "avg_confidence"):
        out[f"pc_{k}"] = pc[k].to_numpy(np.float64)
    out["pc_n_samples"] = pc["n_samples"].to_numpy(np.int64)
    assert sorted(out["pc_category"].tolist()) == [0, 1, 2, 3] and len(set(out["pc_ece"].tolist())) == 4, "equal ece: the order would be open"
    out["scalar_ece"] = np.float64([s.value for s in res.scalars if s.name == "ece"][0])
    plt.close("all")

    path = Path(__file__).resolve().parent / "taxonomic_fixture.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes;", n, "rows;", per_top.tolist(), "rows per category")


if __name__ == "__main__":
    main(Path(sys.argv[1]))
