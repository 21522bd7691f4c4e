"""Head ensembles without a GPU: the numpy definition's own properties (tests/ensemble_checker.py), the host-side pieces of
mermaid_classifier_amd.ensemble (risk-coverage, the selection from a sweep's ranking, every argument and manifest error that must
surface before a device call), and one float64 evidence recipe whose measured values the README entry quotes."""

import json

import numpy as np
import pytest

import ensemble_checker as ec


def random_rows(rng, M, rows, K, sharp=3.0):
    z = rng.normal(0, sharp, (M, rows, K))
    p = np.exp(z - z.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)).astype(np.float32)


# ---- the checker ----

def test_one_member_one_view_is_the_identity():
    rng = np.random.default_rng(0)
    v = random_rows(rng, 1, 12, 9)
    d = ec.definition(v, 1, 4)
    assert np.array_equal(d["e"].view(np.uint32), v[0].view(np.uint32)) and np.array_equal(d["m"][0].view(np.uint32), v[0].view(np.uint32))
    assert np.array_equal(d["votes"], np.ones(12, np.int32)) and np.all(d["stats"][:, 2] == 0)
    order = np.argsort(-v[0].astype(np.float64), axis=1, kind="stable")[:, :4]
    assert np.array_equal(d["idx"], order)


def test_views_and_members_are_summed_left_to_right_in_float32():
    v = np.array([[[1e-8, 1.0, 0.0]], [[1.0, 1e-8, 0.0]], [[1e-8, 1e-8, 1.0]]], np.float32)      # M = 3, one row
    e = ec.ensemble_mean(ec.member_means(v, 1))
    f = np.float32
    assert e[0, 0] == (f(f(f(1e-8) + f(1.0)) + f(1e-8)) / f(3)) and e[0, 1] == (f(f(f(1.0) + f(1e-8)) + f(1e-8)) / f(3))
    g = ec.member_means(np.array([[[0.25, 0.75], [0.5, 0.5], [0.125, 0.875]]], np.float32), 3)    # one member, G = 3
    assert g.shape == (1, 1, 2) and g[0, 0, 0] == f(f(f(0.25) + f(0.5)) + f(0.125)) / f(3)


def test_ties_keep_class_order_and_votes_count_first_maxima():
    v = np.array([[[0.4, 0.4, 0.2]], [[0.2, 0.4, 0.4]]], np.float32)
    d = ec.definition(v, 1, 3)
    assert d["idx"].tolist() == [[1, 0, 2]]                      # e = (0.3, 0.4, 0.3): class 1, then the tie in class order
    assert d["votes"].tolist() == [1]                            # member 0's first maximum is class 0, member 1's is class 1
    assert ec.entropy(np.array([0.5, 0.5, 0.0])) == pytest.approx(np.log(2))
    assert np.isnan(ec.entropy(np.array([np.nan, 0.5])))


@pytest.mark.parametrize("M,G,K", [(2, 1, 3), (5, 3, 7), (16, 2, 108)])
def test_jensen_entropy_and_log_loss(M, G, K):
    """H(e) >= mean_j H(m_j) and -log e_y <= mean_j -log m_{j,y}, row by row, within what float32 rounding of e can take."""
    rng = np.random.default_rng(M * 100 + K)
    v = random_rows(rng, M, 40 * G, K)
    d = ec.definition(v, G, 1)
    slack = ec.jensen_slack(K, M) + ec.stats_bound(d["stats"], K, M)[:, 2]
    assert np.all(d["stats"][:, 2] >= -slack)
    y = rng.integers(0, K, 40)
    rows = np.arange(40)
    nll_e = -np.log(d["e"][rows, y].astype(np.float64))
    nll_m = np.mean([-np.log(d["m"][j][rows, y].astype(np.float64)) for j in range(M)], axis=0)
    assert np.all(nll_e <= nll_m + (M + 1) * 2.0 ** -23)
    assert np.all(ec.stats_bound(d["stats"], K, M) < 1e-6) and np.all(d["votes"] >= 0) and np.all(d["votes"] <= M)


# ---- risk-coverage ----

def test_risk_coverage_on_hand_made_rows_with_ties():
    from mermaid_classifier_amd.ensemble import risk_coverage
    correct = np.array([1, 0, 1, 1, 0, 1, 0, 1])
    unc = np.array([0.1, 0.9, 0.1, 0.5, 0.5, 0.1, 0.9, 0.5])
    # stable order by uncertainty: rows 0, 2, 5 | 3, 4, 7 | 1, 6  ->  correct 1 1 1 | 1 0 1 | 0 0
    rc = risk_coverage(correct, unc, [0.25, 0.5, 0.625, 1.0])
    assert rc["accuracy"].tolist() == [1.0, 1.0, 4 / 5, 5 / 8]
    assert rc["aurc"] == pytest.approx(0.25 * 1.0 + 0.125 * 0.9 + 0.375 * (0.8 + 0.625) / 2)
    assert np.array_equal(rc["accuracy"], ec.risk_coverage(correct, unc, [0.25, 0.5, 0.625, 1.0]))
    # ties go by row: with equal uncertainty everywhere the kept rows are the first ones
    assert risk_coverage(correct, np.zeros(8), [0.25, 0.5])["accuracy"].tolist() == [0.5, 0.75]
    assert risk_coverage(correct, unc, [0.01])["accuracy"].tolist() == [1.0]        # at least one row is kept
    for bad in ([], [0.0, 0.5], [0.5, 0.5], [0.5, 1.5]):
        with pytest.raises(ValueError):
            risk_coverage(correct, unc, bad)
    with pytest.raises(ValueError):
        risk_coverage(correct, unc[:3], [0.5])


def test_ensemble_validation_risk_coverage_skips_unscored_rows():
    from mermaid_classifier_amd.ensemble import EnsembleValidation, Uncertainty
    from mermaid_classifier_amd.validation import Validation
    gt = np.array([0, 1, -1, 1, 0], np.int32)
    est = np.array([0, 0, 1, 1, 1], np.int32)
    conf = np.array([[1, 1], [1, 1]])
    v = Validation(["a", "b"], gt, est, [0.9, 0.6, 0.7, 0.8, 0.55], [1, 2, 0, 1, 2], [0.9, 0.4, 0.0, 0.8, 0.45], conf, [2, 2], 5, 2, 1, 0, 0)
    u = Uncertainty(np.array([0.2, 0.6, 0.1, 0.3, 0.7], np.float32), np.zeros(5, np.float32), np.array([0.0, 0.3, 0.0, 0.1, 0.2], np.float32),
                    np.array([3, 2, 3, 3, 1], np.int32))
    ev = EnsembleValidation(v, u, [])
    assert ev.risk_coverage("entropy", [0.5, 1.0])["accuracy"].tolist() == [1.0, 0.5]       # rows 0, 3 | 1, 4; row 2 is unknown
    assert ev.risk_coverage("score", [0.5, 1.0])["accuracy"].tolist() == [1.0, 0.5]
    assert ev.risk_coverage("votes", [0.25, 1.0])["accuracy"].tolist() == [1.0, 0.5]
    assert ev.risk_coverage("mutual_information", [0.75])["accuracy"].tolist() == [2 / 3]   # rows 0, 3, 4
    with pytest.raises(ValueError, match="by must be"):
        ev.risk_coverage("margin")
    with pytest.raises(ValueError, match="rows=True"):
        EnsembleValidation(Validation(["a", "b"], None, None, None, None, None, conf, [2, 2], 5, 2, 1, 0, 0), None, []).risk_coverage()


# ---- from_sweep's selection ----

def test_selection_from_ranking_rows():
    from mermaid_classifier_amd.ensemble import select_from_ranking
    ranking = [{"config": 4, "balanced_accuracy": 0.9}, {"config": 0, "balanced_accuracy": 0.8}, {"config": 2, "balanced_accuracy": 0.8},
               {"config": 1, "balanced_accuracy": 0.1}]
    assert select_from_ranking(ranking, 1) == [4] and select_from_ranking(ranking, 3) == [4, 0, 2]
    for bad in (0, 5, 17, 1.5, True):
        with pytest.raises(ValueError):
            select_from_ranking(ranking, bad)


# ---- errors before any device call ----

def _member(K=4, dim=6, classes=None, seed=0):
    from mermaid_classifier_amd import CalibratedMLP
    rng = np.random.default_rng(seed)
    return CalibratedMLP([rng.normal(0, 1, (K, dim)).astype(np.float32)], [np.zeros(K, np.float32)],
                         [f"c{i}" for i in range(K)] if classes is None else classes, -np.ones(K), np.zeros(K))


def test_head_ensemble_argument_errors_name_the_first_difference():
    from mermaid_classifier_amd import HeadEnsemble
    a = _member()
    ens = HeadEnsemble([a, _member(seed=1)])
    assert len(ens) == 2 and ens.classes == ["c0", "c1", "c2", "c3"] and ens.input_dim == 6 and ens._h is None and ens.ranking is None
    with pytest.raises(ValueError, match="1 .. 16 members"):
        HeadEnsemble([])
    with pytest.raises(ValueError, match="1 .. 16 members"):
        HeadEnsemble([a] * 17)
    with pytest.raises(ValueError, match="member 1 must be a CalibratedMLP or a Predictor"):
        HeadEnsemble([a, object()])
    with pytest.raises(ValueError, match="member 1 has 5 classes, member 0 has 4"):
        HeadEnsemble([a, _member(K=5)])
    with pytest.raises(ValueError, match="member 2's class 1 is 'c2', member 0's is 'c1'"):
        HeadEnsemble([a, a, _member(classes=["c0", "c2", "c1", "c3"])])
    with pytest.raises(ValueError, match="member 1 takes 7 features, member 0 takes 6"):
        HeadEnsemble([a, _member(dim=7)])
    with pytest.raises(ValueError, match="k = 5"):
        ens.topk(np.zeros((2, 6), np.float32), 5)
    with pytest.raises(ValueError, match=r"\(N, 6\)"):
        ens.predict_proba(np.zeros((2, 5), np.float32))
    assert ens._h is None                                              # nothing above made a device handle
    from mermaid_classifier_amd import ensemble_validate, export_ensemble
    with pytest.raises(ValueError, match="HeadEnsemble"):
        ensemble_validate(a, (np.zeros((2, 6), np.float32), ["c0", "c1"]))
    with pytest.raises(ValueError, match="X has 5 features"):
        ensemble_validate(ens, (np.zeros((2, 5), np.float32), ["c0", "c1"]))
    with pytest.raises(ValueError, match="not in the model's classes"):
        ensemble_validate(ens, (np.zeros((2, 6), np.float32), ["c0", "zz"]))
    with pytest.raises(ValueError, match="HeadEnsemble"):
        export_ensemble(a, "unused", np.zeros((2, 6), np.float32))
    assert ens._h is None


def _write_dir(tmp_path, manifest, members):
    d = tmp_path / "ens"
    d.mkdir(parents=True)
    if manifest is not None:
        (d / "ensemble.json").write_text(json.dumps(manifest))
    for name, mj in members.items():
        (d / name).mkdir()
        (d / name / "model.pt").write_bytes(b"not a graph: the manifest checks must fail first")
        (d / name / "model.json").write_text(json.dumps(mj))
    return d


def test_load_ensemble_checks_the_manifest_before_anything_is_loaded(tmp_path, monkeypatch):
    from mermaid_classifier_amd import ManifestError, load_ensemble
    from mermaid_classifier_amd import ensemble as E

    def no_load(*a, **k):
        raise AssertionError("load_predictor was reached")
    monkeypatch.setattr(E, "load_predictor", no_load)
    classes = ["a", "b", "c"]
    good = {"classes": classes, "input_dim": 6}
    cases = [
        (None, {}, "not found"),
        ({"format_version": 2, "members": ["member_00"], "classes": classes, "input_dim": 6}, {"member_00": good}, "format_version=2"),
        ({"format_version": 1, "members": [], "classes": classes, "input_dim": 6}, {}, "0 members"),
        ({"format_version": 1, "members": ["member_00", "member_01"], "classes": classes, "input_dim": 6}, {"member_00": good}, "member 'member_01'.*missing"),
        ({"format_version": 1, "members": ["member_00", "member_01"], "classes": classes, "input_dim": 6},
         {"member_00": good, "member_01": {"classes": ["a", "c", "b"], "input_dim": 6}}, "member 'member_01': its class list differs"),
        ({"format_version": 1, "members": ["member_00"], "classes": classes, "input_dim": 6}, {"member_00": {"classes": classes, "input_dim": 8}},
         "input_dim 8 differs"),
    ]
    for i, (manifest, members, match) in enumerate(cases):
        d = _write_dir(tmp_path / str(i), manifest, members)
        with pytest.raises(ManifestError, match=match):
            load_ensemble(d)
    ok = _write_dir(tmp_path / "ok", {"format_version": 1, "members": ["member_00"], "classes": classes, "input_dim": 6}, {"member_00": good})
    assert E.check_ensemble_dir(ok)["members"] == ["member_00"]
    with pytest.raises(AssertionError, match="load_predictor was reached"):      # only a clean manifest gets as far as loading
        load_ensemble(ok)


def test_point_predictions_fields_are_none_for_a_single_head():
    from mermaid_classifier_amd import PointPredictions
    p = PointPredictions(None, np.zeros((2, 1), np.int32), np.ones((2, 1)), ["a", "b"])
    assert p.entropy is None and p.mutual_information is None and p.votes is None
    q = PointPredictions(None, np.zeros((2, 1), np.int32), np.ones((2, 1)), ["a", "b"], np.array([[0.5, 0.4, 0.1], [0.2, 0.25, -1e-9]], np.float32), [3, 2])
    assert q.entropy.tolist() == [0.5, np.float32(0.2)] and q.mutual_information.tolist() == [np.float32(0.1), 0.0] and q.votes.tolist() == [3, 2]
    with pytest.raises(ValueError, match="do not fit"):
        PointPredictions(None, np.zeros((2, 1), np.int32), np.ones((2, 1)), ["a", "b"], np.zeros((3, 3), np.float32), [1, 1, 1])


# ---- evidence ----

def test_five_seed_ensemble_of_the_float64_recipe():
    """Five seeds of one 12 -> 24 -> 5 head trained by oracle/mlp_train_ref.py (20 passes over 600 rows of five Gaussian classes
    with 25 % of the training labels replaced at random), scored on 1000 clean held-out rows, all ensemble arithmetic in float64.
    Asserted: only what Jensen guarantees (ensemble log-loss <= mean member log-loss; H(e) >= mean member entropy per row).
    Printed, in favour or not (the README entry quotes them): accuracy and log-loss of the ensemble against the mean and the best
    member, and accuracy on the 80 % least-uncertain rows (by predictive entropy) against all rows."""
    from oracle.mlp_train_ref import MLPTrainRef
    rng = np.random.default_rng(2024)
    K, dim, n_train, n_test = 5, 12, 600, 1000
    centres = rng.normal(0, 1.0, (K, dim))

    def draw(n):
        y = rng.integers(0, K, n)
        return (centres[y] + rng.normal(0, 1.2, (n, dim))).astype(np.float32), y
    Xtr, ytr = draw(n_train)
    Xte, yte = draw(n_test)
    noisy = ytr.copy()
    flip = rng.random(n_train) < 0.25
    noisy[flip] = rng.integers(0, K, int(flip.sum()))
    probs = []
    for seed in range(5):
        r = np.random.default_rng(100 + seed)
        dims = (dim, 24, K)
        W = [r.uniform(-1, 1, (dims[i + 1], dims[i])).astype(np.float32) * np.float32(np.sqrt(6.0 / (dims[i] + dims[i + 1]))) for i in range(2)]
        b = [np.zeros(dims[i + 1], np.float32) for i in range(2)]
        net = MLPTrainRef(W, b, lr=3e-3)
        for epoch in range(20):
            net.partial_fit(Xtr, noisy, 100, random_state=seed * 1000 + epoch)
        probs.append(net.predict_proba(Xte))
    probs = np.stack(probs)                                       # (5, n, K) float64
    e = probs.mean(0)
    rows = np.arange(n_test)
    acc_m = [(p.argmax(1) == yte).mean() for p in probs]
    nll_m = [-np.log(np.clip(p[rows, yte], 1e-15, 1)).mean() for p in probs]
    acc_e, nll_e = (e.argmax(1) == yte).mean(), -np.log(np.clip(e[rows, yte], 1e-15, 1)).mean()
    h_e, h_m = ec.entropy(e), np.mean([ec.entropy(p) for p in probs], axis=0)
    kept = np.argsort(h_e, kind="stable")[: int(0.8 * n_test)]
    acc_kept = (e.argmax(1) == yte)[kept].mean()
    print(f"ensemble evidence: accuracy ensemble {acc_e:.4f}, mean member {np.mean(acc_m):.4f}, best member {np.max(acc_m):.4f}; "
          f"log-loss ensemble {nll_e:.4f}, mean member {np.mean(nll_m):.4f}, best member {np.min(nll_m):.4f}; "
          f"accuracy on the 80% least-uncertain rows {acc_kept:.4f} against {acc_e:.4f} on all; "
          f"mean mutual information {np.mean(h_e - h_m):.4f} nats")
    assert nll_e <= np.mean(nll_m) + 1e-12
    assert np.all(h_e >= h_m - 1e-12)
