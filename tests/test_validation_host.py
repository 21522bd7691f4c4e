"""CPU tests of on-device validation (``mmc_head_evaluate*``, ``validation.validate``): the ABI surface, the argument checks that
must fire before a device is touched, ``Validation``'s arithmetic, the label maps of ``previous_accuracies`` -- and the checker
the GPU tests (test_gpu_validation.py) compare the kernel with, itself checked on hand-made rows."""

import numpy as np
import pytest


def check_rows(P, y):
    """What the reference computes per row from (probabilities, true label), restated from metrics/ranking.py:54-65 and
    metrics/probability.py:47-49 with the tie rule made explicit (a STABLE descending sort: equal scores in class order).
    -> dict of est, score, rank (1-based), p_true, n_correct, confusion, rank_hist, nll_q32."""
    P = np.asarray(P)
    y = np.asarray(y, dtype=np.int64)
    n, K = P.shape
    rows = np.arange(n)
    est = P.argmax(1)
    order = np.argsort(-P, axis=1, kind="stable")
    rank = 1 + np.argmax(order == y[:, None], axis=1)
    p_true = P[rows, y]
    nll = -np.log(np.clip(p_true.astype(np.float64), 1e-15, 1.0))
    return dict(est=est.astype(np.int32), score=P[rows, est], rank=rank.astype(np.int32), p_true=p_true,
                n_correct=int((est == y).sum()), confusion=np.bincount(y * K + est, minlength=K * K).reshape(K, K),
                rank_hist=np.bincount(rank - 1, minlength=K), nll_q32=int(np.rint(nll * 2.0 ** 32).astype(np.int64).sum()))


def test_library_and_package_export_the_validation_entry_points():
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    for sym in ("mmc_head_evaluate", "mmc_head_evaluate_set"):
        assert sym in _lib.SYMBOLS and hasattr(lib, sym), sym
    tot = np.zeros(_lib.MMC_EVAL_TOTALS, np.int64)
    assert lib.mmc_head_evaluate(None, None, None, 1, None, 0, None, None, None, None, tot.ctypes.data, None, None, 0, None) == _lib.MMC_ERR_ARG
    assert b"head handle is NULL" in lib.mmc_last_error()
    assert lib.mmc_head_evaluate_set(None, None, 0, 1, None, 0, None, None, None, None, tot.ctypes.data, None, None, None) == _lib.MMC_ERR_ARG
    assert b"head handle is NULL" in lib.mmc_last_error()
    import mermaid_classifier_amd as m
    for name in ("validate", "Validation", "previous_accuracies", "train_and_validate"):
        assert name in m.__all__ and getattr(m, name) is not None, name


class _NoDevice:
    """Stands where a device handle would: any use of it is a test failure."""

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched ({name})")


def _predictor(k_classes=4, input_dim=8):
    from mermaid_classifier_amd.inference import Predictor
    return Predictor(_NoDevice(), [f"c{i}" for i in range(k_classes)], input_dim)


def test_validate_argument_errors_come_before_the_device():
    from mermaid_classifier_amd import FeatureSet, previous_accuracies, validate
    pred = _predictor()
    X = np.zeros((3, 8), np.float32)
    y = ["c0", "c1", "c3"]
    with pytest.raises(ValueError, match="X has 9 features, expected 8"):
        validate(pred, (np.zeros((3, 9), np.float32), y))
    with pytest.raises(ValueError, match="X must be 2D"):
        validate(pred, [(np.zeros((3, 2, 4), np.float32), y)])
    with pytest.raises(ValueError, match=r"y has shape \(2,\), expected \(3,\)"):
        validate(pred, (X, y[:2]))
    with pytest.raises(ValueError, match=r"Labels \['zz'\] are not in the model's classes"):
        validate(pred, (X, ["c0", "zz", "c1"]))
    with pytest.raises(ValueError, match="are not in the model's classes"):          # the second batch, before the first runs
        validate(pred, [(X, y), (X, ["c0", "c9", "c1"])])
    with pytest.raises(ValueError, match="no rows"):
        validate(pred, (np.zeros((0, 8), np.float32), []))
    with pytest.raises(ValueError, match="no rows"):
        validate(pred, [])
    for bad in (1, 0, None, "yes", np.True_):
        with pytest.raises(ValueError, match="rows must be True or False"):
            validate(pred, (X, y), rows=bad)
    with pytest.raises(ValueError, match="must be a CalibratedMLP or a Predictor"):
        validate(object(), (X, y))
    # a feature set that has never been filled has no device handle either
    with pytest.raises(ValueError, match="the feature set has 9 features, expected 8"):
        validate(pred, FeatureSet(9, ["c0", "c1"]))
    with pytest.raises(ValueError, match="no rows"):
        validate(pred, FeatureSet(8, ["c0", "c1"]))
    with pytest.raises(ValueError, match="X has 9 features"):
        previous_accuracies([pred], (np.zeros((3, 9), np.float32), y))
    assert previous_accuracies([], (X, y)) == []


def _hand_made(ranks, K, est=None, gt=None):
    from mermaid_classifier_amd import Validation
    ranks = np.asarray(ranks, np.int32)
    n = len(ranks)
    gt = np.arange(n, dtype=np.int32) % K if gt is None else np.asarray(gt, np.int32)
    est = np.where(ranks == 1, gt, (gt + 1) % K).astype(np.int32) if est is None else np.asarray(est, np.int32)
    scores = 0.5 + np.arange(n) / (4.0 * n)
    p_true = (1.0 / (1.0 + ranks)).astype(np.float32)
    nll = int(np.rint(-np.log(np.clip(p_true.astype(np.float64), 1e-15, 1.0)) * 2.0 ** 32).astype(np.int64).sum())
    return Validation([f"c{i}" for i in range(K)], gt, est, scores, ranks, p_true, np.bincount(gt * K + est, minlength=K * K).reshape(K, K),
                      np.bincount(ranks - 1, minlength=K), n, int((est == gt).sum()), 0, 0, nll)


def test_validation_arithmetic_on_hand_made_integers():
    K = 12
    rng = np.random.default_rng(3)
    ranks = np.concatenate([np.ones(9, np.int32), rng.integers(1, K + 1, 28).astype(np.int32)])
    v = _hand_made(ranks, K)
    assert v.n == 37 and v.n_scored == 37 and v.has_rows
    for k in (1, 3, 5, 10, K + 1, 1000):
        assert v.topk_accuracy(k) == np.mean(ranks <= k), k
    assert v.topk_accuracy(K) == 1.0
    assert v.accuracy == np.mean(ranks == 1) == v.topk_accuracy(1)
    assert v.mrr == pytest.approx(float(np.mean(1.0 / ranks)), rel=1e-14, abs=0)
    assert v.log_loss == v.nll_q32 / (37 << 32)
    assert v.log_loss == pytest.approx(float(np.mean(-np.log(v.p_true.astype(np.float64)))), abs=37 * 2.0 ** -33)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="k must be"):
            v.topk_accuracy(bad)
    # three ragged parts add up to the whole
    parts = [_hand_made(ranks[a:b], K, est=v.est[a:b], gt=v.gt[a:b]) for a, b in ((0, 5), (5, 30), (30, 37))]
    for p, (a, b) in zip(parts, ((0, 5), (5, 30), (30, 37))):
        p.scores = v.scores[a:b]
    m = parts[0].merge(parts[1]).merge(parts[2])
    for name in ("gt", "est", "scores", "ranks", "p_true", "confusion", "rank_hist"):
        assert np.array_equal(getattr(m, name), getattr(v, name)), name
    for name in ("n", "n_correct", "n_unknown", "n_nonfinite", "nll_q32", "classes", "accuracy", "mrr", "log_loss"):
        assert getattr(m, name) == getattr(v, name), name
    # unknown and non-finite rows are misses: they are in n and in no table
    from mermaid_classifier_amd import Validation
    w = Validation(v.classes, None, None, None, None, None, v.confusion, v.rank_hist, 40, v.n_correct, 2, 1, v.nll_q32)
    assert w.n_scored == 37 and not w.has_rows
    assert w.accuracy == v.n_correct / 40 and w.topk_accuracy(3) == int((ranks <= 3).sum()) / 40
    assert w.log_loss == v.nll_q32 / (37 << 32)
    with pytest.raises(ValueError, match="rows=True"):
        w.val_results()
    with pytest.raises(ValueError, match="one side has per-row values"):
        v.merge(w)
    with pytest.raises(ValueError, match="class lists differ"):
        v.merge(_hand_made(ranks, K + 1))
    with pytest.raises(ValueError, match="do not fit"):
        Validation(v.classes, None, None, None, None, None, v.confusion[:-1], v.rank_hist, 1, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="all or none"):
        Validation(v.classes, v.gt, None, None, None, None, v.confusion, v.rank_hist, 37, 0, 0, 0, 0)


def test_val_results_holds_plain_python_lists():
    v = _hand_made([1, 2, 1, 3, 1], 4)
    r = v.val_results()
    assert type(r).__name__ == "ValResults"
    assert r.classes == ["c0", "c1", "c2", "c3"] and type(r.classes) is list
    assert len(r.scores) == len(r.gt) == len(r.est) == 5
    assert all(type(s) is float for s in r.scores) and all(type(i) is int for i in r.gt + r.est)
    assert r.gt == [0, 1, 2, 3, 0] and r.est == [0, 2, 2, 0, 0] and r.scores == v.scores.tolist()
    # a row of a class the model lacks has no index in the model's classes
    from mermaid_classifier_amd import Validation
    u = Validation(v.classes, [0, -1], [0, 1], [0.5, 0.5], [1, 0], [0.5, 0.0], np.zeros((4, 4)), np.zeros(4), 2, 1, 1, 0, 0)
    with pytest.raises(ValueError, match="1 rows carry a class the model lacks"):
        u.val_results()
    from mermaid_classifier_amd.spacer_shim import TrainClassifierReturnMsg, ValResults
    with pytest.raises(ValueError):
        ValResults(scores=[0.5], gt=[0, 1], est=[0], classes=["a", "b"])
    with pytest.raises(ValueError):
        ValResults(scores=[0.5], gt=[2], est=[0], classes=["a", "b"])
    msg = TrainClassifierReturnMsg(acc=0.5, pc_accs=[0.25], ref_accs=[0.1, 0.2], runtime=1.0)
    assert (msg.acc, msg.pc_accs, msg.ref_accs, msg.runtime) == (0.5, [0.25], [0.1, 0.2], 1.0)


def test_the_checker_on_hand_made_rows_with_ties():
    P = np.array([[0.1, 0.4, 0.4, 0.1],        # 1 and 2 tie at the top, 0 and 3 below: order 1 2 0 3
                  [0.25, 0.25, 0.25, 0.25],    # uniform: class order
                  [0.7, 0.1, 0.2, 0.0],
                  [0.0, 0.0, 1.0, 0.0],
                  [0.2, 0.3, 0.2, 0.3]], np.float32)   # order 1 3 0 2
    for y, want_rank in (([1, 0, 0, 2, 1], [1, 1, 1, 1, 1]), ([2, 3, 1, 0, 3], [2, 4, 3, 2, 2]), ([0, 1, 2, 1, 0], [3, 2, 2, 3, 3]),
                         ([3, 2, 3, 3, 2], [4, 3, 4, 4, 4])):
        got = check_rows(P, y)
        assert got["rank"].tolist() == want_rank
        assert got["est"].tolist() == [1, 0, 0, 2, 1]
        assert np.array_equal(got["score"], np.array([0.4, 0.25, 0.7, 1.0, 0.3], np.float32))
        assert np.array_equal(got["p_true"], P[np.arange(5), y])
        assert got["n_correct"] == sum(r == 1 for r in want_rank)
        assert got["rank_hist"].tolist() == [want_rank.count(r) for r in (1, 2, 3, 4)]
        assert got["confusion"].sum() == 5 and all(got["confusion"][g, e] >= 1 for g, e in zip(y, [1, 0, 0, 2, 1]))
    got = check_rows(P, [2, 3, 1, 0, 3])
    want = sum(int(np.rint(-np.log(max(float(p), 1e-15)) * 2.0 ** 32)) for p in (np.float32(0.4), np.float32(0.25), np.float32(0.1), 0.0,
                                                                                  np.float32(0.3)))
    assert got["nll_q32"] == want
    assert check_rows(P, [2, 2, 2, 2, 2])["nll_q32"] < want        # p_true = 1.0 adds exactly 0


def test_label_maps_for_previous_models():
    from mermaid_classifier_amd.validation import _host_labels, label_map
    data = ["algae", "coral", "rock", "sand"]
    assert label_map(data, data).tolist() == [0, 1, 2, 3]
    assert label_map(["sand", "algae", "rock", "coral"], data).tolist() == [1, 3, 2, 0]              # permuted
    assert label_map(["coral", "sand", "algae"], data).tolist() == [2, 0, -1, 1]                      # the model lacks "rock"
    assert label_map(["algae", "coral", "kelp", "rock", "sand"], data).tolist() == [0, 1, 3, 4]       # the model has an extra class
    assert label_map([3, 1, 2], np.array([1, 2, 3, 4])).tolist() == [1, 2, 0, -1] and label_map(data, data).dtype == np.int32
    with pytest.raises(ValueError, match="duplicates"):
        label_map(["a", "a", "b"], ["a"])
    # host labels: straight indices while every label is known; else indices into [0 .. K-1, -1]
    model = ["coral", "sand", "algae"]
    yi, lmap = _host_labels(model, ["sand", "algae", "sand", "coral"], 4, strict=True)
    assert yi.tolist() == [1, 2, 1, 0] and yi.dtype == np.int32 and lmap is None
    yi, lmap = _host_labels(model, np.array(["sand", "rock", "coral", "rock"]), 4, strict=False)
    assert yi.tolist() == [1, 3, 0, 3] and lmap.tolist() == [0, 1, 2, -1] and lmap[yi].tolist() == [1, -1, 0, -1]
    with pytest.raises(ValueError, match=r"Labels \['rock'\]"):
        _host_labels(model, ["sand", "rock"], 2, strict=True)
