"""-m gpu: on-device validation (calibrate_eval_kernel behind mmc_head_evaluate / mmc_head_evaluate_set, validation.validate).

Integers (est, rank, the three tables, the counters) and the bits of score / p_true are compared for identity with the checker of
test_validation_host.py applied to the same handle's own mmc_head_predict probabilities; the loss sum within one 2^-32 unit per row
of the host's (device log against host log) and for identity between device routes; the ranks against the reference's recorded
Predictor outputs within the band the existing probability gates leave.  Shapes: K = 5 (fewer classes than lanes), 108 (some lanes
own two classes), 2500 (row in global memory); row counts that are no multiple of the 4 rows per workgroup; 65 536 + 7 rows at
width 8 (the chunk boundary)."""

import numpy as np
import pytest

from conftest import GOLDEN
from test_validation_host import check_rows

pytestmark = pytest.mark.gpu

TOTALS = ("n", "n_correct", "n_unknown", "n_nonfinite", "nll_q32")


def _load(name):
    from mermaid_classifier_amd import load_predictor
    return load_predictor(GOLDEN / name / "model.pt", GOLDEN / name / "model.json")


def _ptr(a):
    return None if a is None else a.ctypes.data


def _outputs(n, K):
    return dict(est=np.full(n, -7, np.int32), score=np.full(n, -7, np.float32), rank=np.full(n, -7, np.int32),
                p_true=np.full(n, -7, np.float32), totals=np.full(5, -7, np.int64), confusion=np.full((K, K), -7, np.int64),
                rank_hist=np.full(K, -7, np.int64))


def c_evaluate(head, X, y, lmap=None, device=False):
    """mmc_head_evaluate on host rows, or on the same rows uploaded first (device pointer, flags 0)."""
    from mermaid_classifier_amd import _lib
    X = np.ascontiguousarray(X, np.float32)
    y = np.ascontiguousarray(y, np.int32)
    o = _outputs(len(X), head.n_classes)
    if device:
        import torch
        xd = torch.from_numpy(X).cuda()
        src, flags = xd.data_ptr(), 0
    else:
        src, flags = X.ctypes.data, _lib.MMC_IN_HOST
    _lib.check(_lib.lib().mmc_head_evaluate(head._h, src, y.ctypes.data, len(X), _ptr(lmap), 0 if lmap is None else len(lmap),
                                            o["est"].ctypes.data, o["score"].ctypes.data, o["rank"].ctypes.data, o["p_true"].ctypes.data,
                                            o["totals"].ctypes.data, o["confusion"].ctypes.data, o["rank_hist"].ctypes.data, flags, None))
    return o


def c_evaluate_set(head, fs, first, n, lmap=None):
    from mermaid_classifier_amd import _lib
    o = _outputs(n, head.n_classes)
    _lib.check(_lib.lib().mmc_head_evaluate_set(head._h, fs._handle(), first, n, _ptr(lmap), 0 if lmap is None else len(lmap),
                                                o["est"].ctypes.data, o["score"].ctypes.data, o["rank"].ctypes.data,
                                                o["p_true"].ctypes.data, o["totals"].ctypes.data, o["confusion"].ctypes.data,
                                                o["rank_hist"].ctypes.data, None))
    return o


def same_outputs(a, b):
    for k in ("est", "rank", "totals", "confusion", "rank_hist"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("score", "p_true"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def matches_checker(o, proba, y, what=""):
    """Every integer and every bit against the checker on `proba`; the loss sum within one unit per row."""
    want = check_rows(proba, y)
    n = len(y)
    assert np.array_equal(o["est"], want["est"]), what
    assert np.array_equal(o["rank"], want["rank"]), what
    assert np.array_equal(o["score"].view(np.uint32), want["score"].view(np.uint32)), what
    assert np.array_equal(o["p_true"].view(np.uint32), want["p_true"].view(np.uint32)), what
    assert np.array_equal(o["confusion"], want["confusion"]), what
    assert np.array_equal(o["rank_hist"], want["rank_hist"]), what
    assert o["totals"][:4].tolist() == [n, want["n_correct"], 0, 0], what
    gap = abs(int(o["totals"][4]) - want["nll_q32"])
    print(f"{what}: {n} rows, |sum_nll_q32 - host| = {gap} units of 2^-32 (allowed {n})")
    assert gap <= n, what


def _set_of(head, X, y):
    from mermaid_classifier_amd import FeatureSet
    return FeatureSet(head.input_dim, list(range(head.n_classes))).append(X, y)


# ---- 1. same bits as the served head ----

@pytest.mark.parametrize("name", ["head_fixture", "head108"])
def test_evaluate_has_the_bits_of_the_served_head(name):
    head = _load(name)._head
    K = head.n_classes
    X = np.load(GOLDEN / f"{name}_io.npz")["X"]
    assert len(X) == (512 if name == "head_fixture" else 256)
    y = (7 * np.arange(len(X))) % K
    proba, arg = head.predict(X)
    host = c_evaluate(head, X, y)
    matches_checker(host, proba, y, f"{name} host pointers")
    assert np.array_equal(host["est"], arg)
    dev = c_evaluate(head, X, y, device=True)
    matches_checker(dev, proba, y, f"{name} device pointers")
    same_outputs(host, dev)
    fs = _set_of(head, X, y)
    same_outputs(host, c_evaluate_set(head, fs, 0, len(X)))
    # a ragged last workgroup
    m = len(X) - 3
    assert m % 4 != 0
    matches_checker(c_evaluate(head, X[:m], y[:m]), proba[:m], y[:m], f"{name} {m} rows")
    fs.close()


# ---- 2. routes and splits ----

def test_routes_and_ragged_pieces_add_up_to_the_whole_call():
    head = _load("head_fixture")._head
    X = np.load(GOLDEN / "head_fixture_io.npz")["X"]
    n, K = len(X), head.n_classes
    y = (7 * np.arange(n)) % K
    whole = c_evaluate(head, X, y)
    fs = _set_of(head, X, y)
    same_outputs(whole, c_evaluate_set(head, fs, 0, n))
    for route in ("host", "set"):
        parts = [c_evaluate(head, X[a:b], y[a:b]) if route == "host" else c_evaluate_set(head, fs, a, b - a)
                 for a, b in ((0, 5), (5, 300), (300, n))]
        glued = {k: np.concatenate([p[k] for p in parts]) for k in ("est", "score", "rank", "p_true")}
        glued.update({k: sum(p[k] for p in parts) for k in ("totals", "confusion", "rank_hist")})
        same_outputs(whole, glued)
    same_outputs(whole, c_evaluate(head, X, y))                                    # a repeat call: the same bits
    # the optional outputs may be NULL: the totals do not change
    from mermaid_classifier_amd import _lib
    tot = np.zeros(5, np.int64)
    yi = np.ascontiguousarray(y, np.int32)
    _lib.check(_lib.lib().mmc_head_evaluate(head._h, X.ctypes.data, yi.ctypes.data, n, None, 0, None, None, None, None, tot.ctypes.data,
                                            None, None, _lib.MMC_IN_HOST, None))
    assert np.array_equal(tot, whole["totals"])
    fs.close()


def test_evaluate_above_the_65536_row_chunk():
    head = _load("head_fixture")._head
    X0 = np.load(GOLDEN / "head_fixture_io.npz")["X"]
    n, K = 65536 + 7, head.n_classes
    X = np.ascontiguousarray(np.tile(X0, (-(-n // len(X0)), 1))[:n])
    y = (7 * np.arange(n)) % K
    proba, _ = head.predict(X)
    host = c_evaluate(head, X, y)
    matches_checker(host, proba, y, "65543 rows")
    same_outputs(host, c_evaluate(head, X, y))
    fs = _set_of(head, X, y)
    same_outputs(host, c_evaluate_set(head, fs, 0, n))
    tail = c_evaluate_set(head, fs, 11, n - 11)                                    # the chunk boundary falls elsewhere in the set
    assert np.array_equal(tail["rank"], host["rank"][11:]) and np.array_equal(tail["p_true"].view(np.uint32), host["p_true"][11:].view(np.uint32))
    head_part = c_evaluate_set(head, fs, 0, 11)
    for k in ("totals", "confusion", "rank_hist"):
        assert np.array_equal(tail[k] + head_part[k], host[k]), k
    fs.close()


# ---- 3. a head wider than the LDS row ----

def test_evaluate_of_a_head_wider_than_the_lds_row():
    from mermaid_classifier_amd.inference import DeviceHead, HeadParams
    rng = np.random.default_rng(5)
    K = 2500
    prm = HeadParams([rng.normal(0, 0.5, (K, 8)).astype(np.float32)], [rng.normal(0, 0.1, K).astype(np.float32)],
                     rng.uniform(-30, -5, K).astype(np.float32), rng.uniform(1, 4, K).astype(np.float32))
    head = DeviceHead(prm)
    X = rng.normal(0, 1, (37, 8)).astype(np.float32)
    y = (7 * np.arange(37) * 41) % K
    proba, _ = head.predict(X)
    o = c_evaluate(head, X, y)
    matches_checker(o, proba, y, "K = 2500")
    y2 = check_rows(proba, y)["est"].copy()                                        # and with the true class on top in most rows
    y2[::5] = (y2[::5] + 1) % K
    matches_checker(c_evaluate(head, X, y2, device=True), proba, y2, "K = 2500, y = est")
    same_outputs(o, c_evaluate(head, X, y))
    head.close()


# ---- 4. ties ----

def _fixture_params(**override):
    from mermaid_classifier_amd.inference import HeadParams
    io = np.load(GOLDEN / "head_fixture_io.npz")
    d = {k: io[k].copy() for k in ("W0", "b0", "W1", "b1", "a", "b")}
    d.update(override)
    return HeadParams([d["W0"], d["W1"]], [d["b0"], d["b1"]], d["a"], d["b"]), io["X"]


def test_uniform_rows_rank_in_class_order():
    """Every Platt b = +200: every row is the uniform row 1/K, a K-way tie: est = 0 and the true class y ranks y + 1."""
    from mermaid_classifier_amd.inference import DeviceHead
    prm, X = _fixture_params(b=np.full(5, 200.0, np.float32))
    head = DeviceHead(prm)
    y = (7 * np.arange(len(X))) % 5
    o = c_evaluate(head, X, y)
    fifth = np.float32(1.0) / np.float32(5.0)
    assert np.all(o["est"] == 0) and np.all(o["score"] == fifth) and np.all(o["p_true"] == fifth)
    assert np.array_equal(o["rank"], (y + 1).astype(np.int32))
    assert o["totals"][:4].tolist() == [len(X), int((y == 0).sum()), 0, 0]
    matches_checker(o, head.predict(X)[0], y, "uniform rows")
    head.close()


def test_two_identical_classes_rank_lower_class_first():
    from mermaid_classifier_amd.inference import DeviceHead
    io = np.load(GOLDEN / "head_fixture_io.npz")
    W1, b1, a, b = io["W1"].copy(), io["b1"].copy(), io["a"].copy(), io["b"].copy()
    W1[3], b1[3], a[3], b[3] = W1[1], b1[1], a[1], b[1]
    prm, X = _fixture_params(W1=W1, b1=b1, a=a, b=b)
    head = DeviceHead(prm)
    proba, _ = head.predict(X)
    assert np.array_equal(proba[:, 1].view(np.uint32), proba[:, 3].view(np.uint32))
    ones, threes = np.full(len(X), 1), np.full(len(X), 3)
    o1, o3 = c_evaluate(head, X, ones), c_evaluate(head, X, threes)
    assert np.array_equal(o3["rank"], o1["rank"] + 1)                              # class 1 directly above class 3 in every row
    assert np.array_equal(o1["p_true"].view(np.uint32), o3["p_true"].view(np.uint32))
    assert not np.any(o1["est"] == 3)
    matches_checker(o1, proba, ones, "tie, y = 1")
    matches_checker(o3, proba, threes, "tie, y = 3")
    head.close()


# ---- 5. NaN ----

def test_a_nan_row_is_counted_and_leaves_totals_and_neighbours_alone():
    """A one-layer head, so that a NaN feature reaches the probabilities (a hidden ReLU would turn it into 0)."""
    from mermaid_classifier_amd.inference import DeviceHead, HeadParams
    rng = np.random.default_rng(9)
    K = 5
    prm = HeadParams([rng.normal(0, 0.7, (K, 8)).astype(np.float32)], [rng.normal(0, 0.1, K).astype(np.float32)],
                     rng.uniform(-12, -4, K).astype(np.float32), rng.uniform(0.5, 2, K).astype(np.float32))
    head = DeviceHead(prm)
    X = rng.normal(0, 1, (5, 8)).astype(np.float32)
    y = np.array([0, 3, 2, 4, 1])
    keep = np.array([0, 1, 3, 4])
    four = c_evaluate(head, X[keep], y[keep])
    matches_checker(four, head.predict(X[keep])[0], y[keep], "the four clean rows")
    for bad_row in (X[2] * np.nan, np.where(np.arange(8) == 6, np.nan, X[2]).astype(np.float32)):
        bad = X.copy()
        bad[2] = bad_row
        assert np.isnan(head.predict(bad)[0][2]).any()
        five = c_evaluate(head, bad, y)
        assert five["totals"].tolist() == [5, four["totals"][1], 0, 1, four["totals"][4]]
        assert np.array_equal(five["confusion"], four["confusion"]) and np.array_equal(five["rank_hist"], four["rank_hist"])
        assert 0 <= five["est"][2] < K and 1 <= five["rank"][2] <= K
        for k in ("est", "rank"):
            assert np.array_equal(five[k][keep], four[k])
        for k in ("score", "p_true"):
            assert np.array_equal(five[k][keep].view(np.uint32), four[k].view(np.uint32))
    head.close()


# ---- 6. label maps ----

def test_label_maps_permuted_and_with_an_unknown_class():
    pred = _load("head_fixture")
    head = pred._head
    X = np.load(GOLDEN / "head_fixture_io.npz")["X"]
    n, K = len(X), head.n_classes
    y = (7 * np.arange(n)) % K
    plain = c_evaluate(head, X, y)
    perm = np.array([3, 0, 4, 1, 2], np.int32)                                     # caller's label j is the head's class perm[j]
    inv = np.argsort(perm)
    same_outputs(plain, c_evaluate(head, X, inv[y], lmap=perm))
    from mermaid_classifier_amd import FeatureSet
    fs = FeatureSet(8, list(range(K))).append(X, inv[y])
    same_outputs(plain, c_evaluate_set(head, fs, 0, n, lmap=perm))
    fs.close()
    # the caller's label 2 (the head's class 4) is unknown to the head
    lost = perm.copy()
    lost[2] = -1
    o = c_evaluate(head, X, inv[y], lmap=lost)
    gone = y == 4
    assert gone.sum() > 0 and o["totals"][2] == gone.sum() and o["totals"][0] == n and o["totals"][3] == 0
    assert np.all(o["rank"][gone] == 0) and np.all(o["p_true"][gone] == 0)
    assert np.array_equal(o["rank"][~gone], plain["rank"][~gone]) and np.array_equal(o["est"], plain["est"])
    assert np.array_equal(o["score"].view(np.uint32), plain["score"].view(np.uint32))
    rest = check_rows(head.predict(X[~gone])[0], y[~gone])
    assert o["totals"][1] == rest["n_correct"] and np.array_equal(o["confusion"], rest["confusion"])
    assert np.array_equal(o["rank_hist"], rest["rank_hist"]) and o["rank_hist"].sum() == n - gone.sum()
    # the Python route: a set with its own class list (sorted, one class the model lacks); accuracy as the host compares strings
    from mermaid_classifier_amd import previous_accuracies, validate
    names = np.array(pred.classes + ["zz unknown to the model"])
    labels = names[np.where(np.arange(n) % 11 == 0, K, y)]
    vs = FeatureSet(8, names.tolist()).append(X, labels)
    assert vs.classes.tolist() != pred.classes
    v = validate(pred, vs)
    want_acc = float(np.mean(np.asarray(pred.predict(X)) == labels))
    assert v.n == n and v.n_unknown == int((labels == names[K]).sum()) > 0 and v.accuracy == want_acc
    assert np.all(v.gt[labels == names[K]] == -1) and np.all(v.ranks[labels == names[K]] == 0)
    assert [pred.classes[i] for i in v.gt[v.gt >= 0]] == labels[v.gt >= 0].tolist()
    t = validate(pred, vs, rows=False)
    assert not t.has_rows and all(getattr(t, k) == getattr(v, k) for k in TOTALS)
    assert np.array_equal(t.confusion, v.confusion) and np.array_equal(t.rank_hist, v.rank_hist)
    assert previous_accuracies([pred, pred], vs) == [want_acc, want_acc]
    assert previous_accuracies([pred], (X, labels)) == [want_acc]                  # host rows, unknown labels allowed here
    with pytest.raises(ValueError, match="are not in the model's classes"):
        validate(pred, (X, labels))
    # host batches of known labels == the set of the same rows
    known = names[y]
    hb = validate(pred, [(X[:100], known[:100]), (X[100:], known[100:])])
    ks = FeatureSet(8, pred.classes).append(X, known)
    kv = validate(pred, ks)
    for k in ("gt", "est", "scores", "ranks", "p_true", "confusion", "rank_hist"):
        assert np.array_equal(getattr(hb, k), getattr(kv, k)), k
    assert all(getattr(hb, k) == getattr(kv, k) for k in TOTALS)
    assert np.array_equal(kv.ranks, plain["rank"]) and kv.scores.dtype == np.float64 and np.array_equal(kv.scores, plain["score"].astype(np.float64))
    assert kv.nll_q32 == plain["totals"][4] and kv.log_loss == kv.nll_q32 / (n << 32)
    vs.close()
    ks.close()


def test_c_abi_argument_checks_with_a_live_head():
    from mermaid_classifier_amd import FeatureSet, _lib
    lib = _lib.lib()
    head = _load("head_fixture")._head
    X = np.load(GOLDEN / "head_fixture_io.npz")["X"][:8].copy()
    tot = np.full(5, -1, np.int64)
    F = _lib.MMC_IN_HOST

    def call(y, n=8, lmap=None, n_labels=None, totals=tot):
        y = np.ascontiguousarray(y, np.int32)
        nl = (0 if lmap is None else len(lmap)) if n_labels is None else n_labels
        return lib.mmc_head_evaluate(head._h, X.ctypes.data, y.ctypes.data, n, _ptr(lmap), nl, None, None, None, None, _ptr(totals), None, None, F, None)

    ok = np.arange(8) % 5
    assert call(ok, n=-1) == _lib.MMC_ERR_ARG and b"negative" in lib.mmc_last_error()
    assert call(ok, n=0) == _lib.MMC_OK and tot.tolist() == [0] * 5
    assert call(ok, totals=None) == _lib.MMC_ERR_ARG and b"totals is NULL" in lib.mmc_last_error()
    assert call([0, 1, 2, 3, 4, 5, 0, 1]) == _lib.MMC_ERR_ARG and b"y[5] = 5 outside [0, 5)" in lib.mmc_last_error()
    assert call([0, -1, 2, 3, 4, 0, 0, 1]) == _lib.MMC_ERR_ARG
    m = np.array([0, 1, 2, 3, 4, -1, 2], np.int32)
    assert call([0, 1, 2, 3, 4, 5, 6, 7], lmap=m) == _lib.MMC_ERR_ARG and b"y[7] = 7 outside [0, 7)" in lib.mmc_last_error()
    assert call([0, 1, 2, 3, 4, 5, 6, 6], lmap=m) == _lib.MMC_OK and tot[0] == 8 and tot[2] == 1
    assert call(ok, lmap=np.array([0, 5], np.int32)) == _lib.MMC_ERR_ARG and b"label_map[1] = 5 outside [-1, 5)" in lib.mmc_last_error()
    assert call(ok, lmap=np.array([-2, 1], np.int32)) == _lib.MMC_ERR_ARG
    assert call(ok, n_labels=3) == _lib.MMC_ERR_ARG and b"without a label_map" in lib.mmc_last_error()
    assert call(ok, n=59000001) == _lib.MMC_ERR_ARG and b"split it" in lib.mmc_last_error()

    def call_set(fs, first, n, lmap=None):
        return lib.mmc_head_evaluate_set(head._h, None if fs is None else fs._handle(), first, n, _ptr(lmap), 0 if lmap is None else len(lmap),
                                         None, None, None, None, tot.ctypes.data, None, None, None)

    assert call_set(None, 0, 1) == _lib.MMC_ERR_ARG and b"feature set handle is NULL" in lib.mmc_last_error()
    wide = FeatureSet(9, list(range(5))).append(np.zeros((2, 9), np.float32), [0, 1])
    assert call_set(wide, 0, 2) == _lib.MMC_ERR_ARG and b"9 columns, head expects 8" in lib.mmc_last_error()
    six = FeatureSet(8, list(range(6))).append(X, ok)
    assert call_set(six, 0, 8) == _lib.MMC_ERR_ARG and b"6 classes, head 5" in lib.mmc_last_error()
    assert call_set(six, 0, 8, lmap=m) == _lib.MMC_ERR_ARG and b"6 classes, label_map covers 7" in lib.mmc_last_error()
    assert call_set(six, 0, 8, lmap=m[:6]) == _lib.MMC_OK and tot[0] == 8
    five = FeatureSet(8, list(range(5))).append(X, ok)
    for first, n in ((0, 9), (-1, 2), (8, 1), (3, -1)):
        assert call_set(five, first, n) == _lib.MMC_ERR_ARG and b"outside the set's 8 rows" in lib.mmc_last_error()
    assert call_set(five, 8, 0) == _lib.MMC_OK and tot.tolist() == [0] * 5
    assert call_set(five, 3, 5) == _lib.MMC_OK and tot[0] == 5
    for fs in (wide, six, five):
        fs.close()


# ---- 7. against the reference's own outputs ----

@pytest.mark.parametrize("name,dp_bound,max_undecidable", [("head_fixture", 1e-6, 0), ("head108", 2e-5, 12)])   # 12 = 5 % of 256 rows
def test_ranks_against_the_reference_predictor(name, dp_bound, max_undecidable):
    """Labels: the reference's class at rank [1,1,1,2,3,1,2,5][i mod 8] of its recorded probabilities (golden proba_predictor_f64).
    dp = measured max|p_gpu - p_ref|, bounded by the head's existing gate.  The device rank of row i must lie in
    [1 + #{c: P_ref[c] > P_ref[y] + 2dp}, #{c: P_ref[c] >= P_ref[y] - 2dp}]; where the two ends meet the row is decidable and the
    rank is the reference's.  Undecidable rows are counted, printed and capped (the recorded probabilities alone give 6 of 256 for
    head108 at 2dp = 2e-5 and 10 at 4e-5, the largest the gate admits; 0 for the fixture)."""
    from mermaid_classifier_amd import Validation, validate
    pred = _load(name)
    io = np.load(GOLDEN / f"{name}_io.npz")
    X, p_ref = io["X"], io["proba_predictor_f64"]
    n, K = p_ref.shape
    order_ref = np.argsort(-p_ref, axis=1, kind="stable")
    want_rank = np.array([1, 1, 1, 2, 3, 1, 2, 5])[np.arange(n) % 8]
    y = order_ref[np.arange(n), want_rank - 1]
    dp = float(np.abs(pred.predict_proba(X) - p_ref).max())
    v = validate(pred, (X, np.asarray(pred.classes)[y]))
    p_y = p_ref[np.arange(n), y][:, None]
    lo = 1 + (p_ref > p_y + 2 * dp).sum(1)
    hi = (p_ref >= p_y - 2 * dp).sum(1)
    undecidable = int((lo != hi).sum())
    print(f"{name}: max|dp| {dp:.3g} (bound {dp_bound:g}); undecidable rows {undecidable} of {n} (cap {max_undecidable}); "
          f"rows whose rank differs from the reference's {int((v.ranks != want_rank).sum())}")
    assert dp <= dp_bound
    assert np.all((lo <= v.ranks) & (v.ranks <= hi))
    assert np.array_equal(v.ranks[lo == hi], want_rank[lo == hi])
    assert undecidable <= max_undecidable
    assert np.array_equal(v.est, p_ref.argmax(1))
    assert np.array_equal(v.gt, y) and v.n_unknown == 0 and v.n_nonfinite == 0
    assert np.abs(v.p_true.astype(np.float64) - p_y[:, 0]).max() <= dp_bound and np.abs(v.scores - p_ref.max(1)).max() <= dp_bound
    if max_undecidable == 0:    # every row decidable: the rank statistics of the recorded probabilities, exactly
        ref = Validation(pred.classes, None, None, None, None, None, np.zeros((K, K)), np.bincount(want_rank - 1, minlength=K), n,
                         int((want_rank == 1).sum()), 0, 0, 0)
        for k in (1, 3, 5):
            assert v.topk_accuracy(k) == ref.topk_accuracy(k) == np.mean(want_rank <= k)
        assert v.mrr == ref.mrr and v.mrr == pytest.approx(float(np.mean(1.0 / want_rank)), rel=1e-14, abs=0)


# ---- 8. end to end ----

def test_train_and_validate_returns_the_reference_triple():
    from mermaid_classifier_amd import FeatureSet, train_and_validate
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    rng = np.random.default_rng(17)
    K, dim = 4, 16
    classes = [f"class {i}" for i in range(K)]
    centres = rng.normal(0, 1.5, (K, dim))
    yi = rng.integers(0, K, 1000)
    X = (centres[yi] + rng.normal(0, 1.0, (1000, dim))).astype(np.float32)
    labels = np.asarray(classes)[yi]
    splits = (slice(0, 600), slice(600, 800), slice(800, 1000))

    def run(pc_models):
        sets = [FeatureSet(dim, classes).append(X[s], labels[s]) for s in splits]
        clf = TorchMLPClassifier(hidden_layer_sizes=(32, 16), learning_rate_init=1e-2, random_state=0)
        out = train_and_validate(*sets, 3, batch_size=200, clf=clf, pc_models=pc_models)
        for s in sets:
            s.close()
        return out

    cal, res, msg = run(())
    assert type(res).__name__ == "ValResults" and type(msg).__name__ == "TrainClassifierReturnMsg"
    assert len(res.scores) == len(res.gt) == len(res.est) == 200 and res.classes == classes
    assert res.gt == yi[splits[2]].tolist()
    want = cal.predict(X[splits[2]])
    assert [classes[i] for i in res.est] == want.tolist()
    assert msg.acc == float(np.mean(want == labels[splits[2]]))
    assert np.array_equal(np.asarray(res.scores), cal.predict_proba(X[splits[2]]).max(1))
    assert msg.pc_accs == [] and len(msg.ref_accs) == 3 and msg.runtime > 0
    cal2, res2, msg2 = run([cal.predictor()])
    assert msg2.acc == msg.acc and msg2.pc_accs == [msg.acc] and len(msg2.ref_accs) == 3
    assert res2.est == res.est and res2.scores == res.scores
