"""Group-robust training without a device: the ABI's declarations, the Python-side argument checks, ``group_balance_weights``
against a hand count, the fp32 emulation of the stage against the bounds of tests/group_dro_checker.py, and the float64 training
loop on a two-group recipe that the README's claim about group DRO rests on."""

import re
from pathlib import Path

import numpy as np
import pytest

import group_dro_checker as gc

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ["mmc_trainer_set_group_dro", "mmc_trainer_group_dro_state", "mmc_trainer_partial_fit_set_weighted",
               "mmc_trainer_group_partial_fit_set_weighted", "mmc_trainer_loss_gradient_weighted"]


def test_header_declares_and_symbols_list_every_entry_point():
    header = (ROOT / "include" / "mmc.h").read_text()
    binding = (ROOT / "mermaid_classifier_amd" / "_lib.py").read_text()
    listed = re.search(r"SYMBOLS = \[(.*?)\n\]", binding, re.S).group(1)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert f'"{name}"' in listed, name
        assert f"lib.{name}.argtypes" in binding, name
    assert re.search(r"#define MMC_DRO_MAX_GROUPS 1024\b", header)
    assert "group-robust training" in header
    source = (ROOT / "mermaid_classifier_amd" / "csrc" / "trainer.hip").read_text()
    for kernel in ("ce_grad_weighted_kernel", "dro_update_kernel", "row_scale_kernel"):
        assert re.search(rf"__global__ [^\n]*void {kernel}\(", source), kernel


# ---- argument checks on the Python side (none of these reaches the library) ---------------------------------------------------------
def _clf(**kw):
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    return TorchMLPClassifier(hidden_layer_sizes=(9,), **kw)


def test_constructor_ranges_params_and_config():
    from mermaid_classifier_amd.sweep import SweepConfig
    for bad in (dict(group_dro_eta=-0.1), dict(group_dro_eta=10.5), dict(group_dro_eta=float("nan")), dict(n_groups=0),
                dict(n_groups=1025), dict(n_groups=2.0), dict(n_groups=True)):
        with pytest.raises(ValueError):
            _clf(**bad)
    clf = _clf(group_dro_eta=0.5, n_groups=3)
    params = clf.get_params()
    assert params["group_dro_eta"] == 0.5 and params["n_groups"] == 3
    assert _clf().get_params()["n_groups"] is None and _clf().get_params()["group_dro_eta"] == 0.0
    clf.set_params(group_dro_eta=1.0, n_groups=7)
    assert (clf.group_dro_eta, clf.n_groups) == (1.0, 7)
    cfg = SweepConfig(hidden_layer_sizes=(9,), group_dro_eta=0.25, n_groups=4, row_group=np.zeros(3, np.int32), row_weight=np.ones(3))
    made = cfg.classifier()
    assert (made.group_dro_eta, made.n_groups) == (0.25, 4)
    import dataclasses
    kw_only = {f.name for f in dataclasses.fields(SweepConfig) if f.kw_only}
    assert {"row_weight", "row_group", "group_dro_eta", "n_groups"} <= kw_only               # keyword only: no positional slot


def test_row_arrays_are_checked_before_any_device_work():
    from mermaid_classifier_amd.torch_classifier import by_position, check_row_arrays
    n = 6
    ok_w, ok_g = np.linspace(0.0, 2.0, n), np.array([0, 1, 2, 0, 1, 2])
    dro = _clf(n_groups=3)
    rw, rg = check_row_arrays(dro, n, ok_w, ok_g)
    assert rw.dtype == np.float32 and rg.dtype == np.int32 and rw.flags.c_contiguous and rg.flags.c_contiguous
    assert check_row_arrays(_clf(), n, None, None) == (None, None)
    assert check_row_arrays(_clf(), n, np.arange(n), None)[0].dtype == np.float32          # integer weights are real numbers
    bad = [
        (dro, ok_w[:-1], None, "one entry per row"), (dro, None, ok_g[:-1], "one entry per row"),
        (dro, ok_w.reshape(2, 3), None, "one entry per row"), (dro, ok_w.astype(complex), None, "real-valued"),
        (dro, np.array(["a"] * n), None, "real-valued"), (dro, ok_w > 1, None, "real-valued"),
        (dro, None, ok_g.astype(np.float64), "integer array"), (dro, None, ok_g > 0, "integer array"),
        (dro, -ok_w, None, "negative or not finite"), (dro, np.where(ok_w > 1, np.inf, ok_w), None, "negative or not finite"),
        (dro, np.where(ok_w > 1, np.nan, ok_w), None, "negative or not finite"), (dro, ok_w * 1e39, None, "negative or not finite"),
        (dro, None, ok_g + 1, "outside [0, 3)"), (dro, None, ok_g - 1, "outside [0, 3)"),
        (_clf(), None, ok_g, "n_groups"),
        (_clf(mixup_alpha=0.4), ok_w, None, "mixup_alpha"), (_clf(mixup_alpha=0.4, n_groups=3), None, ok_g, "mixup_alpha"),
    ]
    for clf, w, g, word in bad:
        with pytest.raises(ValueError, match=re.escape(word)):
            check_row_arrays(clf, n, w, g)
    visit = np.array([4, 0, 5], np.int64)
    assert by_position(rw, visit, 3).tolist() == rw[[4, 0, 5]].tolist() and by_position(rg, None, n) is not None
    assert by_position(None, visit, 3) is None

    class _NoDevice:                                      # a set that fails the test if the pass gets as far as touching it
        dim, classes = 4, np.arange(3)
        def __len__(self):
            return n
        def _handle(self):
            raise AssertionError("device work before the argument check")
        _check_against = _handle
    for clf, w, g, word in bad:
        with pytest.raises(ValueError, match=re.escape(word)):
            clf.partial_fit_rows(_NoDevice(), None, row_weight=w, row_group=g)
        assert not clf._fitted()


def test_group_arrays_per_classifier():
    from mermaid_classifier_amd.sweep import _arrays_per_classifier
    one = np.ones(4)
    assert _arrays_per_classifier("row_weight", None, 3) == [None, None, None]
    assert all(a is one for a in _arrays_per_classifier("row_weight", one, 3))
    per = _arrays_per_classifier("row_weight", [one, None, one * 2], 3)
    assert per[0] is one and per[1] is None and per[2][0] == 2.0
    with pytest.raises(ValueError, match="2 entries for 3"):
        _arrays_per_classifier("row_group", [one, None], 3)


def test_group_balance_weights_against_a_hand_count():
    from mermaid_classifier_amd.sampling import group_balance_weights
    groups = np.array([7, 7, 7, 7, 7, 7, 3, 3, 3, 9])            # 6, 3 and 1 rows
    w = group_balance_weights(groups)
    assert w.dtype == np.float32 and w.shape == (10,)
    # r proportional to 1/6, 1/3, 1: sum = 3, so the scale is 10 / 3
    want = np.array([10 / 18] * 6 + [10 / 9] * 3 + [10 / 3])
    np.testing.assert_allclose(w, want, rtol=1e-6)
    assert abs(float(w.mean()) - 1.0) < 1e-6
    for g in (7, 3, 9):
        assert abs(float(w[groups == g].sum()) - 10 / 3) < 1e-5     # every group carries the same total
    labels = np.array(["a", "a", "a", "a", "b", "b", "a", "b", "b", "a"])
    # cells (7,a) 4, (7,b) 2, (3,a) 1, (3,b) 2, (9,a) 1: five cells, each with total 2
    w2 = group_balance_weights(groups, labels)
    np.testing.assert_allclose(w2, [0.5, 0.5, 0.5, 0.5, 1.0, 1.0, 2.0, 1.0, 1.0, 2.0], rtol=1e-6)
    assert abs(float(w2.mean()) - 1.0) < 1e-6
    np.testing.assert_allclose(group_balance_weights(["x"] * 4), np.ones(4))
    for bad in (np.zeros((2, 2)), np.array([])):
        with pytest.raises(ValueError):
            group_balance_weights(bad)
    with pytest.raises(ValueError):
        group_balance_weights(groups, labels[:-1])


# ---- the fp32 emulation within the bounds ---------------------------------------------------------------------------------------------
def test_fp32_emulation_stays_within_the_bounds_on_the_shared_inputs():
    peak = [0.0, 0.0, 0.0]
    for name, K, G, sl, eta, kind, opts, logq in gc.stage_cases():
        inp = gc.inputs(K)
        z, y, r, a = inp["z"][sl], inp["y"][sl], inp["r"][sl], gc.row_groups(G)[sl]
        loss = gc.loss_options(opts, inp["prior"])
        ref = gc.checker(z, y, inp["w"], r, a, logq, eta, G, **loss)
        bnd = gc.bounds(ref, y, inp["w"], r, a, eta, G)
        d, l, q = gc.emulate(z, y, inp["w"], r, a, logq, eta, G, **loss)
        rd, rl, rq = gc.ratios(d, l, q, ref, bnd)
        assert rd <= 1.0 and rl <= 1.0 and rq <= 1.0, (name, rd, rl, rq)
        assert abs(logsum := gc.logsumexp(q)) < 1e-12, (name, logsum)
        peak = [max(p, v) for p, v in zip(peak, (rd, rl, rq))]
        # groups without mass have no loss and keep their share of q relative to each other
        assert np.array_equal(np.isnan(ref["group_loss"]), ~(ref["V"] > 0))
    for K in (5, 70):                                       # row weights only, and nothing at all
        inp = gc.inputs(K)
        for r in (inp["r"], None):
            for kind, opts in gc.LOSS_KINDS:
                loss = gc.loss_options(opts, inp["prior"])
                ref = gc.checker(inp["z"], inp["y"], inp["w"], r, **loss)
                bnd = gc.bounds(ref, inp["y"], inp["w"], r)
                d, l, _ = gc.emulate(inp["z"], inp["y"], inp["w"], r, **loss)
                rd, rl, _ = gc.ratios(d, l, None, ref, bnd)
                assert rd <= 1.0 and rl <= 1.0, (K, kind, rd, rl)
                peak = [max(peak[0], rd), max(peak[1], rl), peak[2]]
    print(f"emulation peak over bound: dlogits {peak[0]:.3f} row_loss {peak[1]:.3f} logq {peak[2]:.3f}")
    assert min(peak) > 1e-3                                  # the bounds are of the errors' order, not orders above them


def test_bounds_catch_wrong_stages():
    """Three wrong stages miss the bounds by orders of magnitude: q not moved, the weight forgotten, V taken without class weights."""
    inp = gc.inputs(5)
    z, y, w, r, a = inp["z"], inp["y"], inp["w"], inp["r"], gc.row_groups(3)
    ref = gc.checker(z, y, w, r, a, gc.uniform_logq(3), 0.5, 3)
    bnd = gc.bounds(ref, y, w, r, a, 0.5, 3)
    d0, l0, q0 = gc.emulate(z, y, w, r, a, gc.uniform_logq(3), 0.0, 3)                    # eta dropped
    assert max(gc.ratios(d0, l0, q0, ref, bnd)) > 100
    d1, l1, q1 = gc.emulate(z, y, w, None, a, gc.uniform_logq(3), 0.5, 3)                 # row weights dropped
    assert max(gc.ratios(d1, l1, q1, ref, bnd)) > 100
    d2, l2, q2 = gc.emulate(z, y, None, r, a, gc.uniform_logq(3), 0.5, 3)                 # class weights dropped
    assert max(gc.ratios(d2, l2, q2, ref, bnd)) > 100
    ref_w = gc.checker(z, y, w, r)
    bnd_w = gc.bounds(ref_w, y, w, r)
    d3, l3, _ = gc.emulate(z, y, w, None)
    assert max(gc.ratios(d3, l3, None, ref_w, bnd_w)[:2]) > 100


def test_emulated_order_of_group_sums_is_the_kernels():
    """16 / ceil(G / 64) slices per tile of 2048 rows, slices added in order: the result depends on M and G alone."""
    rng = np.random.default_rng(5)
    for M, G in ((17, 3), (5000, 20), (4100, 1024), (300, 65)):
        R = rng.uniform(0, 3, M).astype(np.float32)
        a = rng.integers(0, G, M).astype(np.int32)
        S = gc.group_sums(R, a, G)
        exact = np.zeros(G)
        np.add.at(exact, a, R.astype(np.float64))
        np.testing.assert_allclose(S, exact, rtol=1e-13, atol=0)


# ---- the recipe behind the README's claim -----------------------------------------------------------------------------------------------
def _two_group_data(seed, n=2000, minority=0.05):
    """Feature 0 follows the label in the majority group and opposes it in the minority; feature 1 follows it in both, with noise
    0.8 in the majority and 1.6 in the minority, so the minority stays the harder group even for a head that ignores feature 0."""
    rng = np.random.default_rng(seed)
    grp = (rng.uniform(size=n) < minority).astype(np.int64)
    y = rng.integers(0, 2, n)
    sign = 2.0 * y - 1.0
    x0 = np.where(grp == 0, sign, -sign) + 0.4 * rng.standard_normal(n)
    x1 = sign + np.where(grp == 0, 0.8, 1.6) * rng.standard_normal(n)
    X = np.stack([x0, x1, rng.standard_normal(n)], axis=1)
    return X, y, grp


def _train_f64(X, y, grp, eta, dro, steps=400, mb=100, hidden=8, lr=0.05, seed=0):
    """A 2-layer ReLU head in float64 numpy, plain SGD on the step's loss of include/mmc.h: the mean CE (ERM) or sum_a q_a L_a."""
    rng = np.random.default_rng(seed)
    d, G = X.shape[1], 2
    W1, b1 = rng.normal(0, 0.5, (hidden, d)), np.zeros(hidden)
    W2, b2 = rng.normal(0, 0.5, (2, hidden)), np.zeros(2)
    logq = np.full(G, -np.log(G))
    n = len(y)

    def forward(Xb):
        h = np.maximum(Xb @ W1.T + b1, 0.0)
        zz = h @ W2.T + b2
        zz = zz - zz.max(axis=1, keepdims=True)
        logp = zz - np.log(np.exp(zz).sum(axis=1, keepdims=True))
        return h, logp

    for s in range(steps):
        idx = rng.integers(0, n, mb)
        Xb, yb, ab = X[idx], y[idx], grp[idx]
        h, logp = forward(Xb)
        l = -logp[np.arange(mb), yb]
        if dro:
            V = np.bincount(ab, minlength=G).astype(np.float64)
            S = np.bincount(ab, weights=l, minlength=G)
            has = V > 0
            logq[has] += eta * S[has] / V[has]
            logq -= gc.logsumexp(logq)
            c = np.where(has, np.exp(logq) / np.where(has, V, 1.0), 0.0)[ab]
        else:
            c = np.full(mb, 1.0 / mb)
        dz = np.exp(logp)
        dz[np.arange(mb), yb] -= 1.0
        dz *= c[:, None]
        dW2, db2 = dz.T @ h, dz.sum(axis=0)
        dh = (dz @ W2) * (h > 0)
        dW1, db1 = dh.T @ Xb, dh.sum(axis=0)
        W1 -= lr * dW1; b1 -= lr * db1; W2 -= lr * dW2; b2 -= lr * db2
    _, logp = forward(X)
    l = -logp[np.arange(n), y]
    return np.array([l[grp == a].mean() for a in range(G)]), np.exp(logq)


def test_float64_loop_dro_lowers_the_worst_group_loss():
    ETA = 0.1
    for seed in (0, 1, 2):
        X, y, grp = _two_group_data(seed)
        erm, _ = _train_f64(X, y, grp, 0.0, dro=False, seed=seed)
        dro, q = _train_f64(X, y, grp, ETA, dro=True, seed=seed)
        print(f"seed {seed}: ERM group losses {erm.round(3).tolist()}  DRO {dro.round(3).tolist()}  q {q.round(3).tolist()}")
        assert erm.argmax() == 1                             # ERM leaves the minority behind
        assert dro.max() < 0.5 * erm.max()                   # a wide margin (measured: 0.27 to 0.30 of ERM's), not a rounding matter
        assert q[1] > 0.53                                   # q above 1 / G on the minority (measured: 0.56 to 0.59)
        assert abs(q.sum() - 1.0) < 1e-12
