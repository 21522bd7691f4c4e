"""CPU checks of ``oracle/mlp_step_ref.py`` (the float64 reference and per-element bounds ``tests/test_gpu_trainer_step.py`` holds
one trainer step to), before any GPU run:

a. sound -- on every input of the GPU file the margin condition holds and the numpy fp32 oracle (``oracle/mlp_train_ref.py``:
   BLAS matmuls, another summation order) has its logits, loss and gradients within 1 x bound of the float64 reference;
b. sharp -- wrong steps each exceed 2 x bound on at least one element, on a ragged mini-batch with alpha > 0: the four mutants
   that pass ``tests/test_trainer.py``'s end-to-end tolerances (every logit gradient halved, the L2 term of dW dropped or scaled by
   the full batch size, the bias gradient tripled), the two it catches, and ``>=`` for ``>`` in the ReLU mask;
c. Adam -- ``adam_f32`` has the bits of the oracle's update, ``adam_param_ref`` bounds the oracle's parameters, and
   ``1.0f - (float)beta2`` in place of ``(float)(1.0 - beta2)`` changes the bits of ``exp_avg_sq``."""

import numpy as np
import pytest

from oracle import mlp_step_ref as sr
from oracle.mlp_train_ref import MLPTrainRef

F32 = np.float32


def _oracle(ws, bs, cw, X, y, **kw):
    """The fp32 oracle's step -> ({name: tensor} as step_ref names them, the oracle after the step)."""
    o = MLPTrainRef(ws, bs, alpha=sr.ALPHA, class_weight=cw, **kw)
    g = {}
    o.step(X, y, g)
    got = {"logits": g["logits"], "loss": np.asarray(g["loss"])}
    for l in range(len(ws)):
        got[f"gW{l}"], got[f"gb{l}"] = g["gW"][l], g["gb"][l]
    return got, o


def _inputs():
    """Every (id, weights, biases, class weights, X, y) the GPU file holds against ``step_ref``."""
    out = [(c.id,) + tuple(sr.make_case(c)) for c in sr.CASES]
    for d in sr.RAGGED_SEEDS:
        ws, bs, cw, X, y, order = sr.ragged_pass(d)
        for s, rows in enumerate((order[:64], order[64:])):
            out.append((f"ragged{d}-step{s}", ws, bs, cw, X[rows], y[rows]))
    X, y, members = sr.group_pass()
    for m, (ws, bs, cw, visit) in enumerate(members):
        out.append((f"group-member{m}", ws, bs, cw, X[visit], y[visit]))
    return out


INPUTS = _inputs()


# ---- a. sound -----------------------------------------------------------------------------------------------------------------

def test_cases_sit_on_the_edges():
    assert [(c.dims, c.mb) for c in sr.CASES] == [((67, 129, 18, 7), m) for m in (1, 5, 64, 65, 77)] + [
        ((64, 64, 16, 4), 64), ((64, 64, 16, 4), 128), ((10, 16, 5), 50), ((67, 7), 13), ((260, 260, 3), 9)]
    assert sum(c.weighted for c in sr.CASES) == len(sr.CASES) // 2
    for c in sr.CASES:
        if c.weighted:
            assert (sr.make_case(c)[2] == 0).sum() == 1
    assert 260 * 260 > sr.SUMSQ_STRIDE


@pytest.mark.parametrize("inp", INPUTS, ids=[i[0] for i in INPUTS])
def test_fp32_oracle_stays_within_one_bound(inp):
    name, ws, bs, cw, X, y = inp
    ref, bound = sr.step_ref(ws, bs, X, y, sr.ALPHA, cw)          # raises if the margin condition fails
    got, _ = _oracle(ws, bs, cw, X, y)
    assert set(got) == set(ref) == set(bound) and len(ref) == 2 + 2 * len(ws)
    bad = []
    for k in ref:
        assert got[k].shape == ref[k].shape == bound[k].shape and np.isfinite(bound[k]).all() and (bound[k] >= 0).all(), k
        ratio, idx = sr.worst_ratio(got[k], ref[k], bound[k])
        print(f"{name:24s} {k:7s} max|got-ref|/bound {ratio:.4f} at {idx}")
        if ratio > 1.0:
            bad.append(sr.exceed_report(k, len(ws), got[k], ref[k], bound[k], 1.0))
    assert not bad, "\n".join(bad)


def test_margin_violation_raises():
    ws, bs, cw, X, y = sr.make_case(sr.CASES[4])
    X = X.copy()
    bs = [b.copy() for b in bs]
    z = X[3].astype(np.float64) @ ws[0][5].astype(np.float64)
    bs[0][5] = F32(-z)                                          # row 3's pre-activation of unit 5 becomes a rounding error
    with pytest.raises(sr.MarginError, match="layer 0"):
        sr.step_ref(ws, bs, X, y, sr.ALPHA, cw)


# ---- b. sharp -----------------------------------------------------------------------------------------------------------------

def _emulate(ws, bs, cw, X, y, alpha, mutant=None, batch_size=None):
    """The gradients of ``MLPTrainRef.step`` in its own arithmetic, with one deliberate bug -> {name: tensor}."""
    L, mb = len(ws), X.shape[0]
    hs = [np.asarray(X, F32)]
    for i, (w, b) in enumerate(zip(ws, bs)):
        z = hs[-1] @ w.T + b
        hs.append(np.maximum(z, F32(0)) if i < L - 1 else z)
    z = hs[-1]
    zs = z - z.max(axis=1, keepdims=True)
    lse = np.log(np.exp(zs).sum(axis=1, dtype=F32))
    logp = zs - lse[:, None]
    w_i = np.ones(mb, F32) if cw is None else cw[y]
    wsum = F32(w_i.sum(dtype=np.float64))
    dz = np.exp(logp)
    dz[np.arange(mb), y] -= F32(1)
    dz *= (w_i / wsum)[:, None]
    if mutant == "logit gradient x 0.5":
        dz = dz * F32(0.5)
    scale = F32(alpha / (batch_size if mutant == "L2 scaled by alpha / batch_size" else mb))
    out = {}
    for l in range(L - 1, -1, -1):
        kept = mb - mb % 16 if mutant == "dW drops the last mb % 16 rows" else mb
        out[f"gW{l}"] = dz[:kept].T @ hs[l][:kept] + (F32(0) if mutant == "L2 term dropped" else scale) * ws[l]
        kept = mb - mb % 4 if mutant == "colsum drops the last mb % 4 rows" else mb
        out[f"gb{l}"] = dz[:kept].sum(axis=0, dtype=F32) * (F32(3) if mutant == "bias gradient x 3" else F32(1))
        if l > 0:
            dz = (dz @ ws[l]) * ((hs[l] >= 0) if mutant == ">= in the mask" else (hs[l] > 0))
    return out


def _dead_unit(ws, bs):
    """Unit 9 of the first hidden layer gets a zero weight row and a zero bias: its pre-activation is an exact 0."""
    ws, bs = [w.copy() for w in ws], [b.copy() for b in bs]
    ws[0][9] = 0
    bs[0][9] = 0
    return ws, bs


def _scenarios():
    ws, bs, cw, X, y, order = sr.ragged_pass(67)
    last = order[64:]
    c = sr.CASES[4]
    ws2, bs2, _, X2, y2 = sr.make_case(c)
    cw2 = sr.make_weights(np.random.default_rng(5), 7)
    y, y2 = y[last].copy(), y2.copy()
    y[-1], y2[-1] = (int(np.flatnonzero(w > 0)[0]) for w in (cw, cw2))     # the row a short column sum drops carries weight
    return {"the 13-row last mini-batch of 77 rows in batches of 64": (ws, bs, cw, X[last], y, 64),
            "77 rows in a batch of 200": (ws2, bs2, cw2, X2, y2, 200)}


MUTANTS = ["logit gradient x 0.5", "L2 term dropped", "L2 scaled by alpha / batch_size", "bias gradient x 3",
           "dW drops the last mb % 16 rows", "colsum drops the last mb % 4 rows", ">= in the mask"]


@pytest.mark.parametrize("scenario", list(_scenarios()))
def test_wrong_steps_exceed_twice_the_bound(scenario):
    ws, bs, cw, X, y, batch_size = _scenarios()[scenario]
    mb = X.shape[0]
    assert sr.ALPHA > 0 and mb % 16 and mb % 4 and mb != batch_size and cw is not None and (cw == 0).sum() == 1
    ws, bs = _dead_unit(ws, bs)
    ref, bound = sr.step_ref(ws, bs, X, y, sr.ALPHA, cw)
    assert (ref["gb0"][9] == 0 and bound["gb0"][9] == 0), "the dead unit's gradient is an exact 0"
    honest = _emulate(ws, bs, cw, X, y, sr.ALPHA)
    want, _ = _oracle(ws, bs, cw, X, y)
    for k in honest:                                            # the emulation is the oracle, and the oracle is within 1 x bound
        assert np.array_equal(honest[k], want[k]), k
        assert sr.worst_ratio(honest[k], ref[k], bound[k])[0] <= 1.0, k
    escaped = []
    for mutant in MUTANTS:
        got = _emulate(ws, bs, cw, X, y, sr.ALPHA, mutant, batch_size)
        over = {k: int((np.abs(got[k].astype(np.float64) - ref[k]) > 2.0 * bound[k]).sum()) for k in got}
        worst = max(got, key=lambda k: sr.worst_ratio(got[k], ref[k], bound[k])[0])
        print(f"{mutant:36s} {sum(over.values()):6d} elements over 2 x bound; worst {worst} "
              f"{sr.worst_ratio(got[worst], ref[worst], bound[worst])[0]:.3g}")
        if not any(over.values()):
            escaped.append(mutant)
    assert not escaped, f"the bound is too loose to catch: {escaped}"


def test_mutants_hit_the_tensor_the_bug_is_in():
    ws, bs, cw, X, y, batch_size = _scenarios()["77 rows in a batch of 200"]
    ref, bound = sr.step_ref(ws, bs, X, y, sr.ALPHA, cw)

    def over(mutant):
        got = _emulate(ws, bs, cw, X, y, sr.ALPHA, mutant, batch_size)
        return {k for k in got if (np.abs(got[k].astype(np.float64) - ref[k]) > 2.0 * bound[k]).any()}
    assert over("bias gradient x 3") == {"gb0", "gb1", "gb2"}
    assert over("L2 term dropped") == over("L2 scaled by alpha / batch_size") == {"gW0", "gW1", "gW2"}
    assert over("colsum drops the last mb % 4 rows") == {"gb0", "gb1", "gb2"}
    assert "gW2" in sr.exceed_report("gW2", 3, _emulate(ws, bs, cw, X, y, sr.ALPHA, "L2 term dropped")["gW2"], ref["gW2"], bound["gW2"])
    assert "EPI_L2, layer 2" in sr.launch_of("gW2", 3) and "colsum" in sr.launch_of("gb0", 3)


# ---- c. Adam ------------------------------------------------------------------------------------------------------------------

def test_adam_emulation_is_the_oracle_s_and_the_fp32_one_minus_beta2_differs():
    ws, bs, cw, X, y = sr.make_case(sr.CASES[4])
    rng = np.random.default_rng(8)
    got, o = _oracle(ws, bs, cw, X, y)                          # one step from zero moments: t = 1
    s = sr.adam_scalars(1)
    for l in range(len(ws)):
        g = got[f"gW{l}"]
        m1, v1 = sr.adam_f32(g, np.zeros_like(g), np.zeros_like(g), s)
        assert np.array_equal(m1, o.mW[l]) and np.array_equal(v1, o.vW[l])
        ref, bound = sr.adam_param_ref(ws[l], m1, v1, s)
        assert (np.abs(o.W[l] - ref) <= bound).all()
    # beta1 = 0 from zero moments: exp_avg is the gradient, bit for bit
    s0 = sr.adam_scalars(1, beta1=0.0)
    assert s0.om_beta1 == F32(1.0)
    assert np.array_equal(sr.adam_f32(g, np.zeros_like(g), np.zeros_like(g), s0)[0], g)
    # the mutant scalar, on random moments at step 1001
    s, bad = sr.adam_scalars(1001), sr.adam_scalars(1001, om_beta2_in_fp32=True)
    assert s.om_beta2 == F32(1.0 - 0.999) and bad.om_beta2 == F32(1.0) - F32(0.999) and s.om_beta2 != bad.om_beta2
    assert s[:2] == bad[:2] and s[3:] == bad[3:]
    m = rng.standard_normal(g.shape).astype(F32) * F32(1e-3)
    v = (rng.uniform(0, 1e-5, g.shape)).astype(F32)
    m1, v1 = sr.adam_f32(g, m, v, s)
    m1b, v1b = sr.adam_f32(g, m, v, bad)
    assert np.array_equal(m1, m1b) and not np.array_equal(v1, v1b)
    print("elements of exp_avg_sq whose bits differ:", int((v1 != v1b).sum()), "of", v1.size)
