"""CPU checks of the trainer's optimiser options (include/mmc.h, "optimiser options"), before any GPU run:

a. ``optim.lr_at`` against the library's ``mmc_lr_schedule_at`` (the function ``mmc_trainer_lr_at`` evaluates with the trainer's own
   options; host code, no device) over warm-up, boundary and past-the-end steps of the three kinds, to a relative 1e-15 -- the two
   ``cos`` implementations may differ in the last place -- and the C argument checks;
b. the float64 clipping reference of ``tests/optimizer_checker.py`` against ``torch.nn.utils.clip_grad_norm_`` in float64;
c. the checker's bounds hold for a numpy fp32 emulation of the device's summation order, on the gradients of the GPU file's inputs,
   and those inputs satisfy ``step_ref``'s margin condition;
d. Python argument validation, ``SweepConfig`` round trip, the schedule fill-in of ``train_classifier`` / ``train_sweep``;
e. a classifier state carrying the new fields pickles, and an old state loads with the defaults."""

import ctypes as C
import pickle

import numpy as np
import pytest

import optimizer_checker as oc
from oracle import mlp_step_ref as sr

from mermaid_classifier_amd import optim
from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier

F32, F64 = np.float32, np.float64


def _c_lr_at(lr, kind, warmup, total, ratio, step):
    from mermaid_classifier_amd import _lib
    out = C.c_double(np.nan)
    status = _lib.lib().mmc_lr_schedule_at(lr, optim.LR_KINDS[kind] if isinstance(kind, str) else kind, warmup, total, ratio, step,
                                           C.byref(out))
    return status, out.value


# ---- a. the schedule ---------------------------------------------------------------------------------------------------------------

SCHEDULES = [("constant", 0, 0, 0.0), ("constant", 7, 0, 0.0), ("linear", 0, 40, 0.0), ("linear", 7, 40, 0.25), ("cosine", 0, 40, 0.0),
             ("cosine", 7, 40, 0.1), ("cosine", 39, 40, 1.0), ("linear", 1, 2, 1.0)]


@pytest.mark.parametrize("kind,warmup,total,ratio", SCHEDULES)
def test_lr_at_matches_the_library(kind, warmup, total, ratio):
    lr = 3e-4
    steps = sorted({1, 2, max(1, warmup - 1), max(1, warmup), warmup + 1, (warmup + total) // 2 + 1, max(1, total - 1), max(1, total),
                    total + 1, total + 1000, 10 ** 12})
    for s in steps:
        status, want = _c_lr_at(lr, kind, warmup, total, ratio, s)
        assert status == 0
        got = optim.lr_at(s, lr, kind, warmup, total, ratio)
        assert abs(got - want) <= 1e-15 * abs(want), (s, got, want)
        assert 0.0 <= got <= lr
        if kind != "cosine":
            assert got == want, (s, got, want)


def test_schedule_landmarks():
    lr = 1e-3
    assert optim.lr_at(1, lr) == lr and optim.lr_at(10 ** 9, lr) == lr                      # the default is the constant rate, exactly
    assert _c_lr_at(lr, "constant", 0, 0, 0.0, 5) == (0, lr)
    assert optim.lr_at(3, lr, "constant", 6) == lr * 0.5 and optim.lr_at(6, lr, "constant", 6) == lr
    assert optim.lr_at(40, lr, "linear", 0, 40, 0.25) == lr * 0.25 == optim.lr_at(99, lr, "linear", 0, 40, 0.25)
    assert optim.lr_at(20, lr, "linear", 0, 40, 0.0) == lr * 0.5
    assert abs(optim.lr_at(20, lr, "cosine", 0, 40, 0.0) - lr * 0.5) <= 1e-18
    assert abs(optim.lr_at(41, lr, "cosine", 0, 40, 0.1) - lr * 0.1) <= 1e-18
    assert optim.lr_at(10, lr, "cosine", 10, 40, 0.0) == lr                                 # the end of the warm-up is the peak


@pytest.mark.parametrize("kind,warmup,total,ratio", [(3, 0, 10, 0.0), (-1, 0, 10, 0.0), (1, -1, 10, 0.0), (1, 10, 10, 0.0), (2, 10, 5, 0.0),
                                                     (1, 0, 10, -0.1), (2, 0, 10, 1.5), (0, 0, 0, float("nan"))])
def test_library_rejects_bad_schedules(kind, warmup, total, ratio):
    from mermaid_classifier_amd import _lib
    status, value = _c_lr_at(1e-3, kind, warmup, total, ratio, 1)
    assert status == _lib.MMC_ERR_ARG and np.isnan(value)


# ---- b. the float64 reference against torch ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm", [0.05, 1.0, 1e6])
def test_clip_reference_is_clip_grad_norm(max_norm):
    import torch
    rng = np.random.default_rng(3)
    grads = [rng.standard_normal(s) for s in ((65, 1028), (65,), (130, 65), (130,), (5, 130), (5,))]
    params = [torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g.copy())
    total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    n, clipped = oc.clip_f64(grads, max_norm)
    assert abs(n - total) <= 1e-14 * total
    for p, c in zip(params, clipped):
        assert np.allclose(p.grad.numpy(), c, rtol=1e-14, atol=0.0)
    assert (oc.coef_ref(n, max_norm) == 1.0) == (max_norm == 1e6)


def test_clip_coefficient_mirror():
    assert optim.clip_coefficient(2.0, 1.0) == F32(1.0) / (F32(2.0) + F32(1e-6))
    assert optim.clip_coefficient(0.5, 1.0) == F32(1.0) and optim.clip_coefficient(0.0, 1.0) == F32(1.0)
    assert optim.clip_coefficient(np.inf, 1.0) == F32(0.0) and np.isnan(optim.clip_coefficient(np.nan, 1.0))
    for n, m in ((3.7, 0.9), (1e-3, 1e-4), (9.4591, 4.7)):
        assert abs(float(optim.clip_coefficient(n, m)) - oc.coef_ref(n, m)) <= 4.0 * oc.V * oc.coef_ref(n, m)


# ---- c. the bounds hold for the device's summation order -------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[5, 108])
def case_step(request):
    """(K, step_ref's (ref, bound) on the first mini-batch): raises if the margin condition fails on the GPU file's inputs."""
    K = request.param
    ws, bs, cw, X, y = oc.make_case(K)
    assert [w.shape for w in ws] == [(65, 1028), (130, 65), (K, 130)] and X.shape == (oc.ROWS, 1028)
    assert 65 * 1028 > oc.STRIDE and 65 * 1028 % oc.STRIDE and oc.ROWS == 2 * oc.MB + 30
    return K, sr.step_ref(ws, bs, X[:oc.MB], y[:oc.MB], oc.ALPHA, cw)


def test_emulated_norm_and_clip_within_the_bounds(case_step):
    K, (ref, bound) = case_step
    L = 3
    names = oc.grad_names(L)
    g32 = {k: ref[k].astype(F32) for k in names}                   # an fp32 gradient whose float64 norm is known exactly
    exact, nb = oc.norm_ref(g32, None, L)
    got = float(oc.emulate_norm([g32[k] for k in names]))
    print(f"K={K}: emulated norm {got:.9g}, float64 {exact:.9g}, |diff| / bound {abs(got - exact) / nb:.4f}")
    assert abs(got - exact) <= nb
    # the bound with the gradient's own error is wider, and the L2 term is a visible part of the norm
    n_ref, nb_full = oc.norm_ref(ref, bound, L)
    assert nb_full > nb and nb_full < 0.01 * n_ref
    ws = oc.make_case(K)[0]
    no_l2 = {k: (ref[k] - oc.ALPHA / oc.MB * ws[int(k[2:])].astype(F64) if k.startswith("gW") else ref[k]) for k in names}
    assert abs(oc.norm_ref(no_l2, None, L)[0] - n_ref) > 10.0 * nb_full
    # clipping at half the norm: the emulated fl(g coef) within the derived per-element bound (e = 0)
    c, cb, want, wb = oc.clip_ref(g32, None, L, 0.5 * exact)
    coef = optim.clip_coefficient(F32(got), 0.5 * exact)
    assert abs(float(coef) - c) <= cb
    for k in names:
        ratio, idx = sr.worst_ratio(g32[k] * coef, want[k], wb[k])
        assert ratio <= 1.0, (k, ratio, idx)


def test_a_wrong_summand_breaks_the_norm_bound(case_step):
    """Sharp: dropping the ragged second trip of the first layer's weights (1 284 of 66 820 elements) leaves the bound."""
    K, (ref, _) = case_step
    names = oc.grad_names(3)
    g32 = [ref[k].astype(F32) for k in names]
    exact, nb = oc.norm_ref({k: g for k, g in zip(names, g32)}, None, 3)
    cut = [g32[0].ravel()[:oc.STRIDE]] + g32[1:]
    assert abs(float(oc.emulate_norm(cut)) - exact) > nb


def test_ema_replay_is_fp32_in_the_written_order():
    rng = np.random.default_rng(0)
    s, p = rng.standard_normal(1000).astype(F32), rng.standard_normal(1000).astype(F32)
    out = oc.ema_replay(s, p, 0.999)
    om = F32(1.0 - 0.999)
    assert om != F32(1.0) - F32(0.999)                              # the double expression, not the fp32 one
    assert out.dtype == F32 and np.array_equal(out, s + om * (p - s))
    assert not np.array_equal(out, (F32(0.999) * s + om * p).astype(F32))


# ---- d. Python arguments -------------------------------------------------------------------------------------------------------------------

BAD = [dict(lr_schedule="step"), dict(lr_schedule=None), dict(warmup_steps=-1), dict(warmup_steps=1.5), dict(warmup_steps=True),
       dict(lr_schedule="linear", schedule_steps=10, warmup_steps=10), dict(lr_schedule="cosine", schedule_steps=3, warmup_steps=5),
       dict(schedule_steps=-1), dict(schedule_steps=2.5), dict(final_lr_ratio=-0.01), dict(final_lr_ratio=1.01),
       dict(final_lr_ratio=float("nan")), dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(max_grad_norm=float("inf")),
       dict(max_grad_norm=float("nan")), dict(max_grad_norm=1e39), dict(max_grad_norm=1e-50), dict(max_grad_norm="1"),
       dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=float("nan")), dict(ema_decay=True)]


@pytest.mark.parametrize("kw", BAD, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in BAD])
def test_constructor_rejects(kw):
    with pytest.raises(ValueError):
        TorchMLPClassifier(**kw)


def test_constructor_accepts_and_get_params_carries():
    kw = dict(lr_schedule="cosine", warmup_steps=5, schedule_steps=100, final_lr_ratio=0.1, max_grad_norm=2.5, ema_decay=0.99)
    clf = TorchMLPClassifier(**kw)
    params = clf.get_params()
    assert {k: params[k] for k in kw} == kw
    twin = TorchMLPClassifier(**params)
    assert twin.get_params() == params
    d = TorchMLPClassifier().get_params()
    assert (d["lr_schedule"], d["warmup_steps"], d["schedule_steps"], d["final_lr_ratio"], d["max_grad_norm"], d["ema_decay"]) == \
        ("constant", 0, None, 0.0, None, 0.0)
    TorchMLPClassifier(lr_schedule="linear", warmup_steps=3)        # schedule_steps may wait for train_classifier
    with pytest.raises(ValueError):
        TorchMLPClassifier().use_weights("averaged")
    with pytest.raises(ValueError):
        TorchMLPClassifier(ema_decay=0.9).use_weights("mean")


def test_sweep_config_round_trip():
    from mermaid_classifier_amd import SweepConfig
    kw = dict(lr_schedule="linear", warmup_steps=2, schedule_steps=None, final_lr_ratio=0.5, max_grad_norm=1.0, ema_decay=0.9)
    cfg = SweepConfig((8,), 1e-3, **kw)
    clf = cfg.classifier()
    assert {k: clf.get_params()[k] for k in kw} == kw and clf.hidden_layer_sizes == (8,)
    plain = SweepConfig().classifier().get_params()
    assert plain == TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), learning_rate_init=1e-4, random_state=0).get_params()
    with pytest.raises(TypeError):
        SweepConfig((8,), 1e-3, 1e-4, None, 0, "auto", 0.9, 0.999, 1e-8, None, 0.0, 0.0, None, "cosine")   # keyword only
    with pytest.raises(ValueError):
        SweepConfig(ema_decay=2.0).classifier()


def test_schedule_steps_filled_from_the_budget():
    from mermaid_classifier_amd.training import _contiguous_batches, _fill_schedule_steps
    batches = _contiguous_batches(1000, 300)                        # 300, 300, 300, 100 rows
    assert optim.steps_per_epoch(batches(0), "auto") == 2 + 2 + 2 + 1
    assert optim.steps_per_epoch(batches(0), 64) == 5 + 5 + 5 + 2
    clf = TorchMLPClassifier(lr_schedule="cosine", warmup_steps=3, batch_size=64)
    _fill_schedule_steps(clf, batches, 6)
    assert clf.schedule_steps == 6 * 17
    _fill_schedule_steps(clf, batches, 60)                          # a given value is kept
    assert clf.schedule_steps == 6 * 17
    const = TorchMLPClassifier(warmup_steps=3)
    _fill_schedule_steps(const, batches, 6)
    assert const.schedule_steps is None


# ---- e. pickling -----------------------------------------------------------------------------------------------------------------------

def test_unfitted_state_round_trip_and_old_state_defaults():
    clf = TorchMLPClassifier(hidden_layer_sizes=(8,), lr_schedule="linear", warmup_steps=2, schedule_steps=50, final_lr_ratio=0.2,
                             max_grad_norm=3.0, ema_decay=0.95)
    clf.use_weights("raw")
    twin = pickle.loads(pickle.dumps(clf))
    assert twin.get_params() == clf.get_params() and twin._eval_weights == "raw" and not twin._fitted()
    old = {k: v for k, v in TorchMLPClassifier(hidden_layer_sizes=(8,)).__getstate__().items()
           if k not in ("lr_schedule", "warmup_steps", "schedule_steps", "final_lr_ratio", "max_grad_norm", "ema_decay")}
    assert "ema_decay" not in old and "dropout" in old
    loaded = TorchMLPClassifier.__new__(TorchMLPClassifier)
    loaded.__setstate__(dict(old))
    assert loaded.get_params() == TorchMLPClassifier(hidden_layer_sizes=(8,)).get_params()
    assert not loaded._averages() and loaded.max_grad_norm is None
