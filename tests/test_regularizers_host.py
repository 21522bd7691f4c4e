"""CPU checks of the trainer's regularisers (include/mmc.h, "regularisers"), before any GPU run:

a. the numpy Philox of tests/regularizer_checker.py gives the three known answers, and the masks keep the share they should;
b. the float64 step of that module is ``oracle/mlp_step_ref.step_ref`` when nothing is switched on, its gradients are torch float64
   autograd's with the masks as constants, a numpy fp32 restatement stays within 1 x bound on every case of the GPU file, and five
   wrong steps each exceed 2 x bound;
c. ``sampling.mixup_plan``;
d. the Python surface: constructor, ``set_params``, pickles from before the options, ``SweepConfig``, the ``ValueError``s;
e. the header declares the new entry points, ``_lib.SYMBOLS`` lists them, and they reject bad arguments without a device."""

import ctypes as C
import pickle
from pathlib import Path

import numpy as np
import pytest

import regularizer_checker as rc
from oracle import mlp_step_ref as sr

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["mmc_trainer_set_dropout", "mmc_trainer_partial_fit_set_mixed", "mmc_trainer_group_partial_fit_set_mixed",
               "mmc_trainer_loss_gradient_mixed"]


# ---- a. Philox and the masks ---------------------------------------------------------------------------------------------------
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    for ctr, key, want in KNOWN:
        assert tuple(int(v) for v in rc.philox4x32_10(ctr, key)) == want
    both = rc.philox4x32_10([k[0] for k in KNOWN[:1]] * 2, KNOWN[0][1])          # vectorised over leading dimensions
    assert both.shape == (2, 4) and both.dtype == np.uint32 and np.array_equal(both[0], both[1])


@pytest.mark.parametrize("p", [0.5, 0.1])
def test_keep_fraction_is_binomial(p):
    n = 1 << 20
    keep = rc.keep_mask(rc.MASK_SEED, 7, 1, 1024, 1024, p)
    q = 1.0 - rc.thresh(p) / 2.0 ** 32
    dev = abs(keep.sum() / n - q) / np.sqrt(q * (1 - q) / n)
    print(f"p {p}: kept {keep.sum()} of {n}, {dev:.2f} standard deviations from {q:.6f}")
    assert dev <= 5.0


def test_mask_depends_on_seed_step_site_and_position_only():
    a = rc.keep_mask(rc.MASK_SEED, 3, 1, 67, 130, 0.5)
    assert np.array_equal(a[:10], rc.keep_mask(rc.MASK_SEED, 3, 1, 10, 130, 0.5))           # rows do not depend on how many follow
    for other in (rc.keep_mask(rc.MASK_SEED + 1, 3, 1, 67, 130, 0.5), rc.keep_mask(rc.MASK_SEED + (1 << 32), 3, 1, 67, 130, 0.5),
                  rc.keep_mask(rc.MASK_SEED, 4, 1, 67, 130, 0.5), rc.keep_mask(rc.MASK_SEED, 3, 2, 67, 130, 0.5),
                  rc.keep_mask(rc.MASK_SEED, 3, 1, 67, 130, 0.5, width=192)):
        assert 0.3 < (a != other).mean() < 0.7
    assert rc.keep_mask(1, 0, 0, 5, 7, 0.0).all() and rc.thresh(1e-11) == 0 and rc.thresh(0.9) == 3865470566
    assert rc.scale32(0.5) == np.float32(2.0) and rc.scale32(0.1) == np.float32(1.0 / 0.9)


# ---- b. the float64 step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [sr.CASES[4], sr.CASES[5], sr.CASES[8]], ids=lambda c: c.id)
def test_checker_without_regularisers_is_step_ref(case):
    ws, bs, cw, X, y = sr.make_case(case)
    want, want_bound = sr.step_ref(ws, bs, X, y, sr.ALPHA, cw)
    got, bound = rc.step(ws, bs, X, y, sr.ALPHA, cw, masks=rc.step_masks(5, 0, case.dims, case.mb, 0.0, 0.0))
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(got[k], want[k]) and np.array_equal(bound[k], want_bound[k]), k


def _torch_step(ws, bs, X, y, alpha, cw, masks, y2, lam, eps):
    """The definition in torch float64, masks as constants -> {name: tensor}."""
    import torch
    W = [torch.tensor(np.asarray(w, np.float64), requires_grad=True) for w in ws]
    b = [torch.tensor(np.asarray(v, np.float64), requires_grad=True) for v in bs]
    mult = [None if m is None else torch.tensor(np.where(m[0], 1.0 / (1.0 - m[1]), 0.0)) for m in masks]
    h = torch.tensor(np.asarray(X, np.float64))
    if mult[0] is not None:
        h = h * mult[0]
    L, mb = len(W), X.shape[0]
    for l in range(L):
        h = h @ W[l].T + b[l]
        if l < L - 1:
            h = torch.relu(h)
            if mult[l + 1] is not None:
                h = h * mult[l + 1]
    K = h.shape[1]
    w = torch.ones(K, dtype=torch.float64) if cw is None else torch.tensor(cw.astype(np.float64))
    logp = torch.log_softmax(h, dim=1)
    smooth = (eps / K) * -(logp * w[None, :]).sum(dim=1)

    def term(t):
        t = torch.tensor(np.asarray(t, np.int64))
        return (1.0 - eps) * w[t] * -logp.gather(1, t[:, None])[:, 0] + smooth, w[t]
    if y2 is None:
        l, wt = term(y)
    else:
        la, lb = float(np.float32(lam)), float(np.float32(1.0) - np.float32(lam))
        (l1, w1), (l2, w2) = term(y), term(y2)
        l, wt = la * l1 + lb * l2, la * w1 + lb * w2
    loss = l.sum() / wt.sum() + 0.5 * alpha / mb * sum((v ** 2).sum() for v in W)
    loss.backward()
    out = {"logits": h.detach().numpy(), "loss": np.asarray(float(loss.detach()))}
    for i in range(L):
        out[f"gW{i}"] = W[i].grad.numpy() + 0.0
        out[f"gb{i}"] = b[i].grad.numpy() + 0.0
    # autograd differentiates 0.5 alpha / mb sum W^2 into (alpha / mb) W: the L2 term of dW
    return out


def _close(got, want, tol=1e-10):
    return float(np.max(np.abs(np.asarray(got) - want) / np.maximum(1.0, np.abs(want)))) <= tol


def test_checker_gradients_are_torch_autograd_with_the_masks_as_constants():
    for c in (rc.DROP_CASES[2], rc.DROP_CASES[7]):
        ws, bs, cw, X, y, masks = rc.make_drop_case(c)
        for seed in range(64):                                                # input dropout too: a seed that keeps the margin
            masks[0] = (rc.keep_mask(seed, c.step0, 0, rc.MB, c.dims[0], 0.25), 0.25)
            try:
                ref, _ = rc.step(ws, bs, X, y, rc.ALPHA, cw, masks, eps=c.eps)
                break
            except sr.MarginError:
                continue
        else:
            raise AssertionError("no input mask keeps the margin condition")
        want = _torch_step(ws, bs, X, y, rc.ALPHA, cw, masks, None, None, c.eps)
        assert set(ref) == set(want)
        for k in want:
            assert _close(ref[k], want[k]), (c.id, k)
    ws, bs, cw, X, y, visit, partner, lam, masks = rc.mixed_step_case()
    Xm = rc.mix_rows(X, visit, partner, lam[0])
    for eps in (0.0, 0.1):
        ref, _ = rc.step(ws, bs, Xm, y[visit], rc.ALPHA, cw, masks, y2=y[partner], lam=lam[0], eps=eps)
        want = _torch_step(ws, bs, Xm, y[visit], rc.ALPHA, cw, masks, y[partner], lam[0], eps)
        for k in want:
            assert _close(ref[k], want[k]), ("mixed", eps, k)


def _worst(got, ref, bound):
    return {k: sr.worst_ratio(got[k], ref[k], bound[k])[0] for k in ref}


@pytest.mark.parametrize("case", rc.DROP_CASES, ids=[c.id for c in rc.DROP_CASES])
def test_fp32_restatement_of_a_dropout_step_stays_within_one_bound(case):
    ws, bs, cw, X, y, masks = rc.make_drop_case(case)
    assert masks[0] is None and all(m is not None and not m[0].all() and m[0].any() for m in masks[1:])
    ref, bound = rc.step(ws, bs, X, y, rc.ALPHA, cw, masks, eps=case.eps)        # raises if the margin condition fails
    got = rc.emulate_step(ws, bs, X, y, rc.ALPHA, cw, masks, eps=case.eps)
    worst = _worst(got, ref, bound)
    print(case.id, {k: round(v, 4) for k, v in worst.items()})
    assert set(got) == set(ref) and max(worst.values()) <= 1.0, worst


def _mixed():
    ws, bs, cw, X, y, visit, partner, lam, masks = rc.mixed_step_case()
    return ws, bs, cw, X, rc.mix_rows(X, visit, partner, lam[0]), y[visit], y[partner], lam[0], masks


def test_fp32_restatement_of_the_mixed_step_stays_within_one_bound():
    ws, bs, cw, _, Xm, ya, yb, lam, masks = _mixed()
    assert (ya != yb).sum() > 30 and (cw == 0).sum() == 1
    ref, bound = rc.step(ws, bs, Xm, ya, rc.ALPHA, cw, masks, y2=yb, lam=lam)
    worst = _worst(rc.emulate_step(ws, bs, Xm, ya, rc.ALPHA, cw, masks, y2=yb, lam=lam), ref, bound)
    print({k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


FAULTS = ["mask ignored in backward", "scale missing", "counter built on a padded width", "step not advancing",
          "oml on the wrong target"]


@pytest.mark.parametrize("fault", FAULTS)
def test_wrong_steps_exceed_twice_the_bound(fault):
    ws, bs, cw, _, Xm, ya, yb, lam, masks = _mixed()
    dims = (70, 130, 65, 5)
    ref, bound = rc.step(ws, bs, Xm, ya, rc.ALPHA, cw, masks, y2=yb, lam=lam)
    wrong_masks, emu_fault = masks, None
    if fault == "counter built on a padded width":
        wrong_masks = rc.step_masks(rc.MASK_SEED, 1, dims, rc.MB, 0.0, 0.25, width=lambda n: -(-n // 64) * 64)
    elif fault == "step not advancing":
        wrong_masks = rc.step_masks(rc.MASK_SEED, 0, dims, rc.MB, 0.0, 0.25)
    else:
        emu_fault = fault
    got = rc.emulate_step(ws, bs, Xm, ya, rc.ALPHA, cw, wrong_masks, y2=yb, lam=lam, fault=emu_fault)
    over = {k: int((np.abs(got[k].astype(np.float64) - ref[k]) > 2.0 * bound[k]).sum()) for k in ref}
    print(fault, over)
    assert any(over.values()), f"the bound is too loose to catch: {fault}"
    if fault == "mask ignored in backward":
        assert over["logits"] == 0 and over["loss"] == 0 and over["gW2"] == 0 and over["gW0"] > 0     # the forward is right
    if fault == "oml on the wrong target":
        assert over["logits"] == 0 and over["gb2"] > 0


def test_mixed_loss_is_the_combination_of_the_checker():
    import loss_checker as lc
    rng = np.random.default_rng(11)
    z, ya = lc.logit_rows(rng, 24, 5, 4.0)
    yb = rng.integers(0, 5, size=24)
    w = lc.class_weights(rng, 5)
    yb[0] = ya[0] = int(np.flatnonzero(w > 0)[0])
    for lam, y_one in ((1.0, ya), (0.0, yb)):                             # lam = 1 / 0: the unmixed loss of one target
        grad, rows, bd, bl = rc.mixed_loss(z, ya, yb, lam, w, eps=0.1, gamma=2.0)
        want_g, want_r, _, _ = lc.checker(z, y_one, w, None, 0.1, 2.0)
        assert np.allclose(grad, want_g, rtol=1e-13, atol=1e-300) and np.allclose(rows, want_r, rtol=1e-13, atol=1e-300)
        one_d, one_l = lc.bounds(y_one, w, want_r)
        assert (bd >= one_d).all() and (bl >= one_l * (1 - 1e-12)).all() and (bd <= 1.5 * one_d).all()
    with pytest.raises(ZeroDivisionError):
        dead = int(np.flatnonzero(w == 0)[0])
        rc.mixed_loss(z[:2], [dead, dead], [dead, dead], 0.5, w)


# ---- c. the plan -----------------------------------------------------------------------------------------------------------------
def test_mixup_plan():
    import mermaid_classifier_amd as pkg
    from mermaid_classifier_amd import sampling
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    assert "mixup_plan" in sampling.__all__ and pkg.mixup_plan is sampling.mixup_plan and "mixup_plan" in pkg.__all__
    visit = np.random.default_rng(0).permutation(1000)[:164].astype(np.int64)
    partner, lam = sampling.mixup_plan(visit, 67, 0.2, np.random.default_rng([5, 0]))
    assert partner.dtype == np.int64 and partner.shape == (164,) and lam.dtype == np.float32 and lam.shape == (3,)
    for s in range(3):
        sl = slice(67 * s, 67 * s + 67)
        assert sorted(partner[sl].tolist()) == sorted(visit[sl].tolist())            # a permutation of its own mini-batch
    assert ((lam >= 0) & (lam <= 1)).all() and len(set(lam.tolist())) == 3 and (partner != visit).any()
    again = sampling.mixup_plan(visit, 67, 0.2, np.random.default_rng([5, 0]))
    assert np.array_equal(again[0], partner) and np.array_equal(again[1], lam)     # deterministic per seed
    other = sampling.mixup_plan(visit, 67, 0.2, np.random.default_rng([5, 1]))       # ... and another pass differs
    assert not np.array_equal(other[0], partner) and not np.array_equal(other[1], lam)
    p1, l1 = sampling.mixup_plan(visit[:5], 200, 1.0, np.random.default_rng(0))      # batch larger than the rows: one mini-batch
    assert l1.shape == (1,) and sorted(p1.tolist()) == sorted(visit[:5].tolist())
    for bad in (dict(visit=np.zeros((2, 2), np.int64)), dict(visit=np.zeros(0, np.int64)), dict(batch_size=0), dict(alpha=0.0),
                dict(alpha=float("nan")), dict(alpha=float("inf"))):
        args = dict(visit=visit, batch_size=67, alpha=0.2, rng=np.random.default_rng(0))
        args.update(bad)
        with pytest.raises(ValueError):
            sampling.mixup_plan(**args)
    # the classifier's plan: default_rng([seed, n_iter_])
    clf = TorchMLPClassifier(mixup_alpha=0.2, random_state=5)
    clf.n_iter_ = 0
    v, q, w = clf._mix_plan(visit, 164, 67)
    assert v is visit and np.array_equal(q, partner) and np.array_equal(w, lam)
    clf.n_iter_ = 1
    assert np.array_equal(clf._mix_plan(visit, 164, 67)[1], other[0])
    v, q, w = clf._mix_plan(None, 10, 4)                                            # no visiting order: the rows in stored order
    assert np.array_equal(v, np.arange(10)) and sorted(q[:4].tolist()) == [0, 1, 2, 3] and w.shape == (3,)
    assert TorchMLPClassifier()._mix_plan(None, 10, 4) == (None, None, None)


# ---- d. the Python surface -------------------------------------------------------------------------------------------------------
def test_classifier_and_sweep_config_regularizer_options():
    import mermaid_classifier_amd as pkg
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    clf = TorchMLPClassifier()
    assert (clf.dropout, clf.input_dropout, clf.mixup_alpha, clf.regularizer_seed) == (0.0, 0.0, 0.0, None)
    params = clf.get_params()
    assert [params[k] for k in ("dropout", "input_dropout", "mixup_alpha", "regularizer_seed")] == [0.0, 0.0, 0.0, None]
    for name in ("dropout", "input_dropout"):
        for bad in (-0.1, 0.91, 1.0, float("nan"), float("inf"), "0.1", None, True):
            with pytest.raises(ValueError, match=name):
                TorchMLPClassifier(**{name: bad})
        TorchMLPClassifier(**{name: 0.9})
    for bad in (-0.1, float("nan"), float("inf"), "0.2", None, True):
        with pytest.raises(ValueError, match="mixup_alpha"):
            TorchMLPClassifier(mixup_alpha=bad)
    for bad in (-1, 2 ** 64, 1.5, "7", True):
        with pytest.raises(ValueError, match="regularizer_seed"):
            TorchMLPClassifier(regularizer_seed=bad)
    with pytest.raises(TypeError):                                           # keyword only: no positional slot after `device`
        TorchMLPClassifier((8,), "relu", "adam", 1e-4, "auto", 1e-3, 200, True, 0, 1e-4, 0.9, 0.999, 1e-8, None, 0, 0.2)
    clf = TorchMLPClassifier(dropout=0.2, input_dropout=0.1, mixup_alpha=0.4, regularizer_seed=2 ** 64 - 1)
    assert clf.get_params() == dict(TorchMLPClassifier().get_params(), dropout=0.2, input_dropout=0.1, mixup_alpha=0.4,
                                    regularizer_seed=2 ** 64 - 1)
    clf.set_params(dropout=0.5, regularizer_seed=None)
    assert (clf.dropout, clf.regularizer_seed) == (0.5, None)
    with pytest.raises(ValueError, match="Invalid parameter"):
        clf.set_params(drop_out=0.5)
    # the seed: regularizer_seed, else random_state, else one draw that is kept
    assert TorchMLPClassifier(regularizer_seed=9, random_state=3)._regularizer_seed_value() == 9
    assert TorchMLPClassifier(random_state=3)._regularizer_seed_value() == 3
    free = TorchMLPClassifier()
    drawn = free._regularizer_seed_value()
    assert 0 <= drawn < 2 ** 64 and free._regularizer_seed_value() == drawn
    assert pickle.loads(pickle.dumps(free))._regularizer_seed_value() == drawn
    # mixup needs resident rows: the host-fed pass says where to go, before it looks at anything else
    with pytest.raises(ValueError, match="partial_fit_rows"):
        TorchMLPClassifier(mixup_alpha=0.2).partial_fit(np.zeros((4, 3), np.float32), [0, 1, 0, 1])
    with pytest.raises(ValueError, match="partial_fit_rows"):
        TorchMLPClassifier(mixup_alpha=0.2).fit(np.zeros((4, 3), np.float32), [0, 1, 0, 1])

    cfg = pkg.SweepConfig()
    assert (cfg.dropout, cfg.input_dropout, cfg.mixup_alpha, cfg.regularizer_seed) == (0.0, 0.0, 0.0, None)
    assert cfg.classifier().get_params() == TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), learning_rate_init=1e-4,
                                                               random_state=0).get_params()
    got = pkg.SweepConfig(hidden_layer_sizes=(8,), dropout=0.2, input_dropout=0.1, mixup_alpha=0.3, regularizer_seed=4).classifier("cuda:0")
    assert (got.dropout, got.input_dropout, got.mixup_alpha, got.regularizer_seed, got.device) == (0.2, 0.1, 0.3, 4, "cuda:0")
    with pytest.raises(ValueError, match="dropout"):
        pkg.SweepConfig(dropout=0.95).classifier()
    with pytest.raises(TypeError):                                           # keyword only here too: positional callers are undisturbed
        pkg.SweepConfig((8,), 1e-4, 1e-4, None, 0, "auto", 0.9, 0.999, 1e-8, None, 0.0, 0.0, None, 0.2)


def test_state_from_before_the_regularizers_loads_without_them():
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    new = ("dropout", "input_dropout", "mixup_alpha", "regularizer_seed")
    clf = TorchMLPClassifier(hidden_layer_sizes=(8,), dropout=0.2, input_dropout=0.1, mixup_alpha=0.3, regularizer_seed=7)
    twin = pickle.loads(pickle.dumps(clf))
    assert twin.get_params() == clf.get_params() and not twin._fitted()
    old = {k: v for k, v in clf.__getstate__().items() if k not in new}
    assert "label_smoothing" in old and not set(new) & set(old)
    back = TorchMLPClassifier.__new__(TorchMLPClassifier)
    back.__setstate__(dict(old))
    assert [getattr(back, k) for k in new] == [0.0, 0.0, 0.0, None]
    assert back.get_params() == TorchMLPClassifier(hidden_layer_sizes=(8,)).get_params() and not back._fitted()


# ---- e. the C ABI ----------------------------------------------------------------------------------------------------------------
def test_header_declares_and_symbols_list_the_new_entry_points():
    from mermaid_classifier_amd import _lib
    header = (ROOT / "include" / "mmc.h").read_text()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header and name in _lib.SYMBOLS, name
    assert "regularisers" in header and "0xD2511F53" in header and "0xBB67AE85" in header
    lib = _lib.lib()
    assert all(hasattr(lib, name) for name in NEW_SYMBOLS)
    readme = (ROOT / "README.md").read_text()
    assert "mixup" in readme and "mmc_trainer_set_dropout" in readme


def test_regularizer_c_abi_argument_errors_without_device():
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    fake = C.c_void_p(1234)          # never dereferenced: the calls below fail before the trainer is looked at
    assert lib.mmc_trainer_set_dropout(None, 0.1, 0.1, 0) == _lib.MMC_ERR_ARG
    assert b"NULL" in lib.mmc_last_error()
    for p in (-0.1, 0.9000001, 1.0, float("nan"), float("inf")):
        assert lib.mmc_trainer_set_dropout(fake, p, 0.0, 0) == _lib.MMC_ERR_ARG and b"p_input" in lib.mmc_last_error()
        assert lib.mmc_trainer_set_dropout(fake, 0.0, p, 0) == _lib.MMC_ERR_ARG and b"p_hidden" in lib.mmc_last_error()
    buf = (C.c_float * 6)()
    yb = (C.c_int32 * 2)(0, 1)
    assert lib.mmc_trainer_loss_gradient_mixed(None, buf, yb, yb, 0.5, 2, buf, buf, None) == _lib.MMC_ERR_ARG
    assert b"trainer handle is NULL" in lib.mmc_last_error()
    for args in ((None, yb, yb, 0.5, 2, buf, buf), (buf, None, yb, 0.5, 2, buf, buf), (buf, yb, None, 0.5, 2, buf, buf),
                 (buf, yb, yb, 0.5, 2, None, buf), (buf, yb, yb, 0.5, 2, buf, None)):
        assert lib.mmc_trainer_loss_gradient_mixed(fake, *args, None) == _lib.MMC_ERR_ARG
        assert b"NULL" in lib.mmc_last_error()
    for n in (0, -1, 16385):
        assert lib.mmc_trainer_loss_gradient_mixed(fake, buf, yb, yb, 0.5, n, buf, buf, None) == _lib.MMC_ERR_ARG
        assert b"outside [1, 16384]" in lib.mmc_last_error()
    for lam in (-0.01, 1.01, float("nan"), float("inf")):
        assert lib.mmc_trainer_loss_gradient_mixed(fake, buf, yb, yb, lam, 2, buf, buf, None) == _lib.MMC_ERR_ARG
        assert b"lam" in lib.mmc_last_error()
    assert lib.mmc_trainer_partial_fit_set_mixed(None, fake, None, None, None, 1, 1, None, None) == _lib.MMC_ERR_ARG
    assert lib.mmc_trainer_partial_fit_set_mixed(fake, None, None, None, None, 1, 1, None, None) == _lib.MMC_ERR_ARG
    assert lib.mmc_trainer_group_partial_fit_set_mixed(None, 1, fake, None, None, None, None, None, None, None) == _lib.MMC_ERR_ARG
