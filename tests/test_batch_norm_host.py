"""Batch normalisation in the MLP trainer without a device (include/mmc.h, "batch normalisation"):

a. the float64 definition of tests/batch_norm_checker.py is ``torch.nn.BatchNorm1d`` in float64 plus autograd on every case of the
   GPU file, the fp32 numpy evaluation in the kernels' order stays within half of each bound, and four deliberately wrong variants
   each miss a bound by orders of magnitude;
b. ``fold_batch_norm`` followed by a plain Linear / ReLU forward is the eval-mode forward, and the checker's fold bounds hold for fp32;
c. the numpy training step is torch's in float64, and the torch fp32 and fp64 loops of the GPU file's training recipe differ by under
   a tenth of its tolerances;
d. the Python surface: constructor, ``get_params`` / ``set_params``, pickles from before the option, ``SweepConfig``, the errors;
e. the header declares the entry points, ``_lib.SYMBOLS`` lists them, and they reject bad arguments without a device;
f. a float64 recipe: a three-hidden-layer head at ``lr=1e-3`` and ``1e-2``, plain against normalised, several seeds -- it prints what
   happens and asserts only that the runs are what they claim to be."""

import ctypes as C
import pickle
import re
from pathlib import Path

import numpy as np
import pytest

import batch_norm_checker as ck

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["mmc_trainer_set_batch_norm", "mmc_trainer_batch_norm_state", "mmc_trainer_folded_params", "mmc_trainer_norm_stage"]
CASES = [(M, N) for M in ck.MBS for N in ck.NS]
WRONG = ["unbiased_normaliser", "biased_running", "dropped_term", "one_pass"]


# ---- a. the stage ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", CASES)
def test_checker_is_torch_batchnorm1d_in_float64(M, N):
    import torch
    import torch.nn.functional as F
    Z, dA, gamma, beta, rm, rv = ck.stage_case(M, N)
    want, _ = ck.stage_ref(Z, dA, gamma, beta, rm, rv)
    sc = {k: float(v) for k, v in ck.scalars(M).items()}
    z = torch.tensor(Z, dtype=torch.float64, requires_grad=True)
    g = torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    trm, trv = torch.tensor(rm, dtype=torch.float64), torch.tensor(rv, dtype=torch.float64)
    a = F.batch_norm(z, trm, trv, g, b, training=True, momentum=sc["mom"], eps=sc["eps"])
    H = torch.relu(a)
    # dA is the gradient w.r.t. gamma xhat + beta, whatever the ReLU did before it
    a.backward(torch.tensor(dA, dtype=torch.float64))
    scale = lambda x: 1e-12 * (1.0 + np.abs(x).max())
    assert np.abs(H.detach().numpy() - want["H"]).max() <= scale(want["H"])
    assert np.abs(z.grad.numpy() - want["dZ"]).max() <= 1e-11 * (1.0 + np.abs(want["dZ"]).max())   # the stiff column: rstd 10, M dA - ... cancels
    assert np.abs(g.grad.numpy() - want["g_gamma"]).max() <= 1e-10 * (1.0 + np.abs(want["g_gamma"]).max())
    assert np.abs(b.grad.numpy() - want["g_beta"]).max() <= scale(want["g_beta"])
    assert np.abs(z.detach().numpy().mean(axis=0) - want["mu"]).max() <= scale(want["mu"])
    assert np.abs(z.detach().numpy().var(axis=0) - want["v"]).max() <= scale(want["v"])
    # torch forms 1 - momentum in double; the kernel's scalar is the float of it: 3e-8 relative apart
    assert np.abs(trm.numpy() - want["rm"]).max() <= 1e-7 * (1.0 + np.abs(want["rm"]).max())
    assert np.abs(trv.numpy() - want["rv"]).max() <= 1e-7 * (1.0 + np.abs(want["rv"]).max())
    if N >= 7:
        assert want["v"][ck.CONST_COL] == 0.0 and (want["H"][:, ck.DEAD_COL] == 0.0).all()
        assert 0.003 < want["v"][ck.STIFF_COL] < 0.03 or M < 100      # deviation 0.1: v near 0.01 once there are rows enough


@pytest.mark.parametrize("M,N", CASES)
def test_fp32_in_kernel_order_within_half_a_bound_and_wrong_variants_far_outside(M, N):
    case = ck.stage_case(M, N)
    want, bound = ck.stage_ref(*case)
    got = ck.stage_fp32(*case)
    peaks = {k: ck.peak(got[k], want[k], bound[k]) for k in want}
    print(f"mb {M:3d} N {N:3d} fp32 peak / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in peaks.items()))
    assert all(np.isfinite(a).all() for a in got.values())
    assert max(peaks.values()) <= 0.5, peaks
    if N >= 7:
        assert got["v"][ck.CONST_COL] < 1e-12 and abs(got["v"][ck.STIFF_COL] / want["v"][ck.STIFF_COL] - 1.0) < 1e-3
    for wrong in WRONG:
        bad = ck.stage_fp32(*case, wrong=wrong)
        if wrong == "one_pass":
            if N < 7:
                continue                                   # the stiff column is what a one-pass variance cannot do
            worst = ck.peak(bad["v"][ck.STIFF_COL], want["v"][ck.STIFF_COL], bound["v"][ck.STIFF_COL])
        else:
            worst = max(ck.peak(bad[k], want[k], bound[k]) for k in want)
        print(f"    {wrong:20s} {worst:.1e} x bound")
        assert worst >= 100.0, (wrong, worst)


# ---- b. the fold -----------------------------------------------------------------------------------------------------------------
def _random_head(rng, dims, dtype):
    ws = [rng.normal(0, 0.3, (o, i)).astype(dtype) for i, o in zip(dims[:-1], dims[1:])]
    bs = [rng.normal(0, 0.3, o).astype(dtype) for o in dims[1:]]
    hidden = dims[1:-1]
    gamma = [rng.uniform(0.5, 1.5, n).astype(dtype) * rng.choice([-1, 1], n).astype(dtype) for n in hidden]
    beta = [rng.normal(0, 0.5, n).astype(dtype) for n in hidden]
    rm = [rng.normal(0, 1.0, n).astype(dtype) for n in hidden]
    rv = [rng.uniform(0.01, 2.0, n).astype(dtype) for n in hidden]
    return ws, bs, gamma, beta, rm, rv


def test_fold_then_plain_forward_is_the_eval_mode_forward():
    import torch
    import torch.nn as nn
    from mermaid_classifier_amd import fold_batch_norm
    rng = np.random.default_rng(5)
    dims = [16, 24, 12, 7]
    ws, bs, gamma, beta, rm, rv = _random_head(rng, dims, np.float64)
    eps = 1e-5
    mods = []
    for l, (w, b) in enumerate(zip(ws, bs)):
        lin = nn.Linear(w.shape[1], w.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(b))
        mods.append(lin)
        if l < len(ws) - 1:
            bn = nn.BatchNorm1d(w.shape[0], eps=eps).double()
            with torch.no_grad():
                bn.weight.copy_(torch.from_numpy(gamma[l]))
                bn.bias.copy_(torch.from_numpy(beta[l]))
                bn.running_mean.copy_(torch.from_numpy(rm[l]))
                bn.running_var.copy_(torch.from_numpy(rv[l]))
            mods += [bn, nn.ReLU()]
    X = rng.normal(0, 1, (33, 16))
    want = nn.Sequential(*mods).eval()(torch.from_numpy(X)).detach().numpy()
    fw, fb = fold_batch_norm(ws, bs, gamma, beta, rm, rv, eps)
    h = X
    for l, (w, b) in enumerate(zip(fw, fb)):
        h = h @ w.T + b
        if l < len(fw) - 1:
            h = np.maximum(h, 0)
    assert np.abs(h - want).max() <= 1e-12 * (1 + np.abs(want).max())
    assert np.array_equal(fw[-1], ws[-1]) and np.array_equal(fb[-1], bs[-1])
    with pytest.raises(ValueError, match="arrays each"):
        fold_batch_norm(ws, bs, gamma[:1], beta, rm, rv, eps)


def test_fp32_fold_within_half_the_checkers_bound():
    from mermaid_classifier_amd import fold_batch_norm
    rng = np.random.default_rng(6)
    state = _random_head(rng, [16, 65, 300, 7], np.float32)
    ws, bs, ews, ebs = ck.fold_ref(*state)
    for got_w, got_b in (ck.fold_fp32(*state), fold_batch_norm(*state, 1e-5)):
        assert all(a.dtype == np.float32 for a in got_w + got_b)
        peaks = [max(ck.peak(got_w[l], ws[l], ews[l]), ck.peak(got_b[l], bs[l], ebs[l])) for l in range(3)]
        print("fp32 fold peak / bound per layer:", [f"{p:.3f}" for p in peaks])
        assert max(peaks) <= 0.5


# ---- c. the training step ----------------------------------------------------------------------------------------------------------
def test_numpy_step_is_torchs_in_float64():
    import torch
    data = ck.train_data()
    want = ck.torch_loop(data, torch.float64, passes=2, lr=1e-2)
    w0, b0 = ck.initial_parameters()
    net = ck.NumpyNet(w0, b0, True, lr=1e-2, alpha=1e-3)
    order = np.arange(ck.NROWS)
    np.random.default_rng(0).shuffle(order)
    X, y = data["X"][order], data["y"][order]
    curve = []
    for _ in range(2):
        tot = 0.0
        for s in range(0, ck.NROWS, ck.BATCH):
            tot += net.step(X[s:s + ck.BATCH], y[s:s + ck.BATCH]) * len(y[s:s + ck.BATCH])
        curve.append(tot / ck.NROWS)
    got = dict(curve=curve, W=net.W, b=net.b, gamma=net.gamma, beta=net.beta, rm=net.rm, rv=net.rv)
    dw, dl = ck.train_gap(got, want)
    print(f"numpy fp64 step against torch fp64: parameters {dw:.1e}, loss curve {dl:.1e}")
    assert dw <= 1e-9 and dl <= 1e-11
    assert all(np.array_equal(b, np.zeros_like(b)) for b in net.b[:-1])          # frozen


@pytest.mark.parametrize("lr", [1e-3, 1e-2])
@pytest.mark.parametrize("kind", list(ck.TRAIN_KINDS))
def test_torch_fp32_and_fp64_loops_differ_by_under_a_tenth_of_the_tolerances(kind, lr):
    import torch
    data = ck.train_data()
    a = ck.torch_loop(data, torch.float32, lr=lr, **ck.TRAIN_KINDS[kind])
    b = ck.torch_loop(data, torch.float64, lr=lr, **ck.TRAIN_KINDS[kind])
    dw, dl = ck.train_gap(a, b)
    print(f"{kind} lr {lr:g}: torch fp32 against fp64: parameters {dw:.1e}, loss curve {dl:.1e}")
    assert dw <= ck.W_TOL / 10 and dl <= ck.LOSS_TOL / 10


# ---- d. the Python surface -----------------------------------------------------------------------------------------------------------
def test_constructor_params_pickle_defaults_and_sweep_config():
    from mermaid_classifier_amd import SweepConfig
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    clf = TorchMLPClassifier()
    p = clf.get_params()
    assert (p["batch_norm"], p["batch_norm_eps"], p["batch_norm_momentum"]) == (False, 1e-5, 0.1)
    clf = TorchMLPClassifier(hidden_layer_sizes=(8, 4), batch_norm=True, batch_norm_eps=1e-3, batch_norm_momentum=0.2)
    p = clf.get_params()
    assert (p["batch_norm"], p["batch_norm_eps"], p["batch_norm_momentum"]) == (True, 1e-3, 0.2)
    assert TorchMLPClassifier(**p).get_params() == p
    assert clf.set_params(batch_norm_momentum=0.5).batch_norm_momentum == 0.5
    for bad in (dict(batch_norm=1), dict(batch_norm="yes"), dict(batch_norm_eps=0.0), dict(batch_norm_eps=-1e-5),
                dict(batch_norm_eps=float("nan")), dict(batch_norm_eps=1e-60), dict(batch_norm_eps=True), dict(batch_norm_momentum=0.0),
                dict(batch_norm_momentum=1.5), dict(batch_norm_momentum=float("nan")), dict(batch_norm_momentum=None)):
        with pytest.raises(ValueError, match="batch_norm"):
            TorchMLPClassifier(**bad)
    with pytest.raises(RuntimeError, match="not fitted"):
        clf.batch_norm_state()
    # a pickle from before the option loads as a plain head
    state = TorchMLPClassifier().__getstate__()
    for key in ("batch_norm", "batch_norm_eps", "batch_norm_momentum"):
        del state[key]
    old = TorchMLPClassifier.__new__(TorchMLPClassifier)
    old.__setstate__(state)
    assert (old.batch_norm, old.batch_norm_eps, old.batch_norm_momentum) == (False, 1e-5, 0.1)
    twin = pickle.loads(pickle.dumps(clf))
    assert twin.get_params() == clf.get_params()
    cfg = SweepConfig(hidden_layer_sizes=(8, 4), learning_rate_init=1e-3, batch_norm=True, batch_norm_eps=1e-4, batch_norm_momentum=0.3)
    made = cfg.classifier().get_params()
    assert (made["batch_norm"], made["batch_norm_eps"], made["batch_norm_momentum"], made["learning_rate_init"]) == (True, 1e-4, 0.3, 1e-3)
    assert SweepConfig().classifier().get_params()["batch_norm"] is False
    with pytest.raises(TypeError):
        SweepConfig((8,), 1e-3, 1e-4, None, 0, "auto", 0.9, 0.999, 1e-8, None, 0.0, 0.0, None, True)   # keyword only


# ---- e. the C ABI --------------------------------------------------------------------------------------------------------------------
def test_header_binding_documents_and_source_carry_the_entry_points():
    header = (ROOT / "include" / "mmc.h").read_text()
    binding = (ROOT / "mermaid_classifier_amd" / "_lib.py").read_text()
    listed = re.search(r"SYMBOLS = \[(.*?)\n\]", binding, re.S).group(1)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert f'"{name}"' in listed and f"lib.{name}.argtypes" in binding, name
        assert name in (ROOT / "INTEGRATION.md").read_text(), name
    assert "batch normalisation" in header
    source = (ROOT / "mermaid_classifier_amd" / "csrc" / "trainer.hip").read_text()
    for kernel in ("bn_forward_kernel", "bn_backward_kernel", "bn_fold_kernel"):
        assert re.search(rf"__global__ [^\n]*void {kernel}\(", source), kernel
        assert kernel in (ROOT / "DESIGN.md").read_text(), kernel
    assert "sizeof(BnFwdGroup) <= 4096" in source
    readme = (ROOT / "README.md").read_text()
    assert "mmc_trainer_set_batch_norm" in readme and "batch_norm=True" in readme


def test_c_abi_argument_errors_without_device():
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    assert all(hasattr(lib, name) for name in NEW_SYMBOLS)
    fp = C.POINTER(C.c_float)
    empty = (fp * 0)()
    assert lib.mmc_trainer_set_batch_norm(None, 1, 1e-5, 0.1) == _lib.MMC_ERR_ARG and b"NULL" in lib.mmc_last_error()
    assert lib.mmc_trainer_batch_norm_state(None, 0, *([empty] * 8)) == _lib.MMC_ERR_ARG and b"NULL" in lib.mmc_last_error()
    assert lib.mmc_trainer_folded_params(None, empty, empty) == _lib.MMC_ERR_ARG
    assert lib.mmc_trainer_norm_stage(None, 0, None, None, 2, None, None, None, None, None, None, None) == _lib.MMC_ERR_ARG
    assert b"trainer handle is NULL" in lib.mmc_last_error()


# ---- f. the recipe -----------------------------------------------------------------------------------------------------------------------
def recipe(lrs=(1e-3, 1e-2), seeds=(0, 1, 2), epochs=12, hidden=(64, 48, 32), n=600, dim=32, K=10, batch=50, report=print):
    """A three-hidden-layer head on a synthetic set in float64 (tests/batch_norm_checker.py's ``NumpyNet``), plain against normalised.
    Reports, per rate and seed, the largest jump of the epoch loss (a spike: an epoch loss above 1.5 x the one before), whether the
    run ends finite, the final train loss and the held-out accuracy.  -> the rows."""
    rows = []
    for lr in lrs:
        for seed in seeds:
            rng = np.random.default_rng([seed, 99])
            centres = rng.normal(0, 1.0, (K, dim))
            y = rng.integers(0, K, 2 * n)
            X = centres[y] * 0.7 + rng.normal(0, 1.0, (2 * n, dim))
            X[:, :4] *= 30.0                                   # badly scaled inputs: what a deep plain head at a large step dislikes
            Xt, yt, Xv, yv = X[:n], y[:n], X[n:], y[n:]
            dims = [dim, *hidden, K]
            w0 = [rng.uniform(-1, 1, (o, i)) * np.sqrt(6.0 / (i + o)) for i, o in zip(dims[:-1], dims[1:])]
            b0 = [np.zeros(o) for o in dims[1:]]
            for bn in (False, True):
                net = ck.NumpyNet(w0, b0, bn, lr=lr, alpha=1e-4)
                curve = []
                with np.errstate(all="ignore"):
                    for epoch in range(epochs):
                        order = np.random.default_rng([seed, epoch]).permutation(n)
                        tot = 0.0
                        for s in range(0, n, batch):
                            idx = order[s:s + batch]
                            tot += net.step(Xt[idx], yt[idx]) * len(idx)
                        curve.append(tot / n)
                    acc = float((net.forward_eval(Xv).argmax(axis=1) == yv).mean())
                c = np.asarray(curve)
                spike = float(np.nanmax(c[1:] / c[:-1])) if np.isfinite(c).all() else float("inf")
                rows.append(dict(lr=lr, seed=seed, batch_norm=bn, finite=bool(np.isfinite(c).all()), spike=spike, final=float(c[-1]), acc=acc))
                report(f"lr {lr:g} seed {seed} {'normalised' if bn else 'plain     '}: finite {rows[-1]['finite']}  largest epoch-loss ratio "
                       f"{spike:5.2f}  final train loss {c[-1]:.4f}  held-out accuracy {acc:.3f}")
    return rows


def test_recipe_plain_against_normalised_reports_what_happens():
    rows = recipe(seeds=(0, 1), epochs=6)
    assert len(rows) == 8 and {r["batch_norm"] for r in rows} == {False, True}
    assert all(r["finite"] for r in rows if r["batch_norm"])        # the normalised runs end finite; nothing is claimed of the rest
