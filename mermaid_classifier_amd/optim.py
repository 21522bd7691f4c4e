"""Host mirrors of two definitions of include/mmc.h, "optimiser options", for planning a sweep without a device.

``lr_at`` is ``mmc_lr_schedule_at`` / ``mmc_trainer_lr_at``: the learning rate of the 1-based Adam step ``step``, in Python floats
(doubles), operation for operation as the C code has it.  The two ``cos`` implementations may differ in the last place, so the
cosine kind agrees with the library to a relative 1e-15, not to the bit; code that needs the trainer's own value asks the library.

``clip_coefficient`` is the fp32 arithmetic of ``gnorm_finalize_kernel`` on a given norm: what a step multiplies its gradient by.

``check_optimizer_options`` holds the argument checks that ``TorchMLPClassifier`` makes at construction; they mirror the C checks.

``fold_batch_norm`` is the host mirror of include/mmc.h, "batch normalisation": the Linear / ReLU stack that a normalised head is
with its statistics frozen (``bn_fold_kernel``'s definition, in the dtype of its inputs); ``check_batch_norm`` the argument checks
of ``mmc_trainer_set_batch_norm``.
"""

from __future__ import annotations

import math

import numpy as np

LR_KINDS = {"constant": 0, "linear": 1, "cosine": 2}   # the values of MMC_LR_CONSTANT / _LINEAR / _COSINE

__all__ = ["LR_KINDS", "lr_at", "clip_coefficient", "check_optimizer_options", "steps_per_epoch", "fold_batch_norm", "check_batch_norm"]


def _is_number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def check_optimizer_options(lr_schedule, warmup_steps, schedule_steps, final_lr_ratio, max_grad_norm, ema_decay) -> None:
    """``ValueError`` for what ``mmc_trainer_set_lr_schedule`` / ``_set_grad_clip`` / ``_set_ema`` would reject.  ``schedule_steps``
    may be None (filled in by ``train_classifier`` / ``train_sweep``, or required when the trainer is created); ``max_grad_norm`` None
    and ``ema_decay`` 0 are off."""
    if lr_schedule not in LR_KINDS:
        raise ValueError(f"lr_schedule must be one of {sorted(LR_KINDS)}, got {lr_schedule!r}.")
    if not _is_int(warmup_steps) or int(warmup_steps) < 0:
        raise ValueError(f"warmup_steps must be an integer >= 0, got {warmup_steps!r}.")
    if schedule_steps is not None:
        if not _is_int(schedule_steps) or int(schedule_steps) < 0:
            raise ValueError(f"schedule_steps must be None or an integer >= 0, got {schedule_steps!r}.")
        if lr_schedule != "constant" and not int(schedule_steps) > int(warmup_steps):
            raise ValueError(f"a decaying lr_schedule needs schedule_steps > warmup_steps, got {schedule_steps!r} and {warmup_steps!r}.")
    if not _is_number(final_lr_ratio) or not 0.0 <= float(final_lr_ratio) <= 1.0:
        raise ValueError(f"final_lr_ratio must lie in [0, 1], got {final_lr_ratio!r}.")
    if max_grad_norm is not None:
        ok = _is_number(max_grad_norm) and float(max_grad_norm) > 0.0 and math.isfinite(float(max_grad_norm))
        with np.errstate(over="ignore"):
            ok = ok and bool(np.isfinite(np.float32(max_grad_norm))) and float(np.float32(max_grad_norm)) > 0.0
        if not ok:
            raise ValueError(f"max_grad_norm must be None or a positive finite number (in float32 too), got {max_grad_norm!r}.")
    if not _is_number(ema_decay) or not (float(ema_decay) == 0.0 or 0.0 < float(ema_decay) < 1.0):
        raise ValueError(f"ema_decay must be 0 or lie in (0, 1), got {ema_decay!r}.")


def lr_at(step: int, lr: float, kind: str = "constant", warmup_steps: int = 0, total_steps: int = 0,
          final_ratio: float = 0.0) -> float:
    """Learning rate of the 1-based step ``step``: ``lr * w * d`` with the warm-up factor ``w`` and the decay ``d`` of include/mmc.h."""
    check_optimizer_options(kind, warmup_steps, total_steps, final_ratio, None, 0.0)
    s, wu = float(int(step)), float(int(warmup_steps))
    w = min(1.0, s / wu) if int(warmup_steps) > 0 else 1.0
    u = min(1.0, max(0.0, (s - wu) / float(max(1, int(total_steps) - int(warmup_steps)))))
    r = float(final_ratio)
    d = 1.0
    if kind == "linear":
        d = 1.0 - (1.0 - r) * u
    elif kind == "cosine":
        d = r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * u))
    return float(lr) * w * d


def clip_coefficient(norm, max_norm) -> np.float32:
    """``fminf(1.0f, max_norm / (norm + 1e-6f))`` in float32, one rounding per operation; a NaN norm gives NaN, an infinite one 0
    (``torch.nn.utils.clip_grad_norm_`` with ``error_if_nonfinite=False``)."""
    with np.errstate(invalid="ignore"):
        q = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return q if np.isnan(q) else min(np.float32(1.0), q)


def steps_per_epoch(batches, batch_size) -> int:
    """Adam steps of one epoch whose ``partial_fit_rows`` calls take the row arrays ``batches`` with the classifier's ``batch_size``
    ("auto": ``min(200, rows)``): the sum over the arrays of ``ceil(rows / mini-batch)``."""
    total = 0
    for rows in batches:
        n = len(rows)
        if n < 1:
            continue
        mb = min(200, n) if batch_size == "auto" else min(int(batch_size), n)
        total += -(-n // mb)
    return total


def check_batch_norm(batch_norm, batch_norm_eps, batch_norm_momentum) -> None:
    """``ValueError`` for what ``mmc_trainer_set_batch_norm`` would reject: ``batch_norm`` a bool, ``batch_norm_eps`` > 0 and finite (in
    float32 too), ``batch_norm_momentum`` in (0, 1]."""
    if not isinstance(batch_norm, (bool, np.bool_)):
        raise ValueError(f"batch_norm must be a bool, got {batch_norm!r}.")
    ok = _is_number(batch_norm_eps) and float(batch_norm_eps) > 0.0 and math.isfinite(float(batch_norm_eps))
    ok = ok and float(np.float32(batch_norm_eps)) > 0.0
    if not ok:
        raise ValueError(f"batch_norm_eps must be a positive finite number (in float32 too), got {batch_norm_eps!r}.")
    if not _is_number(batch_norm_momentum) or not 0.0 < float(batch_norm_momentum) <= 1.0:
        raise ValueError(f"batch_norm_momentum must lie in (0, 1], got {batch_norm_momentum!r}.")


def fold_batch_norm(weights, biases, gamma, beta, mean, var, eps):
    """The plain ``Linear -> ReLU -> ... -> Linear`` stack that equals ``Linear -> BatchNorm1d(eval) -> ReLU -> ... -> Linear``:
    for hidden layer l, ``s = gamma / sqrt(var + eps)``, ``W' = s[:, None] * W``, ``b' = beta + s * (b - mean)``; the last layer is
    returned as it is.  ``weights`` / ``biases`` hold every layer, the other four one array per hidden layer.  Computed in the dtype
    of the inputs (float32 in: ``bn_fold_kernel``'s operations, one rounding each; float64 in: the definition).  -> (weights, biases)"""
    weights, biases = [np.asarray(w) for w in weights], [np.asarray(b) for b in biases]
    hidden = len(weights) - 1
    if not (len(biases) == hidden + 1 and len(gamma) == len(beta) == len(mean) == len(var) == hidden):
        raise ValueError(f"{hidden + 1} layers need {hidden} arrays each of gamma, beta, mean and var.")
    ws, bs = [], []
    for l in range(hidden):
        w, b = weights[l], biases[l]
        dt = w.dtype.type
        g, be, mu, v = (np.asarray(a, dtype=w.dtype) for a in (gamma[l], beta[l], mean[l], var[l]))
        if not (g.shape == be.shape == mu.shape == v.shape == b.shape == (w.shape[0],)):
            raise ValueError(f"hidden layer {l}: gamma, beta, mean, var and the bias must each have {w.shape[0]} entries.")
        s = g / np.sqrt(v + dt(eps))
        ws.append(s[:, None] * w)
        bs.append(be + s * (b - mu))
    ws.append(weights[-1].copy())
    bs.append(biases[-1].copy())
    return ws, bs
