"""What tests/test_cover_host.py and tests/test_gpu_cover.py share: a numpy evaluation of the cover definition of include/mmc.h
("cover estimation": that text is the definition, this module follows it line by line), the label-shift recipe and a direct
restatement of the reference's compute_cover arithmetic.  Not a test module."""

import numpy as np


def usable_rows(v):
    """A point is usable when all K values are finite."""
    return np.isfinite(np.asarray(v, np.float32)).all(axis=1)


def cover(v, offsets, train_prior=None, strength=1.0, iters=20, dtype=np.float64):
    """-> (count (G, K) int64, soft_q32 (G, K) int64, unusable (G,) int64, prior (G, K) ``dtype``).  ``dtype`` is the type the EM
    runs in: float64 is the definition, np.longdouble shows how well the input is conditioned."""
    v = np.asarray(v, np.float32)
    n, K = v.shape
    offsets = np.asarray(offsets, np.int64)
    G = len(offsets) - 1
    tp = (np.full(K, 1.0 / K) if train_prior is None else np.asarray(train_prior, np.float64)).astype(dtype)
    ok = usable_rows(v)
    count = np.zeros((G, K), np.int64)
    soft = np.zeros((G, K), np.int64)
    unusable = np.zeros(G, np.int64)
    prior = np.zeros((G, K), dtype)
    for g in range(G):
        rows = slice(offsets[g], offsets[g + 1])
        use = v[rows][ok[rows]]
        unusable[g] = (~ok[rows]).sum()
        n_g = len(use)
        count[g] = np.bincount(use.argmax(axis=1), minlength=K) if n_g else 0          # the first maximum
        soft[g] = np.rint(use.astype(np.float64) * 4294967296.0).astype(np.int64).sum(axis=0)   # llrint: ties to even
        pi = tp.copy()
        for _ in range(iters):
            if n_g == 0:
                break                                                                    # keeps train_prior
            pi = (posterior(use, pi / tp, dtype).sum(axis=0) + dtype(strength) * tp) / (dtype(n_g) + dtype(strength))
        prior[g] = pi
    return count, soft, unusable, prior


def posterior(v, w, dtype=np.float64):
    """q of every row of ``v`` under the weights ``w``: tq = (double)v * w, Z = sum tq, q = tq / Z when Z is finite and > 0,
    otherwise q = (double)v."""
    vd = np.asarray(v, np.float32).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        tq = vd * np.asarray(w, dtype)
        Z = tq.sum(axis=1)
        good = np.isfinite(Z) & (Z > 0)
        q = np.where(good[:, None], tq / np.where(good, Z, 1)[:, None], vd)
    return q


def adapted_topk(v, offsets, prior, train_prior, k):
    """-> (idx (n, k) int32, scores (n, k) float32, all (n, K) float32 scores): score = (float)q under w = prior[g] / train_prior,
    ordered by the key rule of mmc_head_topk: the fp32 bit pattern descending, equal scores in class order."""
    v = np.asarray(v, np.float32)
    n, K = v.shape
    offsets = np.asarray(offsets, np.int64)
    tp = np.full(K, 1.0 / K) if train_prior is None else np.asarray(train_prior, np.float64)
    scores = np.empty((n, K), np.float32)
    for g in range(len(offsets) - 1):
        rows = slice(offsets[g], offsets[g + 1])
        with np.errstate(invalid="ignore", over="ignore"):
            scores[rows] = posterior(v[rows], np.asarray(prior[g], np.float64) / tp).astype(np.float32)
    bad = ~usable_rows(v)
    scores[bad] = v[bad]                                                                 # q = (double)v, back to its own bits
    key = (scores.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(K, dtype=np.uint64))
    order = np.argsort(key, axis=1, kind="stable")[:, ::-1][:, :k]
    return order.astype(np.int32), np.take_along_axis(scores, order, 1), scores


def ulp_distance(a, b):
    """Units in the last place between two float32 arrays of non-negative finite numbers."""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def prior_atol(iters, n_max):
    """A device M-step sums at most n_max terms in [0, 1] in another order and with contracted FMAs: 64 * max(iters, 1) * n_max *
    2^-53, the 64 being margin for amplification across iterations."""
    return 64.0 * max(int(iters), 1) * int(n_max) * 2.0 ** -53


# ---- the label-shift recipe ----

def mixture_trials(trials=8, K=6, d=2, n=2000, seed=11):
    """-> (v (trials * n, K) float32: the exact posterior of a Gaussian mixture under the uniform train prior, y (trials * n,) the
    drawn classes, offsets): every trial draws its own class frequencies from Dirichlet(0.5)."""
    rng = np.random.default_rng(seed)
    mu = rng.normal(0, 1.6, (K, d))
    vs, ys = [], []
    for _ in range(trials):
        true = rng.dirichlet(np.full(K, .5))
        y = rng.choice(K, n, p=true)
        x = mu[y] + rng.normal(0, 1, (n, d))
        logp = -0.5 * ((x[:, None, :] - mu[None]) ** 2).sum(-1)
        logp -= logp.max(axis=1, keepdims=True)
        p = np.exp(logp)
        vs.append((p / p.sum(axis=1, keepdims=True)).astype(np.float32))
        ys.append(y)
    return np.concatenate(vs), np.concatenate(ys), np.arange(trials + 1, dtype=np.int64) * n


def label_shift_l1(count, soft_q32, prior, y, offsets):
    """Per group the L1 distance to the empirical class frequencies of (hard cover, soft cover, adapted prior)."""
    K = count.shape[1]
    out = []
    for g in range(len(offsets) - 1):
        yy = y[offsets[g]:offsets[g + 1]]
        emp = np.bincount(yy, minlength=K) / len(yy)
        n_g = count[g].sum()
        out.append((np.abs(count[g] / n_g - emp).sum(), np.abs(soft_q32[g] / 4294967296.0 / n_g - emp).sum(),
                    np.abs(np.asarray(prior[g], np.float64) - emp).sum()))
    return np.asarray(out)


# ---- compute_cover, restated ----

def reference_cover_metrics(true_cover, pred_cover):
    """mermaid_classifier/pyspacer/metrics/cover.py:62-120 on (n_images, K) cover fractions, with numpy alone -> (table columns by
    mean true cover descending, for the classes that occur; the four scalars)."""
    t, p = np.asarray(true_cover, np.float64), np.asarray(pred_cover, np.float64)
    keep = np.flatnonzero((t.sum(0) > 0) | (p.sum(0) > 0))
    t, p = t[:, keep], p[:, keep]
    err = p - t
    r2 = np.full(len(keep), np.nan)
    for i in range(len(keep)):
        if t[:, i].std() > 0:
            r2[i] = 1.0 - ((t[:, i] - p[:, i]) ** 2).sum() / ((t[:, i] - t[:, i].mean()) ** 2).sum()   # sklearn r2_score
    cols = {"class": keep, "mean_true_cover_pct": t.mean(0) * 100, "bias_pct": err.mean(0) * 100,
            "rmse_pct": np.sqrt((err ** 2).mean(0)) * 100, "mae_pct": np.abs(err).mean(0) * 100, "r_squared": r2}
    order = np.argsort(-cols["mean_true_cover_pct"], kind="stable")
    cols = {k: v[order] for k, v in cols.items()}
    sig = cols["mean_true_cover_pct"] > 0.5
    names = ("cover_mean_abs_bias_pct", "cover_mean_rmse_pct", "cover_mean_mae_pct", "cover_median_r_squared")
    if not sig.any():
        return cols, dict.fromkeys(names, 0.0)
    r = cols["r_squared"][sig]
    r = r[~np.isnan(r)]
    return cols, {names[0]: float(np.abs(cols["bias_pct"][sig]).mean()), names[1]: float(cols["rmse_pct"][sig].mean()),
                  names[2]: float(cols["mae_pct"][sig].mean()), names[3]: float(np.median(r)) if len(r) else float("nan")}
