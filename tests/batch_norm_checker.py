"""What tests/test_batch_norm_host.py and tests/test_gpu_batch_norm.py share: the float64 definition of batch normalisation in the MLP
trainer (include/mmc.h, "batch normalisation": the stage, the running statistics, the fold, the training step), the per-element bounds,
a numpy fp32 evaluation in ``bn_forward_kernel`` / ``bn_backward_kernel`` / ``bn_fold_kernel``'s order of operations with the
deliberately wrong variants, the cases both files run, and the torch training loop both compare against.  Not a test module.

The definition, per column j of Z [M][N], in float64 on the fp32 inputs::

    mu = mean_m Z;  v = mean_m (Z - mu)^2;  rstd = 1 / sqrt(v + eps);  xhat = (Z - mu) rstd;  H = relu(gamma xhat + beta)
    g_beta = sum_m dA;  g_gamma = sum_m dA xhat;  dZ = (gamma rstd / M) (M dA - g_beta - xhat g_gamma)
    rm' = om rm + mom mu;  rv' = om rv + mom v unb            eps, mom, om = 1 - mom, unb = M / (M - 1): the floats of the doubles
    s = gamma / sqrt(rv + eps);  W' = s W;  b' = beta + s (b - rm)

Bounds, per element, first order in ULP = 2^-23, counted from the kernels' operations and relative to the sum of the magnitudes of the
terms of every sum.  Every fp32 operation is allowed one ulp of its result, 2^-23 relative: what a faithfully rounded operation needs,
so the bounds do not lean on the device dividing and taking square roots correctly rounded, and twice what a correctly rounded one
needs -- which is why the numpy evaluation below, whose operations all are, stays within half of every bound.  A column sum adds its M
terms on four chains in each of four row quarters and combines chains and quarters pairwise, so a term passes through at most
``D(M) = ceil(ceil(M / 4) / 4) + 4`` rounded additions: a sum errs by D ULP sum|terms|.

* ``mu``: the sum and the division: ``E_mu = (D + 1) ULP mean|Z|``.
* ``v``: with e = mu - mu_hat the kernel sums fl((Z - mu_hat)^2); sum_m (Z - mu) e vanishes exactly, so the mean of the exact squares
  is v + e^2.  The subtraction (twice in the square), the product, the sum and the division give
  ``E_v = E_mu^2 + (D + 4) ULP (v + E_mu^2)``.
* ``rstd``: the addition of eps, the square root (which halves the relative error of its argument), the reciprocal:
  relative ``rho = E_v / (2 (v + eps)) + 2.5 ULP``.
* ``xhat = fl(fl(Z - mu_hat) rstd_hat)``: ``E_x = E_mu rstd + |xhat| (rho + 2 ULP)``.
* ``H``: relu is 1-Lipschitz, so H errs as a = fl(fl(gamma xhat) + beta): ``E_H = |gamma| E_x + ULP |gamma xhat| + ULP |a|``.
* ``g_beta``: ``D ULP sum|dA|``.   ``g_gamma``: ``E_gg = sum_m |dA| (E_x + ULP |xhat|) + D ULP sum_m |dA xhat|``.
* ``dZ = fl(k t)``, k = fl(fl(gamma rstd) / M) (relative rho + 2 ULP), t = fl(fl(fl(M dA) - g_beta) - fl(xhat g_gamma)):
  ``E_dZ = |k| (E_gb + 2 ULP |M dA| + ULP |M dA - g_beta| + |g_gamma| E_x + |xhat| E_gg + ULP |xhat g_gamma| + ULP |t|) + |dZ| (rho + 3 ULP)``.
* running statistics: ``E_rm = mom E_mu + ULP (|om rm| + |mom mu| + |rm'|)``,
  ``E_rv = mom unb E_v + ULP (|om rv| + 2 |mom v unb| + |rv'|)``.
* fold (its inputs are exact): s is an addition, a square root and a division, relative 2.5 ULP;
  ``E_W' = 3.5 ULP |W'|``,  ``E_b' = 4.5 ULP |s (b - rm)| + ULP |b'|``.

The bound on ``v`` of a column of mean 1000 and deviation 0.1 is a few 1e-4 of v; a one-pass E[z^2] - mu^2 in fp32 is a multiple of
2^-4 there (the spacing of fp32 at 1e6) and comes out negative as often as not."""

import math

import numpy as np

ULP = 2.0 ** -23
F32 = np.float32
W_TOL, LOSS_TOL = 2e-5, 1e-5          # tests/test_trainer.py

MBS, NS = (2, 5, 203, 259), (1, 7, 64, 65, 300)
CONST_COL, STIFF_COL, DEAD_COL = 0, 1, 2      # the special columns of every case with N >= 7


def depth(M):
    return math.ceil(math.ceil(M / 4) / 4) + 4


def scalars(M, eps=1e-5, mom=0.1):
    """The kernel's fp32 scalars, each the float of a double expression."""
    return dict(eps=F32(eps), mom=F32(mom), om=F32(1.0 - mom), unb=F32(M / (M - 1.0)))


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def stage_case(M, N, seed=0):
    """Z, dA [M][N], gamma, beta, rm, rv [N] in fp32.  With N >= 7: column 0 is constant, column 1 has mean 1000 and deviation 0.1,
    and column 2's gamma xhat + beta is negative everywhere (|xhat| <= sqrt(M - 1) < 17 for M <= 259, gamma 0.5, beta -10)."""
    rng = np.random.default_rng([M, N, seed])
    Z = (rng.normal(0.0, 1.0, (M, N)) * rng.uniform(0.2, 3.0, N) + rng.normal(0.0, 1.0, N)).astype(F32)
    dA = (rng.normal(0.0, 1.0, (M, N)) * (rng.random((M, N)) < 0.6)).astype(F32) / F32(M)     # a masked gradient: exact zeros
    gamma = rng.uniform(0.5, 1.5, N).astype(F32) * np.where(rng.random(N) < 0.2, -1, 1).astype(F32)
    beta = rng.normal(0.0, 0.5, N).astype(F32)
    rm = rng.normal(0.0, 1.0, N).astype(F32)
    rv = rng.uniform(0.5, 2.0, N).astype(F32)
    if N >= 7:
        Z[:, CONST_COL] = F32(0.3)
        Z[:, STIFF_COL] = (1000.0 + 0.1 * rng.normal(0.0, 1.0, M)).astype(F32)
        gamma[DEAD_COL], beta[DEAD_COL] = F32(0.5), F32(-10.0)
    return Z, dA, gamma, beta, rm, rv


# ---- the definition and its bounds ----------------------------------------------------------------------------------------------
def stage_ref(Z, dA, gamma, beta, rm, rv, eps=1e-5, mom=0.1):
    """-> (values, bounds): two dicts of float64 arrays keyed mu, v, H, g_beta, g_gamma, dZ, rm, rv."""
    Z, dA, gamma, beta, rm, rv = (np.asarray(a, np.float64) for a in (Z, dA, gamma, beta, rm, rv))
    M = Z.shape[0]
    sc = {k: float(x) for k, x in scalars(M, eps, mom).items()}
    D = depth(M)
    mu = Z.mean(axis=0)
    d = Z - mu
    v = (d * d).mean(axis=0)
    rstd = 1.0 / np.sqrt(v + sc["eps"])
    xh = d * rstd
    a = gamma * xh + beta
    H = np.maximum(a, 0.0)
    gb = dA.sum(axis=0)
    gg = (dA * xh).sum(axis=0)
    k = gamma * rstd / M
    t = M * dA - gb - xh * gg
    dZ = k * t
    rm2 = sc["om"] * rm + sc["mom"] * mu
    rv2 = sc["om"] * rv + sc["mom"] * v * sc["unb"]
    E_mu = (D + 1) * ULP * np.abs(Z).mean(axis=0)
    E_v = E_mu ** 2 + (D + 4) * ULP * (v + E_mu ** 2)
    rho = E_v / (2.0 * (v + sc["eps"])) + 2.5 * ULP
    E_x = E_mu * rstd + np.abs(xh) * (rho + 2 * ULP)
    E_H = np.abs(gamma) * E_x + ULP * np.abs(gamma * xh) + ULP * np.abs(a)
    E_gb = D * ULP * np.abs(dA).sum(axis=0)
    E_gg = (np.abs(dA) * (E_x + ULP * np.abs(xh))).sum(axis=0) + D * ULP * np.abs(dA * xh).sum(axis=0)
    E_dZ = np.abs(k) * (E_gb + 2 * ULP * np.abs(M * dA) + ULP * np.abs(M * dA - gb) + np.abs(gg) * E_x + np.abs(xh) * E_gg
                        + ULP * np.abs(xh * gg) + ULP * np.abs(t)) + np.abs(dZ) * (rho + 3 * ULP)
    E_rm = sc["mom"] * E_mu + ULP * (np.abs(sc["om"] * rm) + np.abs(sc["mom"] * mu) + np.abs(rm2))
    E_rv = sc["mom"] * sc["unb"] * E_v + ULP * (np.abs(sc["om"] * rv) + 2 * np.abs(sc["mom"] * v * sc["unb"]) + np.abs(rv2))
    values = dict(mu=mu, v=v, H=H, g_beta=gb, g_gamma=gg, dZ=dZ, rm=rm2, rv=rv2)
    bounds = dict(mu=E_mu, v=E_v, H=E_H, g_beta=E_gb, g_gamma=E_gg, dZ=E_dZ, rm=E_rm, rv=E_rv)
    return values, bounds


def fold_ref(weights, biases, gamma, beta, rm, rv, eps=1e-5):
    """The float64 fold of fp32 state -> (weights, biases, weight bounds, bias bounds), one entry per layer (the last layer is itself,
    bound 0)."""
    e = float(F32(eps))
    ws, bs, ews, ebs = [], [], [], []
    for l in range(len(weights) - 1):
        W, b = np.asarray(weights[l], np.float64), np.asarray(biases[l], np.float64)
        g, be, mu, v = (np.asarray(a[l], np.float64) for a in (gamma, beta, rm, rv))
        s = g / np.sqrt(v + e)
        ws.append(s[:, None] * W)
        bs.append(be + s * (b - mu))
        ews.append(3.5 * ULP * np.abs(ws[-1]))
        ebs.append(4.5 * ULP * np.abs(s * (b - mu)) + ULP * np.abs(bs[-1]))
    ws.append(np.asarray(weights[-1], np.float64))
    bs.append(np.asarray(biases[-1], np.float64))
    ews.append(np.zeros_like(ws[-1]))
    ebs.append(np.zeros_like(bs[-1]))
    return ws, bs, ews, ebs


def peak(got, want, bound):
    """max over the elements of |got - want| / bound, an element with bound 0 counting 0 when it is exact and inf otherwise."""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(r.max())


# ---- fp32 in the kernels' order -------------------------------------------------------------------------------------------------
def col_sum32(T):
    """The kernels' column sum of the fp32 terms T [M][N]: quarters of ceil(M / 4) rows, four chains each, pairwise combination."""
    M, N = T.shape
    per = (M + 3) // 4
    parts = []
    for q in range(4):
        b = min(q * per, M)
        e = min(b + per, M)
        s = [np.zeros(N, F32) for _ in range(4)]
        m = b
        while m + 3 < e:
            for j in range(4):
                s[j] = s[j] + T[m + j]
            m += 4
        while m < e:
            s[0] = s[0] + T[m]
            m += 1
        parts.append((s[0] + s[1]) + (s[2] + s[3]))
    return (parts[0] + parts[1]) + (parts[2] + parts[3])


def stage_fp32(Z, dA, gamma, beta, rm, rv, eps=1e-5, mom=0.1, wrong=None):
    """``bn_forward_kernel`` and ``bn_backward_kernel`` in numpy fp32, operation for operation.  ``wrong``: None, or one of
    "unbiased_normaliser" (v M / (M - 1) under the square root), "biased_running" (rv moves by the biased v), "dropped_term" (dZ
    without xhat g_gamma), "one_pass" (v = E[z^2] - mu^2)."""
    Z, dA, gamma, beta, rm, rv = (np.asarray(a, F32) for a in (Z, dA, gamma, beta, rm, rv))
    M = Z.shape[0]
    sc = scalars(M, eps, mom)
    mf = F32(M)
    with np.errstate(invalid="ignore"):
        mu = col_sum32(Z) / mf
        if wrong == "one_pass":
            v = col_sum32(Z * Z) / mf - mu * mu
        else:
            d = Z - mu
            v = col_sum32(d * d) / mf
        vn = v * sc["unb"] if wrong == "unbiased_normaliser" else v
        rstd = F32(1.0) / np.sqrt(vn + sc["eps"])
        xh = (Z - mu) * rstd
        H = np.maximum(gamma * xh + beta, F32(0.0))
        gb = col_sum32(dA)
        gg = col_sum32(dA * xh)
        k = (gamma * rstd) / mf
        t = mf * dA - gb
        if wrong != "dropped_term":
            t = t - xh * gg
        dZ = k * t
        rm2 = sc["om"] * rm + sc["mom"] * mu
        rv2 = sc["om"] * rv + sc["mom"] * (v if wrong == "biased_running" else v * sc["unb"])
    out = dict(mu=mu, v=v, H=H, g_beta=gb, g_gamma=gg, dZ=dZ, rm=rm2, rv=rv2)
    assert all(a.dtype == F32 for a in out.values())
    return out


def fold_fp32(weights, biases, gamma, beta, rm, rv, eps=1e-5):
    """``bn_fold_kernel`` in numpy fp32."""
    ws, bs = [], []
    for l in range(len(weights) - 1):
        s = gamma[l] / np.sqrt(rv[l] + F32(eps))
        ws.append(s[:, None] * weights[l])
        bs.append(beta[l] + s * (biases[l] - rm[l]))
    return ws + [weights[-1]], bs + [biases[-1]]


# ---- the training step: Linear -> BatchNorm1d -> ReLU ... -> Linear, weighted CE + L2, Adam ------------------------------------------
class NumpyNet:
    """The definition of the training step in numpy, in ``dtype`` (float64: the reference of the recipe; the sums are numpy's).
    ``batch_norm=False`` is the plain head.  Mean-reduced cross-entropy plus (0.5 alpha / mb) sum W^2, torch.optim.Adam's update."""

    def __init__(self, weights, biases, batch_norm, lr, alpha=1e-4, eps=1e-5, mom=0.1, dtype=np.float64):
        self.W = [np.array(w, dtype) for w in weights]
        self.b = [np.array(b, dtype) for b in biases]
        self.bn, self.lr, self.alpha, self.eps, self.mom = batch_norm, lr, alpha, eps, mom
        hidden = [w.shape[0] for w in weights[:-1]]
        self.gamma = [np.ones(n, dtype) for n in hidden]
        self.beta = [np.zeros(n, dtype) for n in hidden]
        self.rm = [np.zeros(n, dtype) for n in hidden]
        self.rv = [np.ones(n, dtype) for n in hidden]
        self.params = self.W + self.b + (self.gamma + self.beta if batch_norm else [])
        self.m = [np.zeros_like(p) for p in self.params]
        self.v = [np.zeros_like(p) for p in self.params]
        self.t = 0

    def forward_eval(self, X):
        h = np.asarray(X, self.W[0].dtype)
        for l, (W, b) in enumerate(zip(self.W, self.b)):
            h = h @ W.T + b
            if l < len(self.W) - 1:
                if self.bn:
                    h = self.gamma[l] * (h - self.rm[l]) / np.sqrt(self.rv[l] + self.eps) + self.beta[l]
                h = np.maximum(h, 0)
        return h

    def step(self, X, y):
        """One Adam step on the mini-batch -> its loss (before the update)."""
        L, M = len(self.W), len(y)
        hs, cache = [np.asarray(X, self.W[0].dtype)], []
        for l in range(L):
            z = hs[-1] @ self.W[l].T + self.b[l]
            if l < L - 1:
                if self.bn:
                    mu, var = z.mean(axis=0), z.var(axis=0)
                    rstd = 1.0 / np.sqrt(var + self.eps)
                    xh = (z - mu) * rstd
                    cache.append((xh, rstd))
                    self.rm[l] = (1 - self.mom) * self.rm[l] + self.mom * mu
                    self.rv[l] = (1 - self.mom) * self.rv[l] + self.mom * var * M / (M - 1.0)
                    z = self.gamma[l] * xh + self.beta[l]
                z = np.maximum(z, 0)
            hs.append(z)
        logits = hs[-1]
        zs = logits - logits.max(axis=1, keepdims=True)
        logp = zs - np.log(np.exp(zs).sum(axis=1, keepdims=True))
        loss = -logp[np.arange(M), y].mean() + 0.5 * self.alpha / M * sum((W * W).sum() for W in self.W)
        g = np.exp(logp)
        g[np.arange(M), y] -= 1.0
        g /= M
        gW, gb, gga, gbe = [None] * L, [None] * L, [None] * (L - 1), [None] * (L - 1)
        for l in range(L - 1, -1, -1):
            gW[l] = g.T @ hs[l] + self.alpha / M * self.W[l]
            gb[l] = g.sum(axis=0)
            if l > 0:
                g = (g @ self.W[l]) * (hs[l] > 0)
                if self.bn:
                    xh, rstd = cache[l - 1]
                    gbe[l - 1] = g.sum(axis=0)
                    gga[l - 1] = (g * xh).sum(axis=0)
                    g = self.gamma[l - 1] * rstd / M * (M * g - gbe[l - 1] - xh * gga[l - 1])
        if self.bn:                         # the bias of a normalised layer cancels: its exact gradient is zero
            for l in range(L - 1):
                gb[l] = np.zeros_like(gb[l])
        grads = gW + gb + (gga + gbe if self.bn else [])
        self.t += 1
        b1, b2, e = 0.9, 0.999, 1e-8
        for p, gr, m, v in zip(self.params, grads, self.m, self.v):
            m += (1 - b1) * (gr - m)
            v *= b2
            v += (1 - b2) * gr * gr
            p -= self.lr / (1 - b1 ** self.t) * m / (np.sqrt(v) / math.sqrt(1 - b2 ** self.t) + e)
        return float(loss)


# ---- the torch loop of the training comparison ----------------------------------------------------------------------------------------
K7, NF, NROWS, BATCH = 7, 16, 230, 50


def train_data():
    """tests/test_gpu_loss.py's set: 230 rows of 16 features in 7 classes, class weights with a zero."""
    rng = np.random.default_rng(17)
    y = rng.integers(0, K7, size=NROWS)
    centres = rng.normal(0, 1.0, (K7, NF))
    X = (centres[y] + rng.normal(0, 1.0, (NROWS, NF))).astype(F32)
    w = np.array([1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.75], F32)
    return dict(X=X, y=y, w=w, cw={k: float(v) for k, v in enumerate(w)})


def initial_parameters(hidden=(24, 12), seed=0):
    """Glorot weights and zero biases drawn as ``TorchMLPClassifier._initial_parameters`` draws them."""
    import torch
    import torch.nn as nn
    torch.manual_seed(seed)
    sizes = [NF, *hidden, K7]
    layers = [nn.Linear(i, o) for i, o in zip(sizes[:-1], sizes[1:])]
    for m in layers:
        nn.init.xavier_uniform_(m.weight)
        nn.init.zeros_(m.bias)
    return [m.weight.detach().numpy().copy() for m in layers], [m.bias.detach().numpy().copy() for m in layers]


def lr_at(step, lr, schedule, total):
    """The cosine schedule of include/mmc.h without warm-up and with final ratio 0 (``optim.lr_at``), or the constant rate."""
    if schedule != "cosine":
        return lr
    u = min(1.0, max(0.0, step / float(max(1, total))))
    return lr * 0.5 * (1.0 + math.cos(math.pi * u))


def torch_loop(data, dtype, passes=3, lr=1e-3, alpha=1e-3, weighted=False, label_smoothing=0.0, max_norm=None, schedule="constant",
               eps=1e-5, mom=0.1, hidden=(24, 12)):
    """``Linear -> BatchNorm1d -> ReLU -> ... -> Linear`` trained by the reference's mini-batch loop in torch on the CPU in ``dtype``:
    the classifier's initial parameters and visiting order, F.cross_entropy, the L2 term (0.5 alpha / mb) sum W^2, clip_grad_norm_,
    torch.optim.Adam with the scheduled rate.  -> dict(curve, W, b, gamma, beta, rm, rv)."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    w0, b0 = initial_parameters(hidden)
    layers = [nn.Linear(w.shape[1], w.shape[0]) for w in w0]
    norms = [nn.BatchNorm1d(w.shape[0], eps=eps, momentum=mom) for w in w0[:-1]]
    with torch.no_grad():
        for m, w, b in zip(layers, w0, b0):
            m.weight.copy_(torch.from_numpy(w))
            m.bias.copy_(torch.from_numpy(b))
    for m in layers + norms:
        m.to(dtype)
        m.train()
    for m in layers[:-1]:                   # the definition: the bias of a normalised layer cancels and is frozen.  Left trainable,
        m.bias.requires_grad_(False)        # Adam walks it on the rounding noise of a gradient that is exactly zero (|g| ~ 1e-9 ~ eps)
    params = [p for m in layers + norms for p in m.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999), eps=1e-8)
    wt = torch.from_numpy(data["w"]).to(dtype) if weighted else None
    order = np.arange(NROWS)
    np.random.default_rng(0).shuffle(order)                     # the classifier's shuffle: a fresh generator per pass
    Xo, yo = torch.from_numpy(data["X"][order]).to(dtype), torch.from_numpy(data["y"][order].astype(np.int64))
    steps_total = passes * -(-NROWS // BATCH)
    curve, step = [], 0
    for _ in range(passes):
        total = 0.0
        for start in range(0, NROWS, BATCH):
            xb, yb = Xo[start:start + BATCH], yo[start:start + BATCH]
            step += 1
            for grp in opt.param_groups:
                grp["lr"] = lr_at(step, lr, schedule, steps_total)
            opt.zero_grad()
            h = xb
            for i, m in enumerate(layers):
                h = m(h)
                if i < len(layers) - 1:
                    h = torch.relu(norms[i](h))
            loss = F.cross_entropy(h, yb, weight=wt, label_smoothing=label_smoothing) \
                + (0.5 * alpha / len(yb)) * sum((m.weight ** 2).sum() for m in layers)
            loss.backward()
            if max_norm is not None:
                torch.nn.utils.clip_grad_norm_(params, max_norm)
            opt.step()
            total += loss.item() * len(yb)
        curve.append(total / NROWS)
    return dict(curve=curve, W=[m.weight.detach().numpy() for m in layers], b=[m.bias.detach().numpy() for m in layers],
                gamma=[m.weight.detach().numpy() for m in norms], beta=[m.bias.detach().numpy() for m in norms],
                rm=[m.running_mean.numpy() for m in norms], rv=[m.running_var.numpy() for m in norms])


TRAIN_KINDS = {"plain": dict(), "weights_clip_cosine": dict(weighted=True, max_norm=0.5, schedule="cosine"),
               "smoothing": dict(label_smoothing=0.1)}


def train_gap(a, b):
    """-> (largest difference over the weights, biases, gamma, beta and running statistics; largest difference of the loss curves)."""
    pairs = [(u, v) for key in ("W", "b", "gamma", "beta", "rm", "rv") for u, v in zip(a[key], b[key])]
    dw = max(float(np.abs(np.asarray(u, np.float64) - np.asarray(v, np.float64)).max()) for u, v in pairs)
    return dw, float(np.abs(np.asarray(a["curve"]) - np.asarray(b["curve"])).max())
