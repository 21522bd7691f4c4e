"""Float64 numpy restatement of include/mmc.h, section "logit calibration": the sums of one pass, a bound for every element of
them, and a reference fit.  tests/test_logit_scaling_host.py holds this file to torch autograd; tests/test_gpu_logit_scaling.py
holds the device to this file.

Definition (all float64 on the fp32 logits)::

    u_nk = a_k z_nk + c_k     m_n = max_k u_nk     e_nk = exp(u_nk - m_n)     s_n = sum_k e_nk     p_nk = e_nk / s_n
    lse_n = m_n + log s_n     F = sum_n (lse_n - u_n,y_n)     r = p - onehot(y)
    g_a = sum_n z r   g_c = sum_n r   D_aa = sum z^2 p   D_ac = sum z p   D_cc = sum p   H = D - sum_n v v^T, v = [z p ; p]

Bounds.  Every output element is a sum of terms; its bound is ``gamma * 2**-53 * A`` with A the sum of the absolute values of the
element's terms (computed here) and gamma an operation count in units of 2**-53 (one unit = the relative error of one correctly
rounded operation; 1 ulp = 2 units).  The counts, for ONE implementation:

``gamma_acc(N)``  additions along the fixed order.  The device adds a block's B = BLOCK_ROWS rows in one chain per element (one fma or
    add per row; a 16x16x4 f64 MFMA is taken as four chained fused multiply-adds per element: one rounding per row), then the blocks'
    partials in block order; the loss additionally folds 32 row slots and 4 butterfly levels, fewer than the B - B/32 rows a lane
    does not see.  ``gamma_acc = min(N, B) + ceil(N / B)``.
``gamma_p``       relative error of p_nk.  With U = max |u_nk|: u is one fma (1 unit of |u| <= U), m is one of the u (U), their
    difference rounds once (<= 2 U): the argument of exp is off by <= 4 U units ABSOLUTE, which exp turns into a relative error;
    exp itself adds ULP_EXP ulp.  s adds K - 1 additions to that; the division is correctly rounded (ULP_DIV ulp = 0.5).
    ``gamma_p = (4 U + 2 ULP_EXP) + (4 U + 2 ULP_EXP + K) + 2 ULP_DIV = 8 U + 4 ULP_EXP + K + 1``.
``ULP_EXP = ULP_LOG = 1``  ASSUMED.  The ROCm device-library documentation is not shipped with the toolchain this was written against;
    1 ulp is what the HIP math tables state for double-precision exp and log, and what numpy's libm delivers.

    element    terms (A sums their absolute values)                       gamma (one implementation)
    g_c[k]     p_nk and -[y_n = k]                                        gamma_acc + gamma_p + 1         (the subtraction)
    g_a[k]     z_nk p_nk and -z_nk [y_n = k]                              gamma_acc + gamma_p + 2         (+ the product)
    D_cc[k]    p_nk                                                       gamma_acc + gamma_p
    D_ac[k]    z_nk p_nk                                                  gamma_acc + gamma_p + 1
    D_aa[k]    z_nk^2 p_nk                                                gamma_acc + gamma_p + 2
    H[i,j]     v_ni v_nj, and the D entry's terms where there is one      gamma_acc + 2 gamma_p + 4       (two v, product, D - .)
    F          m_n, 1 + log s_n, u_n,y_n                                  gamma_acc + 4 U + 2 ULP_EXP + 2 ULP_LOG + K + 2

    F: log s_n has the ABSOLUTE error of s_n's relative one (s_n >= 1), 4 U + 2 ULP_EXP + K units whatever log s_n is -- the "1" among
    the terms carries it; log adds 2 ULP_LOG units of log s_n; m_n, u_n,y_n one unit each, the two additions one each.

The device is compared with THIS file, which makes the same roundings (numpy sums pairwise: shorter chains), so a gate is
``|device - checker| <= bound`` with ``bound = 2 * gamma * 2**-53 * A``: the factor 2 is the two implementations.  All gates are 1x.

Folded head (``LogitScaling.fold``), fp32: logit k of the folded classifier against a_k z_k + c_k of the unfolded one, both from the
same fp32 hidden activations h (d of them).  Folded: W' = fl32(a W) (1 unit of 2**-24 per weight), d products and d additions in an
order the GEMM chooses (<= d + 1 units), b' = fl32(a b + c) (1): d + 3.  Unfolded: z has d + 2 units of sum |W h| + |b|, scaled by
|a|.  ``FOLD_GAMMA(d) = 2 d + 5``; bound = FOLD_GAMMA(d) * 2**-24 * (sum_j |a_k W_kj h_j| + |a_k b_k| + |c_k|).
"""

import numpy as np

BLOCK_ROWS = 1024          # include/mmc.h MMC_LOGITCAL_BLOCK_ROWS: rows per block of the fixed partition
MAX_CLASSES = 128
ULP_EXP = ULP_LOG = 1.0    # assumed, see the header
ULP_DIV = 0.5
EPS = 2.0 ** -53
KINDS = ("temperature", "bias", "vector")


def FOLD_GAMMA(d: int) -> int:
    return 2 * int(d) + 5


def gamma_acc(N: int) -> int:
    return min(int(N), BLOCK_ROWS) + -(-int(N) // BLOCK_ROWS)


def _forward(z, a, c):
    z = np.asarray(z, np.float32).astype(np.float64)
    u = np.asarray(a, np.float64)[None, :] * z + np.asarray(c, np.float64)[None, :]
    m = u.max(axis=1)
    e = np.exp(u - m[:, None])
    s = e.sum(axis=1)
    return z, u, m, s, e / s[:, None]


def stats(z, y, a, c, hess=True):
    """-> dict: ``nll`` (sum), ``grad`` (2K: a then c), ``hess`` (2K x 2K or None), ``counts`` (K,), ``p`` (N x K) and, under
    ``A_nll`` / ``A_grad`` / ``A_hess``, the sums of absolute terms, ``U`` = max |u|."""
    y = np.asarray(y, np.int64)
    z, u, m, s, p = _forward(z, a, c)
    N, K = z.shape
    rows = np.arange(N)
    uy = u[rows, y]
    onehot = np.zeros((N, K))
    onehot[rows, y] = 1.0
    r = p - onehot
    out = {"p": p, "U": float(np.abs(u).max()), "counts": np.bincount(y, minlength=K).astype(np.int64)}
    out["nll"] = float(((m + np.log(s)) - uy).sum())
    out["A_nll"] = float((np.abs(m) + 1.0 + np.log(s) + np.abs(uy)).sum())
    out["grad"] = np.concatenate([(z * r).sum(axis=0), r.sum(axis=0)])
    out["A_grad"] = np.concatenate([(np.abs(z) * (p + onehot)).sum(axis=0), (p + onehot).sum(axis=0)])
    out["hess"] = out["A_hess"] = None
    if hess:
        v = np.concatenate([z * p, p], axis=1)
        av = np.abs(v)
        H = -(v.T @ v)
        A = av.T @ av
        daa, dac, dcc = (z * z * p).sum(axis=0), (z * p).sum(axis=0), p.sum(axis=0)
        k = np.arange(K)
        H[k, k] += daa
        H[K + k, K + k] += dcc
        H[k, K + k] += dac
        H[K + k, k] += dac
        A[k, k] += daa
        A[K + k, K + k] += dcc
        A[k, K + k] += (np.abs(z) * p).sum(axis=0)
        A[K + k, k] += (np.abs(z) * p).sum(axis=0)
        out["hess"], out["A_hess"] = H, A
    return out


def bounds(st, N: int, K: int):
    """``stats``' result -> (bound on nll, bound on grad (2K), bound on hess (2K x 2K) or None): the 1x gates of the header, two
    implementations included."""
    U, ga = st["U"], gamma_acc(N)
    gp = 8.0 * U + 4.0 * ULP_EXP + K + 2.0 * ULP_DIV
    b_nll = 2.0 * (ga + 4.0 * U + 2.0 * ULP_EXP + 2.0 * ULP_LOG + K + 2.0) * EPS * st["A_nll"]
    g_gamma = np.concatenate([np.full(K, ga + gp + 2.0), np.full(K, ga + gp + 1.0)])
    b_grad = 2.0 * g_gamma * EPS * st["A_grad"]
    b_hess = None if st["A_hess"] is None else 2.0 * (ga + 2.0 * gp + 4.0) * EPS * st["A_hess"]
    return b_nll, b_grad, b_hess


def objective(z, y, a, c, l2=0.0):
    """F(a, c), ridge included."""
    st = stats(z, y, a, c, hess=False)
    N = len(np.asarray(y))
    a, c = np.asarray(a, np.float64), np.asarray(c, np.float64)
    return st["nll"] + 0.5 * l2 * N * (((a - 1.0) ** 2).sum() + (c ** 2).sum())


def frozen_mask(counts, kind):
    counts = np.asarray(counts)
    return np.zeros(len(counts), bool) if kind == "temperature" else counts == 0


def active_index(K, kind, frozen):
    """Indices into theta = (a, c) of the active parameters of ``bias`` / ``vector``, in the order of csrc/logit_newton.h."""
    live = np.flatnonzero(~np.asarray(frozen, bool))
    if kind == "bias":
        return K + live
    if kind == "vector":
        return np.concatenate([live, K + live])
    raise ValueError(kind)


def active_gradient(z, y, a, c, kind, l2=0.0, frozen=None):
    """The gradient of F over the active parameters at (a, c), ridge included, and the bound on it (same shape)."""
    y = np.asarray(y)
    N, K = len(y), np.asarray(z).shape[1]
    st = stats(z, y, a, c, hess=False)
    _, b_grad, _ = bounds(st, N, K)
    a, c = np.asarray(a, np.float64), np.asarray(c, np.float64)
    full = st["grad"] + l2 * N * np.concatenate([a - 1.0, c])
    if kind == "temperature":
        return np.array([full[:K].sum()]), np.array([b_grad[:K].sum()])
    idx = active_index(K, kind, frozen_mask(st["counts"], kind) if frozen is None else frozen)
    return full[idx], b_grad[idx]


def fit(z, y, kind, l2=0.0, tol=1e-9, max_trials=100):
    """The rule of csrc/logit_newton.h in numpy (numpy's solver in place of the in-tree Cholesky).  -> dict(a, c, frozen, trials,
    converged, nll_before, nll_after (means))."""
    y = np.asarray(y, np.int64)
    N, K = len(y), np.asarray(z).shape[1]
    counts = np.bincount(y, minlength=K)
    frozen = frozen_mask(counts, kind)
    idx = None if kind == "temperature" else active_index(K, kind, frozen)
    l2N = l2 * N

    def reduced(a, c, st):
        g = st["grad"] + l2N * np.concatenate([a - 1.0, c])
        H = None if st["hess"] is None else st["hess"] + l2N * np.eye(2 * K)
        if kind == "temperature":
            return np.array([g[:K].sum()]), (None if H is None else np.array([[H[:K, :K].sum()]]))
        return g[idx], (None if H is None else H[np.ix_(idx, idx)])

    def step(a, c, d):
        a2, c2 = a.copy(), c.copy()
        if kind == "temperature":
            a2[:] = a[0] + d[0]
        else:
            theta = np.concatenate([a, c])
            theta[idx] += d
            a2, c2 = theta[:K].copy(), theta[K:].copy()
        return a2, c2

    a, c = np.ones(K), np.zeros(K)
    st = stats(z, y, a, c)
    before = after = st["nll"]
    F = st["nll"]
    g, H = reduced(a, c, st)
    lam, trials, converged = 1e-3, 0, False
    n = len(g)
    if n == 0:
        converged = True
    while n:
        if np.abs(g).max() / N <= tol:
            converged = True
            break
        if trials >= max_trials:
            break
        tau = np.trace(H) / n
        tau = tau if tau > 0 and np.isfinite(tau) else 1.0
        d = None
        for _ in range(60):
            try:
                np.linalg.cholesky(H + lam * tau * np.eye(n))
                d = -np.linalg.solve(H + lam * tau * np.eye(n), g)
                if np.isfinite(d).all():
                    break
            except np.linalg.LinAlgError:
                pass
            d = None
            lam *= 8.0
        if d is None:
            break
        a2, c2 = step(a, c, d)
        with np.errstate(all="ignore"):
            st2 = stats(z, y, a2, c2)
        trials += 1
        F2 = st2["nll"] + 0.5 * l2N * (((a2 - 1.0) ** 2).sum() + (c2 ** 2).sum())
        if np.isfinite(F2) and F2 <= F:
            a, c, F, after = a2, c2, F2, st2["nll"]
            lam = max(lam / 8.0, 1e-12)
            g, H = reduced(a, c, st2)
        else:
            lam *= 8.0
    return {"a": a, "c": c, "frozen": frozen, "trials": trials, "converged": converged, "nll_before": before / N, "nll_after": after / N}


def fixture(N: int, K: int, seed: int = 0, dim: int = 16):
    """The fit fixture: logits = 2.5 x (a ``dim``-feature linear score with per-class gains in [0.6, 1.4] and a per-class offset), fp32;
    labels = argmax of the clean score + 1.5 x Gumbel noise.  An over-confident, per-class miscalibrated head."""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((K, dim)) / np.sqrt(dim) * 2.0
    x = rng.standard_normal((N, dim))
    clean = x @ W.T
    gains = rng.uniform(0.6, 1.4, K)
    offsets = rng.standard_normal(K) * 0.5
    z = (2.5 * (gains[None, :] * clean + offsets[None, :])).astype(np.float32)
    y = np.argmax(clean + 1.5 * rng.gumbel(size=(N, K)), axis=1).astype(np.int32)
    return z, y


def separable(n_per=20, K=3):
    """60 x 3: logits 4 * onehot(y) -- every row on the right side, no finite minimiser at l2 = 0."""
    y = np.repeat(np.arange(K), n_per).astype(np.int32)
    z = np.zeros((len(y), K), np.float32)
    z[np.arange(len(y)), y] = 4.0
    return z, y
