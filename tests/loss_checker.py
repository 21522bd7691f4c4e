"""What tests/test_loss_host.py and tests/test_gpu_loss.py share: the fp64 checker of the trainer's loss formulations (label
smoothing, focal modulation, logit prior: include/mmc.h, ``mmc_trainer_set_loss``), the per-element bounds, a numpy fp32 emulation
of the kernel's arithmetic, and the logit rows both are run on.  Not a test module.

The checker is the definition, evaluated by torch autograd in fp64::

    u      = z + o                                  (fp32 add, per element)
    logp_c = log_softmax(u)_c,  p_t = exp(logp_t),  nll = -logp_t,  q = 1 - p_t,  m = q^gamma   (gamma = 0: m = 1)
    l_i    = (1 - eps) w_t m nll + (eps / K) sum_c w_c (-logp_c)
    L      = sum_i l_i / sum_i w[y_i]

Bounds, per element, in units of 2^-24 (the fp32 rounding unit): 128 units of ``g w_max`` on ``dlogits`` and 96 units of
``|l_i g| + g w_max`` on ``row_loss``, with ``g = 1 / sum_i w[y_i]`` and ``w_max`` the largest class weight.  An fp32 evaluation in
the kernel's order peaks at roughly a fifth of them on the grid of test_loss_host.py; the rest is room for a device ``expf`` /
``logf`` / ``powf`` that differs from numpy's by a few ulp."""

import numpy as np

DLOGITS_UNITS, ROW_LOSS_UNITS = 128.0, 96.0
ULP = 2.0 ** -24


def special_rows(K, t=0):
    """Four rows: the true logit (class ``t``) at +60, -60 and +17 over zeros, and an all-zero row; their labels."""
    z = np.zeros((4, K), np.float32)
    z[0, t], z[1, t], z[2, t] = 60.0, -60.0, 17.0
    return z, np.full(4, t, np.int64)


def logit_rows(rng, n, K, scale):
    """``n`` rows: Gaussian logits times ``scale`` with uniform labels, the last four replaced by ``special_rows``."""
    z = (rng.standard_normal((n, K)) * scale).astype(np.float32)
    y = rng.integers(0, K, size=n)
    if n >= 5:
        t = int(rng.integers(0, K))
        z[-4:], y[-4:] = special_rows(K, t)
    return z, y.astype(np.int64)


def class_weights(rng, K):
    """Weights in [0.5, 2), one class at zero."""
    w = rng.uniform(0.5, 2.0, K).astype(np.float32)
    w[int(rng.integers(0, K))] = 0.0
    return w


def dirichlet_prior(rng, K):
    """0.7 log of a Dirichlet draw: the offsets ``logit_adjustment`` would give for class frequencies drawn at random."""
    return (0.7 * np.log(np.maximum(rng.dirichlet(np.ones(K)), 1e-30))).astype(np.float32)


def weight_sum(y, w):
    """sum_i w[y_i] as the library forms it: a double sum over the rows in order."""
    if w is None:
        return float(len(y))
    s = 0.0
    for v in w[y].tolist():
        s += v
    return s


def checker(z, y, w=None, prior=None, eps=0.0, gamma=0.0):
    """-> (dlogits [n][K] fp64, row_loss [n] fp64 = l_i g, L fp64, the torch tensors u / weights for further comparison)."""
    import torch
    n, K = z.shape
    u32 = z if prior is None else (z + prior[None, :]).astype(np.float32)     # the fp32 add of the definition
    u = torch.tensor(u32.astype(np.float64), requires_grad=True)
    yt = torch.tensor(np.asarray(y, np.int64))
    wt = torch.ones(K, dtype=torch.float64) if w is None else torch.tensor(w.astype(np.float64))
    logp = torch.log_softmax(u, dim=1)
    logpt = logp.gather(1, yt[:, None])[:, 0]
    nll = -logpt
    q = -torch.expm1(logpt)                                                    # 1 - p_t without cancellation
    m = q ** gamma if gamma != 0.0 else torch.ones_like(q)
    l = (1.0 - eps) * wt[yt] * m * nll + (eps / K) * -(logp * wt[None, :]).sum(dim=1)
    g = 1.0 / wt[yt].sum()
    L = l.sum() * g
    L.backward()
    return u.grad.numpy().copy(), (l * g).detach().numpy().copy(), float(L.detach()), (u.detach(), yt, wt)


def bounds(y, w, row_loss_ref):
    """-> (bound on every dlogits element, bound per row_loss element) for these rows."""
    wmax = 1.0 if w is None else float(w.max())
    g = 1.0 / weight_sum(np.asarray(y), w)
    return DLOGITS_UNITS * ULP * g * wmax, ROW_LOSS_UNITS * ULP * (np.abs(row_loss_ref) + g * wmax)


def _lane_sum(v):
    """Row sums as the kernel forms them: lane c % 64 adds its elements in order, then the xor butterfly 32, 16, ..., 1."""
    n, K = v.shape
    pad = (-K) % 64
    v = np.concatenate([v, np.zeros((n, pad), np.float32)], axis=1).reshape(n, -1, 64)
    lanes = np.zeros((n, 64), np.float32)
    for j in range(v.shape[1]):
        lanes = lanes + v[:, j, :]
    o = 32
    while o >= 1:
        lanes = lanes[:, :o] + lanes[:, o:2 * o]
        o >>= 1
    return lanes[:, 0]


def emulate(z, y, w=None, prior=None, eps=0.0, gamma=0.0, drop_focal=False, drop_smoothing=False, drop_prior=False):
    """The general kernel's arithmetic in numpy fp32, operation for operation -> (dlogits, row_loss) fp32.  The ``drop_*`` flags
    make the three wrong kernels the bounds have to catch."""
    f32 = np.float32
    n, K = z.shape
    y = np.asarray(y)
    rows = np.arange(n)
    om_eps, eps_k, gam = f32(1.0 - eps), f32(eps / K), f32(gamma)
    w_total = f32(K) if w is None else f32(sum(float(v) for v in w))
    inv_wsum = f32(1.0 / weight_sum(y, w))
    if drop_focal:
        gam = f32(0.0)
    if drop_smoothing:
        eps_k = f32(0.0)
    u = z if (prior is None or drop_prior) else (z + prior[None, :]).astype(f32)
    mx = u.max(axis=1, keepdims=True)
    e = np.exp(u - mx)
    s = _lane_sum(e)
    eo = e.copy()
    eo[rows, y] = 0.0
    so = _lane_sum(eo)
    lse = np.log(s)
    wy = np.ones(n, f32) if w is None else w[y]
    lp = (u - mx) - lse[:, None]
    sw = _lane_sum(lp if w is None else w[None, :] * lp)
    ut = u[rows, y]
    nll = lse - (ut - mx[:, 0])
    if gam != 0:
        q = so / s
        pt = np.exp((ut - mx[:, 0]) - lse)
        pw = np.power(q, f32(gam - f32(1.0)))
        m = pw * q
        f = m + gam * pt * pw * nll
    else:
        m = np.ones(n, f32)
        f = np.ones(n, f32)
    a = om_eps * wy
    af = a * f
    p = np.exp(lp)
    onehot = np.zeros((n, K), f32)
    onehot[rows, y] = 1.0
    d = af[:, None] * (p - onehot)
    l = a * m * nll
    if eps_k != 0:
        wc = np.ones(K, f32) if w is None else w
        d = d + eps_k * (p * w_total - wc[None, :])
        l = l - eps_k * sw
    d = inv_wsum * d
    l = l * inv_wsum
    assert d.dtype == np.float32 and l.dtype == np.float32
    return d, l
