"""What tests/test_distill_host.py and tests/test_gpu_distill.py share: the fp64 checker of the distillation loss (per-row soft
targets: include/mmc.h, "distillation"), the per-element bounds, a numpy fp32 emulation of ``ce_grad_rows_distill``'s arithmetic, the
bank of teacher rows, and a float64 student loop for the evidence test.  Not a test module.

The checker is the definition, evaluated by torch autograd in fp64 on the fp32-rounded u and the stored fp32 q::

    u      = z + o                                  (fp32 add, per element)
    b_i    = the general form of tests/loss_checker.py (the plain weighted CE at its defaults)
    tau = 1:   qt = q,  logpt = log_softmax(u)
    tau != 1:  qt_c = q_c^(1/tau) / sum_c' q_c'^(1/tau) (0 stays 0),  logpt = log_softmax(u / tau), with the exact 1 / tau
    k_i    = -sum_c qt_c logpt_c                    (a class with qt_c == 0 adds 0)
    l_i    = s_i [(1 - alpha) b_i + alpha tau^2 w_t k_i],   s_i as tests/hier_loss_checker.py's ``normaliser``

Bounds, per element, in units of ULP = 2^-24, counted from the kernel's operations exactly as tests/hier_loss_checker.py counts its
own: a correctly rounded fp32 operation errs by one unit of its result, a device ``expf`` / ``logf`` by TRANS = 4 units,
S(K) = ceil(K / 64) - 1 + 6 roundings in a lane-strided sum, ``E_lse(K) = S + TRANS + 1 + TRANS ln K`` units absolute on a log-sum-exp
whose sum is >= 1, ``E_p(K) = E_lse + TRANS + 1`` units relative on a softmax entry.  QS = 1 + 1e-3 is the largest sum of a valid row.
Per row let umax = max|u|, vmax = umax / tau, Lmax = 2 vmax + ln K (the largest |logpt_c|), and over the classes with q_c > 0
A = sum_c qt_c |log q_c| / tau, M = max_c qt_c |log q_c| / tau (float64, from the definition).

* ``pt``.  tau = 1: the hard term's p, ``E_pt = E_p``.  tau != 1: v_c = u_c it with it = (float)(1 / tau) carries the cast and the
  product, 2 |v_c| units absolute; moving every argument of a softmax by at most delta moves an entry by at most 2 delta relative, so
  ``E_pt = E_p + 4 vmax``.
* ``qt``.  tau = 1: the stored value, exact; its lane sum sq is off by ``E_sq = S QS``.  tau != 1: g_c = logf(q_c) it is off by
  (TRANS + 2) |log q_c| / tau units absolute (logf, the cast, the product).  The softmax of g moves by
  |d qt_c| <= qt_c (|d g_c| + sum_c' qt_c' |d g_c'|) <= (TRANS + 2) (M + A) units, plus its own E_p relative:
  ``E_qt = E_p + (TRANS + 2) (M + A)``; summed over the classes, ``E_sumq = E_p + 2 (TRANS + 2) A`` and ``E_sq = S + E_sumq``.  An entry
  that underflows in fp32 is off by less than 2^-126, which no unit sees.
* ``dlogits``.  G_c = pt_c sq - qt_c: ``E_soft = E_pt + E_sq + E_qt + 2`` (the product, the subtraction), at magnitude <= QS.  Then
  (a_grad w) G: the cast of a_grad and two products, 3 roundings; om_alpha d_hard: a cast and a product; the sum, s_i d, s_i's own
  product and cast: 6 roundings at magnitude ((1 - alpha) + alpha tau) QS w_max.  The hard term keeps the DLOGITS_UNITS of
  tests/loss_checker.py, scaled by (1 - alpha).  In all
  ``((1 - alpha) DLOGITS_UNITS + alpha tau QS (E_soft + 3) + 6 ((1 - alpha) + alpha tau) QS)  ULP  s_i w_max``.
* ``row_loss``.  logpt_c is two subtractions at magnitude <= Lmax and a log-sum-exp, and for tau != 1 the shift of its arguments:
  ``E_lp = E_lse + 2 Lmax + [tau != 1] 4 vmax`` units absolute.  k = -sum qt_c logpt_c: qt's weight on E_lp is at most QS, qt's own
  error weighs Lmax E_sumq, and the products and the lane sum are S + 1 roundings relative to |k| (every term has one sign):
  ``E_k = QS E_lp + Lmax E_sumq + (S + 1) |k|``.  The operations on the result -- a_loss's cast, its two products, om_alpha's cast and
  product, the sum, times s_i, s_i's product and cast -- are at most 9 roundings relative to l_i (both terms are >= 0).  The hard term
  keeps ROW_LOSS_UNITS of |l_i| + (1 - alpha) s_i w_max.  In all
  ``(ROW_LOSS_UNITS + 9) ULP |l_i|  +  ((1 - alpha) ROW_LOSS_UNITS + alpha tau^2 E_k)  ULP  s_i w_max``.

The terms in vmax and in |log q| / tau are where the tau != 1 route pays for the rounded 1 / tau and for logf(q): they are conditions
of the arithmetic, read off the inputs, not off any device output."""

import math

import numpy as np

import hier_loss_checker as hc
import loss_checker as lc

ULP = lc.ULP
TRANS = hc.TRANS
QS = 1.0 + 1e-3
normaliser = hc.normaliser
with_groups = hc.with_groups      # group DRO on top of the stage: the composition of tests/group_dro_checker.py, unchanged


# ---- the kinds both test files run, and how they read a result --------------------------------------------------------------------
KINDS = [("a=1 t=1", dict(alpha=1.0, tau=1.0)), ("a=0.3 t=1", dict(alpha=0.3, tau=1.0)), ("a=0.3 t=2", dict(alpha=0.3, tau=2.0)),
         ("a=1 t=0.5", dict(alpha=1.0, tau=0.5)), ("a=0.5 t=4 prior", dict(alpha=0.5, tau=4.0, prior=True)),
         ("a=0.5 t=1 smoothing+focal", dict(alpha=0.5, tau=1.0, eps=0.1, gamma=2.0))]


def kind_options(kind, prior):
    """One entry of ``KINDS`` -> (alpha, tau, the keyword arguments ``checker`` / ``emulate`` take beside them)."""
    o = dict(kind)
    tau, alpha = o.pop("tau"), o.pop("alpha")
    if o.pop("prior", False):
        o["prior"] = prior
    return alpha, tau, o


def peak(err, bound):
    """Peak error over bound; where the bound is 0 (a row of weight zero) the error has to be 0 too."""
    err, bound = np.abs(np.asarray(err, np.float64)), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())


# ---- teacher rows ---------------------------------------------------------------------------------------------------------------
def teacher_rows(rng, y, K):
    """One valid fp32 target row per label of ``y`` (n >= 8).  Rows 0..6: one-hot on the true class; one-hot on another class; the
    uniform row; masses of 1e-30 beside one near 1; a row summing to 1 + 9e-4; one to 1 - 9e-4; a one-hot row beside exact zeros and
    two small masses.  The rest are Dirichlet draws, half of them sparse (concentration 0.1)."""
    y = np.asarray(y)
    n = len(y)
    assert n >= 8
    q = np.zeros((n, K), np.float64)
    q[0, y[0]] = 1.0
    q[1, (y[1] + 1) % K] = 1.0
    q[2] = 1.0 / K
    q[3] = 1e-30
    q[3, y[3]] = 1.0 - (K - 1) * 1e-30
    q[4] = rng.dirichlet(np.ones(K)) * (1.0 + 9e-4)
    q[5] = rng.dirichlet(np.ones(K)) * (1.0 - 9e-4)
    q[6, y[6]] = 0.75
    q[6, (y[6] + 1) % K] = 0.25 - 1e-7
    q[6, (y[6] + 2) % K] += 1e-7
    for i in range(7, n):
        q[i] = rng.dirichlet(np.full(K, 0.1 if i % 2 else 1.0))
    q = q.astype(np.float32)
    assert valid_rows(q).all()
    return q


def valid_rows(q):
    """The target set's rule per row: every entry finite and >= 0, the double sum in class order within 1e-3 of 1."""
    q = np.asarray(q, np.float32)
    ok = (np.isfinite(q) & (q >= 0)).all(axis=1)
    sums = np.array([math.fsum(row.tolist()) if np.isfinite(row).all() else np.nan for row in q])
    return ok & (np.abs(sums - 1.0) <= 1e-3)


def soften(q, tau):
    """qt in float64 from the stored fp32 q: q itself at tau = 1, else q^(1/tau) renormalised, zeros kept."""
    q = np.asarray(q, np.float32).astype(np.float64)
    if tau == 1.0:
        return q
    with np.errstate(divide="ignore"):
        g = np.where(q > 0, np.log(q) / tau, -np.inf)
    e = np.exp(g - g.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def entropy(qt):
    qt = np.asarray(qt, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.where(qt > 0, qt * np.log(qt), 0.0).sum(axis=1)


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def checker(z, y, q, alpha, tau, w=None, prior=None, eps=0.0, gamma=0.0, norm=None):
    """-> (dlogits [n][K] fp64, row_loss [n] fp64 = l_i, k [n] fp64).  ``norm``: the rows' normalisers s_i in float64."""
    import torch
    n, K = z.shape
    u32 = z if prior is None else (z + prior[None, :]).astype(np.float32)
    u = torch.tensor(u32.astype(np.float64), requires_grad=True)
    yt = torch.tensor(np.asarray(y, np.int64))
    wt = torch.ones(K, dtype=torch.float64) if w is None else torch.tensor(w.astype(np.float64))
    logp = torch.log_softmax(u, dim=1)
    logpt_true = logp.gather(1, yt[:, None])[:, 0]
    qq = -torch.expm1(logpt_true)
    m = qq ** gamma if gamma != 0.0 else torch.ones_like(qq)
    base = (1.0 - eps) * wt[yt] * m * -logpt_true + (eps / K) * -(logp * wt[None, :]).sum(dim=1)
    qt = torch.tensor(soften(q, tau))
    logpt = logp if tau == 1.0 else torch.log_softmax(u / tau, dim=1)
    k = -torch.where(qt > 0, qt * logpt, torch.zeros_like(logpt)).sum(dim=1)
    s = torch.tensor(normaliser(y, w, exact=True) if norm is None else np.asarray(norm, np.float64))
    l = s * ((1.0 - alpha) * base + alpha * tau * tau * wt[yt] * k)
    l.sum().backward()
    return u.grad.numpy().copy(), l.detach().numpy().copy(), k.detach().numpy().copy()


def bounds(z, y, q, alpha, tau, w, row_loss_ref, k_ref, prior=None, norm=None):
    """-> (bound on the dlogits elements of every row [n][1], bound per row_loss element [n]); see the module docstring."""
    n, K = z.shape
    wmax = 1.0 if w is None else float(w.max())
    s = normaliser(y, w, exact=True) if norm is None else np.asarray(norm, np.float64)
    u = z if prior is None else (z + prior[None, :]).astype(np.float32)
    umax = np.abs(u.astype(np.float64)).max(axis=1)
    S, e_lse, e_p = hc.sum_units(K), hc.e_lse(K), hc.e_p(K)
    vmax = umax / tau
    lmax = 2 * vmax + math.log(K)
    if tau == 1.0:
        e_pt, e_sumq, e_sq, e_qt, shift = e_p, 0.0, S * QS, 0.0, 0.0
    else:
        q64 = np.asarray(q, np.float32).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(q64 > 0, soften(q, tau) * np.abs(np.log(q64)) / tau, 0.0)
        A, M = t.sum(axis=1), t.max(axis=1)
        e_pt = e_p + 4 * vmax
        e_qt = e_p + (TRANS + 2) * (M + A)
        e_sumq = e_p + 2 * (TRANS + 2) * A
        e_sq = S + e_sumq
        shift = 4 * vmax
    e_soft = e_pt + e_sq + e_qt + 2
    mag = (1.0 - alpha) + alpha * tau
    bd = ULP * s * wmax * ((1.0 - alpha) * lc.DLOGITS_UNITS + alpha * tau * QS * (e_soft + 3) + 6 * mag * QS)
    e_lp = e_lse + 2 * lmax + shift
    e_k = QS * e_lp + lmax * e_sumq + (S + 1) * np.abs(k_ref)
    bl = ULP * ((lc.ROW_LOSS_UNITS + 9) * np.abs(row_loss_ref) + s * wmax * ((1.0 - alpha) * lc.ROW_LOSS_UNITS + alpha * tau * tau * e_k))
    return np.broadcast_to(bd, (n,))[:, None], bl


# ---- the kernel's arithmetic in numpy fp32 ------------------------------------------------------------------------------------------
WRONG = ("tau_for_tau2", "no_tau_in_gradient", "raw_q", "drop_class_weight", "soft_by_one_minus_alpha")


def emulate(z, y, q, alpha, tau, w=None, prior=None, eps=0.0, gamma=0.0, norm=None, wrong=None):
    """``ce_grad_rows_distill`` in numpy fp32, operation for operation -> (dlogits, row_loss) fp32.  ``wrong`` (one of ``WRONG``) builds
    the wrong kernels the bounds have to catch: tau in place of tau^2 in the loss, the factor tau missing in the gradient, q in place
    of qt, w_t dropped from the soft term, the soft term scaled by (1 - alpha)."""
    assert wrong is None or wrong in WRONG
    f32 = np.float32
    n, K = z.shape
    y = np.asarray(y)
    rows = np.arange(n)
    q = np.asarray(q, f32)
    s_i = normaliser(y, w) if norm is None else np.asarray(norm, f32)
    u = z if prior is None else (z + prior[None, :]).astype(f32)
    mx = u.max(axis=1)
    e = np.exp(u - mx[:, None])
    s = lc._lane_sum(e)
    eo = e.copy()
    eo[rows, y] = 0.0
    so = lc._lane_sum(eo)
    lse = np.log(s)
    wy = np.ones(n, f32) if w is None else w[y]
    lp = (u - mx[:, None]) - lse[:, None]
    p = np.exp(lp)
    onehot = np.zeros((n, K), f32)
    onehot[rows, y] = 1.0
    om_eps, eps_k, gam = f32(1.0 - eps), f32(eps / K), f32(gamma)
    w_total = f32(K) if w is None else f32(sum(float(v) for v in w))
    ut = u[rows, y]
    nll = lse - (ut - mx)
    if gam != 0:
        qf = so / s
        ptrue = np.exp((ut - mx) - lse)
        pw = np.power(qf, f32(gam - f32(1.0)))
        m = pw * qf
        f = m + gam * ptrue * pw * nll
    else:
        m = np.ones(n, f32)
        f = np.ones(n, f32)
    a = om_eps * wy
    af = a * f
    lb = a * m * nll
    d = af[:, None] * (p - onehot)
    if eps_k != 0:
        sw = lc._lane_sum(lp if w is None else w[None, :] * lp)
        wc = np.ones(K, f32) if w is None else w
        lb = lb - eps_k * sw
        d = d + eps_k * (p * w_total - wc[None, :])
    # the soft term
    om_alpha = f32(1.0 - alpha)
    a_grad = f32(alpha if wrong == "no_tau_in_gradient" else alpha * tau)
    a_loss = f32(alpha * tau if wrong == "tau_for_tau2" else alpha * tau * tau)
    if wrong == "soft_by_one_minus_alpha":
        a_grad, a_loss = f32((1.0 - alpha) * tau), f32((1.0 - alpha) * tau * tau)
    if tau != 1.0:
        it = f32(1.0 / tau)
        v = u * it
        mv = v.max(axis=1)
        lv = np.log(lc._lane_sum(np.exp(v - mv[:, None])))
        lpt = (v - mv[:, None]) - lv[:, None]
        pt = np.exp(lpt)
        pos = q > 0
        with np.errstate(divide="ignore"):
            g = np.where(pos, np.log(q) * it, f32(-np.inf)).astype(f32)
        mg = g.max(axis=1)
        with np.errstate(under="ignore"):
            lg = np.log(lc._lane_sum(np.where(pos, np.exp(g - mg[:, None]), f32(0.0)).astype(f32)))
            qt = np.where(pos, np.exp((g - mg[:, None]) - lg[:, None]), f32(0.0)).astype(f32)
        if wrong == "raw_q":
            qt = q
    else:
        qt, pt, lpt = q, p, lp
    sq = lc._lane_sum(qt)
    with np.errstate(under="ignore"):
        sk = lc._lane_sum(np.where(qt != 0, qt * lpt, f32(0.0)).astype(f32))
    ws = np.ones(n, f32) if wrong == "drop_class_weight" else wy
    wg, wl = a_grad * ws, a_loss * ws
    d = om_alpha * d + wg[:, None] * (pt * sq[:, None] - qt)
    d = s_i[:, None] * d
    l = (om_alpha * lb + wl * (-sk)) * s_i
    assert d.dtype == np.float32 and l.dtype == np.float32
    return d, l


# ---- a float64 student for the evidence test ------------------------------------------------------------------------------------
class StudentRef:
    """A Linear -> ReLU -> Linear head trained in float64 by Adam on mini-batches of the distillation loss (mean reduction, no class
    weights): ``l_i = (1 - alpha) nll_i + alpha tau^2 k_i`` with ``k_i`` against the given per-row targets; alpha = 0 is the plain
    cross-entropy of oracle/mlp_train_ref.py, which takes no soft targets."""

    def __init__(self, W, b, lr=3e-3, l2=1e-4, alpha=0.0, tau=1.0):
        self.W = [np.array(w, np.float64) for w in W]
        self.b = [np.array(v, np.float64) for v in b]
        self.m = [np.zeros_like(p) for p in self.W + self.b]
        self.v = [np.zeros_like(p) for p in self.W + self.b]
        self.lr, self.l2, self.alpha, self.tau, self.t = lr, l2, alpha, tau, 0

    def logits(self, X):
        h = np.asarray(X, np.float64)
        self._h = [h]
        for i, (w, b) in enumerate(zip(self.W, self.b)):
            h = h @ w.T + b
            if i < len(self.W) - 1:
                h = np.maximum(h, 0.0)
            self._h.append(h)
        return h

    @staticmethod
    def _log_softmax(z):
        z = z - z.max(axis=1, keepdims=True)
        return z - np.log(np.exp(z).sum(axis=1, keepdims=True))

    def step(self, X, y, qt):
        mb = len(y)
        z = self.logits(X)
        logp = self._log_softmax(z)
        dz = np.exp(logp)
        dz[np.arange(mb), y] -= 1.0
        dz *= (1.0 - self.alpha)
        if self.alpha:
            pt = np.exp(self._log_softmax(z / self.tau))
            dz += self.alpha * self.tau * (pt * qt.sum(axis=1, keepdims=True) - qt)
        dz /= mb
        grads_W, grads_b = [None] * len(self.W), [None] * len(self.W)
        for l in range(len(self.W) - 1, -1, -1):
            grads_W[l] = dz.T @ self._h[l] + (self.l2 / mb) * self.W[l]
            grads_b[l] = dz.sum(axis=0)
            if l > 0:
                dz = (dz @ self.W[l]) * (self._h[l] > 0)
        self.t += 1
        c1, c2 = 1.0 - 0.9 ** self.t, 1.0 - 0.999 ** self.t
        for i, (P, g) in enumerate(zip(self.W + self.b, grads_W + grads_b)):
            self.m[i] = 0.9 * self.m[i] + 0.1 * g
            self.v[i] = 0.999 * self.v[i] + 0.001 * g * g
            P -= self.lr / c1 * self.m[i] / (np.sqrt(self.v[i] / c2) + 1e-8)

    def partial_fit(self, X, y, qt, batch_size, random_state):
        order = np.arange(len(y))
        np.random.default_rng(int(random_state)).shuffle(order)
        for s in range(0, len(y), batch_size):
            rows = order[s:s + batch_size]
            self.step(X[rows], y[rows], None if qt is None else qt[rows])

    def predict_proba(self, X):
        return np.exp(self._log_softmax(self.logits(X)))
