"""What tests/test_hier_loss_host.py and tests/test_gpu_hier_loss.py share: the fp64 checker of the taxonomy-aware loss (level-marginal
terms and soft labels: include/mmc.h, ``mmc_trainer_set_hierarchy``), the per-element bounds, a numpy fp32 emulation of
``ce_grad_rows_hier``'s arithmetic, the level arrays and the logit rows both are run on.  Not a test module.

The checker is the definition, evaluated by torch autograd in fp64 on the fp32-rounded u::

    u      = z + o                                  (fp32 add, per element)
    logp   = log_softmax(u),  t = y_i,  w_t the class weight
    base   = the general form of tests/loss_checker.py, or with T:  w_t (-sum_c T[t,c] logp_c)
    h_i    = w_t sum_l lam_l (logsumexp_c u_c - logsumexp_{c : g_l(c) = g_l(t)} u_c)       over the levels with g_l(t) >= 0
    l_i    = (base + h_i) s_i,   s_i = 1 / sum_i w[y_i], or r_i / sum_i r_i w[y_i] on the row-weighted route (in double here)

Bounds, per element, in units of ULP = 2^-24, counted from the kernel's operations.  A correctly rounded fp32 operation errs by at
most one unit of its result; a device ``expf`` / ``logf`` within 2 ulp by TRANS = 4 units.  With S(K) = ceil(K / 64) - 1 + 6 the
roundings of a lane-strided sum and its butterfly (the first add, to zero, is exact):

* ``lse = logf(s)``, s = sum_c expf(u_c - mx) >= 1.  A term carries TRANS for expf and at most 1 for the rounding of u_c - mx (an
  error of |a| units in the argument a <= 0 moves e^a by |a| e^a <= 1/e units); the sum adds S(K).  So s is off by S + TRANS + 1
  units relative, which is lse's absolute error, and logf adds TRANS |lse| <= TRANS ln K:
  ``E_lse(K) = S(K) + TRANS + 1 + TRANS ln K`` units, absolute.  The same holds for a node's ``lS_l`` (its sum is >= 1 too).
* ``p = expf((u - mx) - lse)``: the two roundings of the argument move p by at most 2 |a| e^a < 1 unit, lse's error by E_lse p,
  expf by TRANS p:  ``E_p(K) = E_lse(K) + TRANS + 1``.  The softmax inside a node is the same expression on the node's own sum.
* ``dlogits``.  A level's term lam_l (p - pin) errs by lam_l (2 E_p + 1 [the subtraction] + 1 [the product]), and the running sum hd
  adds one rounding per level (at most 4) of magnitude <= sum lam: (2 E_p + 6) sum_l lam_l.  Then w hd, d + w hd, s_i d, the product
  s_i = rw inv_wsum and the cast of inv_wsum: 5 roundings of magnitude (1 + sum lam) w_max.  The base keeps the 128 units of tests/loss_checker.py; the soft-label
  base w (p st - T) needs E_p + S + 3 of them.  In all
  ``(DLOGITS_UNITS + 5 + (2 E_p(K) + 11) sum_l lam_l)  ULP  s_i w_max``.
* ``row_loss``.  -log P_l = (mx + lse) - (m_l + lS_l): the two inner sums round once each at magnitude <= max|u| + ln K, lse and lS
  are off by E_lse each, and the subtraction rounds once at the magnitude of the result.  Times lam_l w_t that is
  lam_l w_t (2 E_lse + 2 (max|u| + ln K)) absolute.  The operations on the result -- that subtraction, lam_l times, the running sum
  (at most 4), w h, base + w h, times s_i, s_i's own product and cast -- are 7 + 4 roundings relative to the row loss (every term is >= 0, so no
  partial sum exceeds it).  The base keeps 96 units of |l_i| + s_i w_max (the soft-label base needs E_lse + 12 of them).  In all
  ``(ROW_LOSS_UNITS + 11) ULP |l_i|  +  (ROW_LOSS_UNITS + sum_l lam_l (2 E_lse(K) + 2 (max|u| + ln K)))  ULP  s_i w_max``.

The factor sum lam enters exactly where the level terms add, and the row-loss bound carries the term in max|u| 2^-24 because -log P_l
is a difference of two log-sum-exps whose absolute error follows their magnitude."""

import math

import numpy as np

import loss_checker as lc

ULP = lc.ULP
TRANS = 4.0
MAX_LEVELS = 4


def sum_units(K):
    return math.ceil(K / 64) - 1 + 6


def e_lse(K):
    return sum_units(K) + TRANS + 1 + TRANS * math.log(K)


def e_p(K):
    return e_lse(K) + TRANS + 1


def dlogits_units(K, lam):
    return lc.DLOGITS_UNITS + 5 + (2 * e_p(K) + 11) * float(np.sum(_lam32(lam)))


# ---- levels and rows --------------------------------------------------------------------------------------------------------------
def level_bank(K):
    """Four levels [4][K] int32.  0 "rest": every class but the last shares node 0, the last is alone.  1 "branches": three contiguous
    branches.  2 "span": classes 60..70 share a node when K > 70 (lanes on both sides of class 64), pairs otherwise; every fifth
    class has no node.  3 "leaf": every class its own node; class 1 has none."""
    c = np.arange(K)
    rest = np.where(c < K - 1, 0, K - 1)
    branch = np.minimum(c * 3 // K, 2)
    first = np.array([int(np.flatnonzero(branch == b)[0]) for b in range(3)])
    branches = first[branch]
    span = c // 2 * 2
    if K > 70:
        span[60:71] = 60
    span[c % 5 == 4] = -1
    leaf = c.copy()
    leaf[1] = -7
    return np.stack([rest, branches, span, leaf]).astype(np.int32)


def levels_for(K, L):
    return None if L == 0 else level_bank(K)[:L].copy()


def hier_rows(rng, n, K, scale, levels):
    """``loss_checker.logit_rows`` (its four special rows included) plus two rows.  The first: the true class K - 1 and every class that
    shares a node with it at any level sit 120 below the others, so every member of each true node underflows against the row maximum.
    The second: true class 0, whose node at level "rest" holds every class but the last, that one at -60."""
    z, y = lc.logit_rows(rng, n, K, scale)
    extra = np.zeros((2, K), np.float32)
    members = np.zeros(K, bool)
    members[K - 1] = True
    if levels is not None:
        for ids in levels:
            if ids[K - 1] >= 0:
                members |= ids == ids[K - 1]
    assert not members.all()
    extra[0, members] = -120.0
    extra[1, K - 1] = -60.0
    return np.concatenate([z, extra]), np.concatenate([y, np.array([K - 1, 0])]).astype(np.int64)


def soft_targets(rng, K):
    """A K x K fp32 T: 0.7 on the diagonal, the rest spread at random over the class's siblings at level "branches" (over every other
    class where it has none), zeros elsewhere; rows renormalised in double, so they sum to 1 within fp32 rounding."""
    T = np.zeros((K, K), np.float64)
    group = level_bank(K)[1]
    for t in range(K):
        sib = np.flatnonzero((group == group[t]) & (np.arange(K) != t))
        if not len(sib):                                                       # a branch of one class: every other class
            sib = np.flatnonzero(np.arange(K) != t)
        T[t, t] = 0.7
        m = rng.uniform(0.1, 1.0, len(sib))
        T[t, sib] = 0.3 * m / m.sum()
    T = (T / T.sum(axis=1, keepdims=True)).astype(np.float32)
    assert np.abs(T.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6
    return T


def _lam32(lam):
    return np.zeros(0, np.float32) if lam is None else np.asarray(lam, np.float64).astype(np.float32)


def normaliser(y, w, row_weight=None, inv_wsum=None, exact=False):
    """s_i -> [n].  As the library forms it, fp32: (float)(1 / sum_i w[y_i]), or rw_i times (float)(1 / sum of the row masses), one
    rounded fp32 product (``inv_wsum`` given: rw_i times that, the route with groups, where it is 1).  ``exact=True``: the definition's
    float64 value, for the checker."""
    y = np.asarray(y)
    if row_weight is None:
        g = 1.0 / lc.weight_sum(y, w)
        return np.full(len(y), g) if exact else np.full(len(y), np.float32(g), np.float32)
    rw = np.asarray(row_weight, np.float32)
    if inv_wsum is None:
        mass = 0.0
        for i in range(len(y)):
            mass += float(rw[i]) * (1.0 if w is None else float(w[y[i]]))
        inv_wsum = 1.0 / mass
    return rw.astype(np.float64) * inv_wsum if exact else (rw * np.float32(inv_wsum)).astype(np.float32)


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def checker(z, y, w=None, prior=None, eps=0.0, gamma=0.0, levels=None, lam=None, T=None, norm=None):
    """-> (dlogits [n][K] fp64, row_loss [n] fp64 = l_i, L fp64 = sum_i l_i).  ``norm``: the rows' normalisers s_i in float64
    (``normaliser(exact=True)``); None: 1 / sum_i w[y_i]."""
    import torch
    n, K = z.shape
    u32 = z if prior is None else (z + prior[None, :]).astype(np.float32)
    u = torch.tensor(u32.astype(np.float64), requires_grad=True)
    yt = torch.tensor(np.asarray(y, np.int64))
    wt = torch.ones(K, dtype=torch.float64) if w is None else torch.tensor(w.astype(np.float64))
    logp = torch.log_softmax(u, dim=1)
    if T is None:
        logpt = logp.gather(1, yt[:, None])[:, 0]
        q = -torch.expm1(logpt)
        m = q ** gamma if gamma != 0.0 else torch.ones_like(q)
        base = (1.0 - eps) * wt[yt] * m * -logpt + (eps / K) * -(logp * wt[None, :]).sum(dim=1)
    else:
        assert eps == 0.0 and gamma == 0.0
        Tt = torch.tensor(np.asarray(T, np.float32).astype(np.float64))[yt]
        base = wt[yt] * -(Tt * logp).sum(dim=1)
    h = torch.zeros(n, dtype=torch.float64)
    if levels is not None:
        all_lse = torch.logsumexp(u, dim=1)
        for ids, lam_l in zip(np.asarray(levels), _lam32(lam).astype(np.float64)):
            ids_t = torch.tensor(ids.astype(np.int64))
            gt = ids_t[yt]
            has = gt >= 0
            mask = (ids_t[None, :] == gt[:, None]) | ~has[:, None]           # a row without a node: any finite value, times 0 below
            node_lse = torch.logsumexp(u.masked_fill(~mask, -math.inf), dim=1)
            h = h + float(lam_l) * has.to(torch.float64) * (all_lse - node_lse)
    s = torch.tensor(normaliser(y, w, exact=True) if norm is None else np.asarray(norm, np.float64))
    l = (base + wt[yt] * h) * s
    L = l.sum()
    L.backward()
    return u.grad.numpy().copy(), l.detach().numpy().copy(), float(L.detach())


def bounds(z, y, w, row_loss_ref, prior=None, lam=None, norm=None):
    """-> (bound on the dlogits elements of every row [n][1], bound per row_loss element [n]); see the module docstring."""
    n, K = z.shape
    wmax = 1.0 if w is None else float(w.max())
    s = normaliser(y, w, exact=True) if norm is None else np.asarray(norm, np.float64)
    u = z if prior is None else (z + prior[None, :]).astype(np.float32)
    umax = np.abs(u.astype(np.float64)).max(axis=1)
    sl = float(np.sum(_lam32(lam).astype(np.float64)))
    bd = dlogits_units(K, lam) * ULP * s * wmax
    bl = ULP * ((lc.ROW_LOSS_UNITS + 11) * np.abs(row_loss_ref)
                + (lc.ROW_LOSS_UNITS + sl * (2 * e_lse(K) + 2 * (umax + math.log(K)))) * s * wmax)
    return bd[:, None], bl


# ---- the kernel's arithmetic in numpy fp32 ------------------------------------------------------------------------------------------
def _emulate_level(u, p, top, ids, gt, lam_l, h, hd):
    """One level of ``emulate``: the true node's maximum and sum, its term of h and of the gradient."""
    f32 = np.float32
    has = gt >= 0
    mask = (ids[None, :] == gt[:, None]) & has[:, None]
    safe = mask | ~has[:, None]                                                # rows without a node: computed and thrown away
    m_l = np.where(safe, u, f32(-np.inf)).max(axis=1)
    sn = lc._lane_sum(np.where(safe, np.exp(u - m_l[:, None]), f32(0.0)).astype(f32))
    lS = np.log(sn)
    h = np.where(has, h + lam_l * (top - (m_l + lS)), h).astype(f32)
    pin = np.where(mask, np.exp((u - m_l[:, None]) - lS[:, None]), f32(0.0)).astype(f32)
    hd = np.where(has[:, None], hd + lam_l * (p - pin), hd).astype(f32)
    return h, hd


def emulate(z, y, w=None, prior=None, eps=0.0, gamma=0.0, levels=None, lam=None, T=None, norm=None, drop_level=None,
            wrong_group=False, drop_class_weight=False, onehot_for_T=False):
    """``ce_grad_rows_hier`` in numpy fp32, operation for operation -> (dlogits, row_loss) fp32.  The flags build the wrong kernels
    the bounds have to catch: ``drop_level=l`` leaves level l out, ``wrong_group`` takes P_l over the node of the row's argmax instead
    of the true class's, ``drop_class_weight`` leaves w_t off the level terms, ``onehot_for_T`` reads the identity for T."""
    f32 = np.float32
    n, K = z.shape
    y = np.asarray(y)
    rows = np.arange(n)
    lam = _lam32(lam)
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
    if T is not None:
        Tt = onehot if onehot_for_T else np.asarray(T, f32)[y]
        st = lc._lane_sum(Tt)
        sl = lc._lane_sum(Tt * lp)
        lb = -(wy * sl)
        d = wy[:, None] * (p * st[:, None] - Tt)
    else:
        om_eps, eps_k, gam = f32(1.0 - eps), f32(eps / K), f32(gamma)
        w_total = f32(K) if w is None else f32(sum(float(v) for v in w))
        ut = u[rows, y]
        nll = lse - (ut - mx)
        if gam != 0:
            q = so / s
            pt = np.exp((ut - mx) - lse)
            pw = np.power(q, f32(gam - f32(1.0)))
            m = pw * q
            f = m + gam * pt * pw * nll
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
    top = mx + lse
    h = np.zeros(n, f32)
    hd = np.zeros((n, K), f32)
    if levels is not None:
        of = u.argmax(axis=1) if wrong_group else y
        for l, ids in enumerate(np.asarray(levels)):
            if drop_level == l:
                continue
            with np.errstate(over="ignore"):                                   # exp over the classes outside the node is thrown away
                h, hd = _emulate_level(u, p, top, ids, ids[of], lam[l], h, hd)
    wl = np.ones(n, f32) if drop_class_weight else wy
    d = d + wl[:, None] * hd
    d = s_i[:, None] * d
    l = (lb + wl * h) * s_i
    assert d.dtype == np.float32 and l.dtype == np.float32
    return d, l


# ---- the route with groups: group DRO on top of the stage (tests/group_dro_checker.py's composition) ---------------------------------
def with_groups(D, R, bD, bR, v, a, logq, eta, G):
    """The stage's D_i = r_i dl_i and R_i = r_i l_i (float64, normaliser r_i) and their bounds -> (ref, bounds), dicts of dlogits,
    row_loss and logq after the DRO update, composed exactly as tests/group_dro_checker.py composes them: S_a and V_a in double,
    logq_a += eta S_a / V_a, renormalised, c_i = exp(logq_a) / V_a; |err logq_a| <= delta_a + max delta + slack with
    delta_a = eta sum_{i in a} bR_i / V_a, and c_i off by expm1 of that plus 2 units (its cast, its product)."""
    a = np.asarray(a)
    V, S, delta = np.zeros(G), np.zeros(G), np.zeros(G)
    np.add.at(V, a, v)
    np.add.at(S, a, R)
    np.add.at(delta, a, bR)
    has = V > 0
    L = np.where(has, S / np.where(has, V, 1.0), 0.0)
    lq = np.asarray(logq, np.float64) + np.where(has, eta * L, 0.0)
    mx = lq.max()
    lq = lq - (mx + np.log(np.exp(lq - mx).sum()))
    c = np.where(has, np.exp(lq) / np.where(has, V, 1.0), 0.0)[a]
    delta = np.where(has, eta * delta / np.where(has, V, 1.0), 0.0)
    bq = delta + float(delta.max()) + 2.0 ** -40 * (1.0 + np.abs(lq) + eta * np.abs(L))
    rel = np.expm1(bq)[a] + 2.0 * ULP
    ref = dict(dlogits=c[:, None] * D, row_loss=c * R, logq=lq)
    base_d, base_l = c[:, None] * bD, c * bR
    return ref, dict(dlogits=base_d + rel[:, None] * (np.abs(ref["dlogits"]) + base_d),
                     row_loss=base_l + rel * (np.abs(ref["row_loss"]) + base_l), logq=bq)
