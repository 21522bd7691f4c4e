"""What tests/test_group_dro_host.py and tests/test_gpu_group_dro.py share: the float64 checker of group-robust training
(include/mmc.h, "group-robust training": per-row weights and group DRO in the loss stage), the per-element bounds, a numpy fp32
emulation of the stage, and the inputs both are run on.  Not a test module.

The checker is the definition.  The row term l_i and its logit gradient dl_i/dz come from torch autograd in float64, as in
tests/loss_checker.py but before any normalisation; with r_i the row weight, w the class weights and v_i = r_i w[y_i]::

    no groups   g = 1 / sum_i v_i                 dlogits_i = (r_i g) dl_i        row_loss_i = (r_i g) l_i
    groups      R_i = r_i l_i, D_i = r_i dl_i     V_a = sum_{i in a} v_i          S_a = sum_{i in a} R_i       L_a = S_a / V_a (V_a > 0)
                logq_a += eta L_a (those a)       logq_a -= logsumexp(logq)       c_i = exp(logq_{a_i}) / V_{a_i} (0 where V = 0)
                dlogits_i = c_i D_i               row_loss_i = c_i R_i

Bounds, in units of ULP = 2^-24, the relative error of one fp32 rounding.  tests/loss_checker.py bounds the unweighted stage by
128 units of ``g w_max`` on dlogits and 96 units of ``|l_i g| + g w_max`` on row_loss, g the stage's normaliser.  Here every row has
its own normaliser n_i, which replaces g in those two expressions (``base`` below), and the extra fp32 operations add theirs:

    no groups   n_i = s_i = fl(r_i g): one more rounded product than the unweighted kernel, relative error <= 1 unit, so
                  |err| <= base_i + 1 ULP (|ref| + base_i)
    groups      the stage runs with n_i = fl(r_i 1.0f) = r_i exactly: |err R_i| <= bR_i = 96 ULP (|R_i| + r_i w_max), likewise bD.
                log q: the device sums the fp32 R_i in double, so |err S_a| <= sum_{i in a} bR_i and, before normalisation,
                  delta_a = eta (sum_{i in a} bR_i) / V_a   (0 for a group without loss).  logsumexp is 1-Lipschitz in the maximum
                  norm, so the normaliser moves by at most max_b delta_b and
                  |err logq_a| <= bq_a = delta_a + max_b delta_b + slack_a,   slack_a = 2^-40 (1 + |logq_a| + eta |L_a|)
                  for the double arithmetic (sums of at most 16384 terms, exp, log: far below 2^-40 relative).
                c_i = fl32(exp(logq_a) / V_a): relative error <= expm1(bq_a) + 1 unit (the cast); the product c_i D_i one more:
                  |err| <= c_i bD_i + (expm1(bq_a) + 2 ULP) (|ref| + c_i bD_i)       and the same with R for row_loss
                  (c_i bD_i is ``base`` with n_i = c_i r_i).

tests/test_group_dro_host.py runs ``emulate`` -- numpy fp32, operation for operation in the kernels' order -- on every shared input:
its peak is 0.029 of the dlogits bound, 0.050 of the row_loss bound and 0.023 of the log q bound (the values that test prints); the rest
is room for a device ``expf`` / ``logf`` / ``powf`` that differs from numpy's by a few ulp, as in tests/loss_checker.py."""

import numpy as np

import loss_checker as lc

ULP = lc.ULP
EXTRA_ROWS_UNITS = 1.0      # no groups: the product r_i g
EXTRA_GROUP_UNITS = 2.0     # groups: the cast of c_i and the product c_i D_i
SLACK = 2.0 ** -40
MAX_GROUPS = 1024
DRO_TILE = 2048             # dro_update_kernel's tile of rows


# ---- the shared inputs ----------------------------------------------------------------------------------------------------------
N_ROWS, MB = 17, 7                                    # three steps of 7, 7 and 3 rows; loss blocks of 4 rows with a ragged tail
# G = 3 by position: group 2 has only zero-mass rows in mini-batch 0 (weights 0 at positions 2 and 5), group 1 is absent from
# mini-batch 1, all three are present in mini-batch 2
GROUPS3 = np.array([0, 1, 2, 0, 1, 2, 0,  0, 2, 2, 0, 2, 0, 0,  1, 2, 0], np.int32)
ZERO_WEIGHT = (2, 5, 10)                              # positions with r = 0 exactly (10: a zero inside a group that has mass)
LOSS_KINDS = (("plain", {}), ("general", dict(eps=0.1, gamma=2.0, use_prior=True)))
ETAS = (0.0, 0.5)


def row_groups(G):
    if G == 3:
        return GROUPS3.copy()
    if G == 1:
        return np.zeros(N_ROWS, np.int32)
    return np.array([0, 517, 1023], np.int32)[GROUPS3]          # G = 1024 with three groups present


def inputs(K, seed=0):
    """-> dict: 17 logit rows z, labels y, class weights w (one class at zero), row weights r spanning 1e-3 .. 1e3 with zeros, a
    logit prior.  Every mini-batch of 7 keeps a row of positive mass in group 0."""
    rng = np.random.default_rng([K, seed])
    z, y = lc.logit_rows(rng, N_ROWS, K, 4.0)
    w = lc.class_weights(rng, K)
    live = int(np.flatnonzero(w > 0)[0])
    r = (10.0 ** rng.uniform(-3.0, 3.0, N_ROWS)).astype(np.float32)
    r[0], r[-1] = np.float32(1e-3), np.float32(1e3)
    r[list(ZERO_WEIGHT)] = 0.0
    y = y.copy()
    y[[0, 7, 16]] = live                                          # positions of group 0 in each mini-batch: mass > 0
    return dict(z=z, y=y, w=w, r=r, prior=lc.dirichlet_prior(rng, K))


def uniform_logq(G):
    return np.full(G, -np.log(float(G)))


def skewed_logq(G, seed=3):
    q = np.random.default_rng(seed).dirichlet(np.ones(G))
    return np.log(np.maximum(q, 1e-300) / q.sum())


def stage_cases():
    """Every (name, K, G, rows slice, eta, loss kind, options, logq) the per-element test runs: the whole pass as one mini-batch
    and its first two mini-batches on their own (a group without mass; an absent group)."""
    out = []
    for K in (5, 70):
        for G in (3, 1, 1024):
            for sl in (slice(0, N_ROWS), slice(0, MB), slice(MB, 2 * MB)):
                for eta in ETAS:
                    for kind, opts in LOSS_KINDS:
                        for qname, logq in (("uniform", uniform_logq(G)), ("skewed", skewed_logq(G))):
                            if qname == "skewed" and (sl.start != 0 or sl.stop != N_ROWS):
                                continue
                            out.append((f"K{K} G{G} rows{sl.start}:{sl.stop} eta{eta} {kind} {qname}", K, G, sl, eta, kind, opts, logq))
    return out


def loss_options(opts, prior):
    """The keyword arguments of ``row_terms`` / ``emulate`` for a loss kind."""
    return dict(eps=opts.get("eps", 0.0), gamma=opts.get("gamma", 0.0), prior=prior if opts.get("use_prior") else None)


# ---- the definition in float64 ----------------------------------------------------------------------------------------------------
def row_terms(z, y, w=None, prior=None, eps=0.0, gamma=0.0):
    """-> (dl [n][K], l [n]) float64: the trainer's row term and its logit gradient before normalisation (torch autograd)."""
    import torch
    n, K = z.shape
    u32 = z if prior is None else (z + prior[None, :]).astype(np.float32)
    u = torch.tensor(u32.astype(np.float64), requires_grad=True)
    yt = torch.tensor(np.asarray(y, np.int64))
    wt = torch.ones(K, dtype=torch.float64) if w is None else torch.tensor(w.astype(np.float64))
    logp = torch.log_softmax(u, dim=1)
    logpt = logp.gather(1, yt[:, None])[:, 0]
    q = -torch.expm1(logpt)
    m = q ** gamma if gamma != 0.0 else torch.ones_like(q)
    l = (1.0 - eps) * wt[yt] * m * -logpt + (eps / K) * -(logp * wt[None, :]).sum(dim=1)
    l.sum().backward()
    return u.grad.numpy().copy(), l.detach().numpy().copy()


def masses(y, w, r):
    wy = np.ones(len(y)) if w is None else w.astype(np.float64)[np.asarray(y)]
    rr = np.ones(len(y)) if r is None else r.astype(np.float64)
    return rr * wy


def logsumexp(x):
    mx = float(np.max(x))
    s = 0.0
    for v in x.tolist():
        s += np.exp(v - mx)
    return mx + np.log(s)


def checker(z, y, w=None, r=None, a=None, logq=None, eta=0.0, G=0, **loss):
    """-> dict: dlogits, row_loss (float64), and with groups logq, group_loss (NaN where none), c, V, R, D, q."""
    dl, l = row_terms(z, y, w, **loss)
    v = masses(y, w, r)
    rr = np.ones(len(y)) if r is None else r.astype(np.float64)
    if a is None:
        g = 1.0 / float(np.sum(v))
        s = rr * g
        return dict(dlogits=s[:, None] * dl, row_loss=s * l, s=s)
    a = np.asarray(a)
    R, D = rr * l, rr[:, None] * dl
    V, S = np.zeros(G), np.zeros(G)
    np.add.at(V, a, v)
    np.add.at(S, a, R)
    has = V > 0
    L = np.full(G, np.nan)
    L[has] = S[has] / V[has]
    lq = np.asarray(logq, np.float64).copy()
    lq[has] = lq[has] + eta * L[has]
    lq = lq - logsumexp(lq)
    cg = np.where(has, np.exp(lq) / np.where(has, V, 1.0), 0.0)
    c = cg[a]
    return dict(dlogits=c[:, None] * D, row_loss=c * R, logq=lq, group_loss=L, c=c, V=V, R=R, D=D, r=rr)


def bounds(ref, y, w, r=None, a=None, eta=0.0, G=0):
    """-> dict of bounds for ``checker``'s dict ``ref``: dlogits [n][K], row_loss [n], and with groups logq [G] (see the module
    docstring for the derivation)."""
    wmax = 1.0 if w is None else float(w.max())
    if a is None:
        s = ref["s"]
        bd = lc.DLOGITS_UNITS * ULP * s * wmax
        bl = lc.ROW_LOSS_UNITS * ULP * (np.abs(ref["row_loss"]) + s * wmax)
        x = EXTRA_ROWS_UNITS * ULP
        return dict(dlogits=bd[:, None] + x * (np.abs(ref["dlogits"]) + bd[:, None]), row_loss=bl + x * (np.abs(ref["row_loss"]) + bl))
    a = np.asarray(a)
    rr, R, V, c = ref["r"], ref["R"], ref["V"], ref["c"]
    bR = lc.ROW_LOSS_UNITS * ULP * (np.abs(R) + rr * wmax)
    bD = lc.DLOGITS_UNITS * ULP * rr * wmax
    has = V > 0
    delta = np.zeros(G)
    np.add.at(delta, a, bR)
    delta = np.where(has, eta * delta / np.where(has, V, 1.0), 0.0)
    L = np.where(has, np.nan_to_num(ref["group_loss"]), 0.0)
    bq = delta + float(delta.max()) + SLACK * (1.0 + np.abs(ref["logq"]) + eta * np.abs(L))
    rel = np.expm1(bq)[a] + EXTRA_GROUP_UNITS * ULP
    base_d, base_l = c * bD, c * bR
    return dict(dlogits=base_d[:, None] + rel[:, None] * (np.abs(ref["dlogits"]) + base_d[:, None]),
                row_loss=base_l + rel * (np.abs(ref["row_loss"]) + base_l), logq=bq)


# ---- the stage in numpy fp32, operation for operation ------------------------------------------------------------------------------
def _ce_rows(z, y, w, norm, prior=None, eps=0.0, gamma=0.0):
    """ce_grad_rows with the per-row normaliser ``norm`` (fp32 [n]) where the kernel reads inv_wsum: the plain instantiation when
    no loss option is set, the general one otherwise (tests/loss_checker.py's ``emulate`` with a vector normaliser)."""
    f32 = np.float32
    n, K = z.shape
    y = np.asarray(y)
    rows = np.arange(n)
    wy = np.ones(n, f32) if w is None else w[y]
    onehot = np.zeros((n, K), f32)
    onehot[rows, y] = 1.0
    if prior is None and eps == 0.0 and gamma == 0.0:
        mx = z.max(axis=1, keepdims=True)
        s = lc._lane_sum(np.exp(z - mx))
        lse = np.log(s)
        g = wy * norm
        p = np.exp((z - mx) - lse[:, None])
        d = g[:, None] * (p - onehot)
        l = wy * (lse - (z[rows, y] - mx[:, 0])) * norm
        assert d.dtype == np.float32 and l.dtype == np.float32
        return d, l
    om_eps, eps_k, gam = f32(1.0 - eps), f32(eps / K), f32(gamma)
    w_total = f32(K) if w is None else f32(sum(float(v) for v in w))
    u = z if prior is None else (z + prior[None, :]).astype(f32)
    mx = u.max(axis=1, keepdims=True)
    e = np.exp(u - mx)
    s = lc._lane_sum(e)
    eo = e.copy()
    eo[rows, y] = 0.0
    so = lc._lane_sum(eo)
    lse = np.log(s)
    lp = (u - mx) - lse[:, None]
    sw = lc._lane_sum(lp if w is None else w[None, :] * lp)
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
    aa = om_eps * wy
    af = aa * f
    p = np.exp(lp)
    d = af[:, None] * (p - onehot)
    l = aa * m * nll
    if eps_k != 0:
        wc = np.ones(K, f32) if w is None else w
        d = d + eps_k * (p * w_total - wc[None, :])
        l = l - eps_k * sw
    d = norm[:, None] * d
    l = l * norm
    assert d.dtype == np.float32 and l.dtype == np.float32
    return d, l


def group_sums(R32, a, G):
    """S_a as dro_update_kernel forms it: double sums of the fp32 R_i, per slice of each tile in position order, slices in order."""
    M = len(R32)
    NS = 16 // ((G + 63) // 64)
    part = np.zeros((NS, G))
    for r0 in range(0, M, DRO_TILE):
        rows = min(DRO_TILE, M - r0)
        per = (rows + NS - 1) // NS
        for s in range(NS):
            for i in range(s * per, min(rows, (s + 1) * per)):
                part[s, a[r0 + i]] += float(R32[r0 + i])
    S = np.zeros(G)
    for s in range(NS):
        S = S + part[s]
    return S


def emulate(z, y, w=None, r=None, a=None, logq=None, eta=0.0, G=0, **loss):
    """-> (dlogits fp32, row_loss fp32, logq float64 or None): the stage as the kernels compute it."""
    f32 = np.float32
    n = len(y)
    v = masses(y, w, r)
    if a is None:
        tot = 0.0
        for x in v.tolist():
            tot += x
        g = f32(1.0 / tot)
        norm = np.full(n, g, f32) if r is None else r * g
        d, l = _ce_rows(z, y, w, norm.astype(f32), **loss)
        return d, l, None
    a = np.asarray(a)
    norm = np.ones(n, f32) if r is None else r * f32(1.0)
    D, R = _ce_rows(z, y, w, norm, **loss)
    V = np.zeros(G)
    for i in range(n):
        V[a[i]] += v[i]
    S = group_sums(R, a, G)
    has = V > 0
    lq = np.asarray(logq, np.float64).copy()
    lq[has] = lq[has] + eta * (S[has] / V[has])
    lq = lq - logsumexp(lq)
    cg = np.where(has, np.exp(lq) / np.where(has, V, 1.0), 0.0).astype(f32)
    c = cg[a]
    d, l = c[:, None] * D, c * R
    assert d.dtype == np.float32 and l.dtype == np.float32
    return d, l, lq


def ratios(got_d, got_l, got_q, ref, bnd):
    """-> (dlogits, row_loss, logq) peak error over bound (0 where error and bound are both 0; logq None without groups)."""
    def peak(err, b):
        err, b = np.asarray(err, np.float64), np.asarray(b, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0.0, 0.0, err / b)
        return float(np.max(q))
    rd = peak(np.abs(got_d.astype(np.float64) - ref["dlogits"]), bnd["dlogits"])
    rl = peak(np.abs(got_l.astype(np.float64) - ref["row_loss"]), bnd["row_loss"])
    rq = None if got_q is None else peak(np.abs(got_q - ref["logq"]), bnd["logq"])
    return rd, rl, rq
