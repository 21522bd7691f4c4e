"""Cover estimation, host side: the identities of the numpy checker (tests/cover_checker.py, which follows include/mmc.h), the
label-shift property the feature exists for, CoverEstimate.compare against a restatement of the reference's compute_cover, and the
argument checks the Python front-ends make before the device is touched.  No GPU."""

import numpy as np
import pytest

import cover_checker as cc


@pytest.fixture(scope="module")
def mixture():
    return cc.mixture_trials()


@pytest.fixture(scope="module")
def small():
    """90 rows x 7 classes in groups of 1, 25, 0, 64: one NaN row, one infinite row, a Dirichlet train prior."""
    rng = np.random.default_rng(3)
    v = rng.dirichlet(np.full(7, 0.4), 90).astype(np.float32)
    v[5, 2] = np.nan
    v[40, 0] = np.inf
    return v, np.array([0, 1, 26, 26, 90], np.int64), rng.dirichlet(np.full(7, 2.0))


def test_checker_identities(small):
    v, off, tp = small
    for strength in (0.0, 1.0):
        count, soft, unusable, prior = cc.cover(v, off, tp, strength, iters=0)
        assert np.array_equal(prior, np.tile(tp, (4, 1)))                             # iters = 0 gives train_prior
        assert unusable.tolist() == [0, 1, 0, 1]
        n_g = np.diff(off) - unusable
        assert np.array_equal(count.sum(1), n_g)
        ok = cc.usable_rows(v)
        assert np.array_equal(soft.sum(0), np.rint(v[ok].astype(np.float64) * 2.0 ** 32).astype(np.int64).sum(0))
        for iters in (1, 7):
            c2, s2, u2, prior = cc.cover(v, off, tp, strength, iters)
            assert np.array_equal(c2, count) and np.array_equal(s2, soft) and np.array_equal(u2, unusable)
            assert np.allclose(prior.sum(1), 1.0, rtol=0, atol=1e-12)                 # each prior row sums to 1
            assert np.array_equal(prior[2], tp)                                       # the empty group keeps train_prior
            assert (prior > 0).all() or strength == 0
    # one point, no smoothing, one iteration: the prior is the point's own posterior under train_prior (w = 1)
    _, _, _, prior = cc.cover(v[:1], [0, 1], tp, 0.0, 1)
    assert np.allclose(prior[0], v[0].astype(np.float64) / v[0].astype(np.float64).sum(), rtol=1e-15, atol=0)


def test_checker_topk_follows_the_key_rule(small):
    v, off, tp = small
    _, _, _, prior = cc.cover(v, off, tp, 1.0, 5)
    idx, sc, allsc = cc.adapted_topk(v, off, prior, tp, 7)
    assert sorted(idx[5].tolist()) == list(range(7)) and sorted(idx[40].tolist()) == list(range(7))   # unusable rows: 7 distinct classes
    ok = cc.usable_rows(v)
    assert (np.diff(sc[ok], axis=1) <= 0).all()
    assert np.allclose(allsc[ok].astype(np.float64).sum(1), 1.0, atol=1e-6)
    # w = 1 (iters = 0): the adapted order of a usable row is the stable descending order of v / sum v
    idx0, _, _ = cc.adapted_topk(v, off, np.tile(tp, (4, 1)), tp, 3)
    q = (v[ok].astype(np.float64) / v[ok].astype(np.float64).sum(1, keepdims=True)).astype(np.float32)
    assert np.array_equal(idx0[ok], np.argsort(-q, axis=1, kind="stable")[:, :3])


def test_em_recovers_shifted_priors_on_the_mixture_recipe(mixture):
    """The label-shift recipe of the issue: in every trial the adapted prior is closer (L1) to the empirical class frequencies than
    half the better of hard and soft cover.  (Measured with numpy: at most 0.18 x.)"""
    v, y, off = mixture
    count, soft, unusable, prior = cc.cover(v, off, None, strength=1.0, iters=50)
    assert unusable.sum() == 0
    l1 = cc.label_shift_l1(count, soft, prior, y, off)
    ratio = l1[:, 2] / np.minimum(l1[:, 0], l1[:, 1])
    print("L1 hard / soft / adapted per trial:\n", l1, "\nratio", ratio)
    assert (l1[:, 2] < 0.5 * np.minimum(l1[:, 0], l1[:, 1])).all()
    # conditioning: float64 against long double
    _, _, _, wide = cc.cover(v, off, None, 1.0, 50, dtype=np.longdouble)
    assert np.abs(prior - wide.astype(np.float64)).max() < cc.prior_atol(50, 2000) / 64


def _estimate(counts, soft, unusable, sizes, prior):
    from mermaid_classifier_amd import CoverEstimate
    return CoverEstimate(counts, soft, unusable, sizes, prior)


def test_cover_fractions_and_nan_rows(small):
    v, off, tp = small
    count, soft, unusable, prior = cc.cover(v, off, tp, 1.0, 4)
    est = _estimate(count, soft, unusable, np.diff(off), prior)
    assert est.n.tolist() == [1, 24, 0, 63]
    for name in ("hard", "soft", "adapted"):
        c = est.cover(name)
        assert c.shape == (4, 7) and np.isnan(c[2]).all() and np.isfinite(c[[0, 1, 3]]).all()
        assert np.allclose(c[[0, 1, 3]].sum(1), 1.0, atol=1e-6)
    assert np.array_equal(est.hard_cover()[3], count[3] / 63)
    ok = cc.usable_rows(v)
    assert np.allclose(est.soft_cover()[3], v[26:][ok[26:]].astype(np.float64).mean(0), rtol=0, atol=1e-9)
    with pytest.raises(ValueError, match="estimator"):
        est.cover("argmax")


def test_compare_is_compute_cover(mixture):
    """compare() against a direct numpy restatement of cover.py:44-120, on 80 images of 25 points cut from the mixture trials."""
    v, y, _ = mixture
    v, y = v[:2000], y[:2000]
    off = np.arange(81, dtype=np.int64) * 25
    K = v.shape[1]
    count, soft, unusable, prior = cc.cover(v, off, None, 1.0, 10)
    true_counts = np.stack([np.bincount(y[a:b], minlength=K) for a, b in zip(off[:-1], off[1:])])
    est = _estimate(count, soft, unusable, np.diff(off), prior)
    for name, pred in (("hard", count / 25.0), ("soft", soft / 2.0 ** 32 / 25.0), ("adapted", prior)):
        stats = est.compare(true_counts, name)
        cols, scalars = cc.reference_cover_metrics(true_counts / 25.0, pred)
        table = stats.table()
        assert stats.n_images_used == 80 and np.array_equal(table["class"], cols["class"])
        for key in ("mean_true_cover_pct", "bias_pct", "rmse_pct", "mae_pct", "r_squared"):
            assert np.allclose(table[key], cols[key], rtol=1e-12, atol=1e-12, equal_nan=True), (name, key)
        got = stats.scalars()
        for key, want in scalars.items():
            assert got[key] == pytest.approx(want, rel=1e-12, abs=1e-12), (name, key)
    # a group without a usable point, or without a true label, is left out
    unusable2 = unusable.copy()
    unusable2[3] = 25
    count2 = count.copy()
    count2[3] = 0
    true2 = true_counts.copy()
    true2[7] = 0
    est2 = _estimate(count2, soft, unusable2, np.diff(off), prior)
    assert est2.compare(true2, "hard").n_images_used == 78
    with pytest.raises(ValueError, match="true_counts"):
        est.compare(true_counts[:-1], "hard")
    with pytest.raises(ValueError, match="true_counts"):
        est.compare(true_counts.astype(np.float64), "hard")


def test_prior_from_labels():
    from mermaid_classifier_amd import prior_from_labels
    p = prior_from_labels(np.array([0, 2, 2, 1, 2, 0]), 3)
    assert p.dtype == np.float64 and np.array_equal(p, np.array([2, 1, 3]) / 6)
    assert np.array_equal(prior_from_labels(np.array([0, 0, 2]), 3, pseudo_count=1.0), np.array([3, 1, 2]) / 6)
    with pytest.raises(ValueError, match="no label"):
        prior_from_labels(np.array([0, 0, 2]), 3)
    with pytest.raises(ValueError, match="outside"):
        prior_from_labels(np.array([0, 3]), 3)
    with pytest.raises(ValueError, match="integer class indices"):
        prior_from_labels(np.array([0.5, 1.0]), 3)
    with pytest.raises(ValueError, match="pseudo_count"):
        prior_from_labels(np.array([0, 1, 2]), 3, pseudo_count=-1)


def test_arguments_are_checked_on_the_host():
    """Every check raises before a library call: these run without a device (a bad argument never reaches the handle)."""
    from mermaid_classifier_amd import estimate_cover
    from mermaid_classifier_amd.cover import check_cover_arguments, image_groups
    p = np.full((10, 4), 0.25, np.float32)
    off = [0, 4, 10]
    good = dict(train_prior=None, strength=1.0, iters=20, k=0)

    def bad(match, offsets=off, **kw):
        with pytest.raises(ValueError, match=match):
            estimate_cover(p, None, offsets, **{**good, **kw})

    bad("group_offsets", offsets=[1, 4, 10])
    bad("group_offsets", offsets=[0, 4, 9])
    bad("group_offsets", offsets=[0, 6, 4, 10])
    bad("group_offsets", offsets=[[0, 10]])
    bad("group_offsets", offsets=[0.0, 10.0])
    bad("train_prior must have shape", train_prior=[0.5, 0.5])
    bad("positive finite", train_prior=[0.5, 0.5, 0.0, 0.0])
    bad("positive finite", train_prior=[0.5, 0.5, np.nan, 0.0])
    bad("sums to", train_prior=[0.25, 0.25, 0.25, 0.2])
    bad("strength", strength=-0.5)
    bad("strength", strength=float("inf"))
    bad("strength", strength=float("nan"))
    bad("iters", iters=-1)
    bad("iters", iters=1001)
    bad("iters", iters=2.5)
    bad("k must be", k=-1)
    bad("k must be", k=1.5)
    bad("views_per_point", views_per_point=2)
    with pytest.raises(ValueError, match="second must be None"):
        estimate_cover(p, p, off)
    with pytest.raises(ValueError, match="proba must be"):
        estimate_cover(np.zeros(4, np.float32), None, [0, 4])
    with pytest.raises(TypeError, match="Predictor"):
        estimate_cover("model.pt", p, off)
    o, tp, s, it, k = check_cover_arguments(10, 4, off, [0.1, 0.2, 0.3, 0.4], 2, 7, 9)
    assert o.dtype == np.int64 and tp.dtype == np.float64 and (s, it, k) == (2.0, 7, 4)                # k is clamped to K
    with pytest.raises(ValueError, match="group_offsets"):
        check_cover_arguments(10, 4, [0], None, 1.0, 1, 0)
    with pytest.raises(ValueError, match="resident cells"):
        check_cover_arguments(1 << 29, 4, [0, 1 << 29], None, 1.0, 1, 0)
    # the groups of cover_images
    o, ids = image_groups([3, 0, 2, 5])
    assert o.tolist() == [0, 3, 3, 5, 10] and ids == [0, 1, 2, 3]
    o, ids = image_groups([3, 0, 2, 5], ["t1", "t1", "t2", "t2"])
    assert o.tolist() == [0, 3, 10] and ids == ["t1", "t2"]
    with pytest.raises(ValueError, match="comes back"):
        image_groups([1, 1, 1], ["a", "b", "a"])
    with pytest.raises(ValueError, match="entries for"):
        image_groups([1, 1, 1], ["a", "b"])


def test_from_fractions_matches_the_device_layout():
    """CoverStats.from_fractions fills the MMC_COVER_SUMS columns the grouped pass fills."""
    from mermaid_classifier_amd import CoverStats
    from mermaid_classifier_amd import _lib
    rng = np.random.default_rng(1)
    t, p = rng.dirichlet(np.ones(5), 12), rng.dirichlet(np.ones(5), 12)
    s = CoverStats.from_fractions(t, p)
    assert s.sums.shape == (5, _lib.MMC_COVER_SUMS) and s.n_images_used == 12
    d = p - t
    want = np.stack([t.sum(0), p.sum(0), d.sum(0), (d * d).sum(0), np.abs(d).sum(0), t.min(0), t.max(0), ((t - t.mean(0)) ** 2).sum(0)], 1)
    assert np.allclose(s.sums, want, rtol=1e-13, atol=0)
    assert CoverStats.from_fractions(np.zeros((0, 5)), np.zeros((0, 5))).table()["class"].size == 0
    with pytest.raises(ValueError, match="equal"):
        CoverStats.from_fractions(t, p[:, :4])
