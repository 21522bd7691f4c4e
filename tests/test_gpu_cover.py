"""-m gpu: cover estimation (include/mmc.h, "cover estimation") through the C ABI and the Python front-ends.

Counts and the 2^-32 fixed-point sums are compared as exact integers, against the same handle's mmc_head_predict rows; priors
against the float64 checker of tests/cover_checker.py within a derived atol (cover_checker.prior_atol: 64 * max(iters, 1) * n_max *
2^-53), each test also asserting that the checker's own float64-vs-long-double spread on its input is below atol / 64; the adapted
top-k on every row whose consecutive checker scores are more than 4 fp32 ulp apart; and the routes against each other bit for bit."""

import numpy as np
import pytest

import cover_checker as cc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

NAMES = ("count", "soft", "unusable", "prior", "idx", "scores")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return all(np.array_equal(bits(a[n]), bits(b[n])) for n in NAMES if a[n] is not None or b[n] is not None)


def _load(name):
    from mermaid_classifier_amd import load_predictor
    return load_predictor(GOLDEN / name / "model.pt", GOLDEN / name / "model.json")


def _ptr(a):
    return None if a is None else a.ctypes.data


def abi_cover(route, src, n, K, offsets, tp, strength, iters, k, G=1, fill=0, offsets_ptr=True, n_groups=None, tables=True,
              scores_ptr=True):
    """One cover call through the C ABI -> (status, outputs dict).  route: "proba" (src = host (n, K) float32), "proba_dev" (src = cuda
    tensor), "head" (src = (head, host feats)), "head_dev" (src = (head, cuda feats)), "set" (src = (head, FeatureSet)).  Outputs
    start at ``fill`` so that a rejected call's zeroing shows."""
    import torch
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    ng = (len(off) - 1 if off is not None else 0) if n_groups is None else n_groups
    rows = max(ng, 0)
    out = dict(count=np.full((rows, K), fill, np.int64), soft=np.full((rows, K), fill, np.int64), unusable=np.full(rows, fill, np.int64),
               prior=np.full((rows, K), float(fill), np.float64), idx=None, scores=None)
    if k:
        out["idx"], out["scores"] = np.full((max(n, 0), max(k, 0)), fill, np.int32), np.full((max(n, 0), max(k, 0)), float(fill), np.float32)
    tpa = None if tp is None else np.ascontiguousarray(tp, dtype=np.float64)
    common = (_ptr(off) if offsets_ptr else None, ng, _ptr(tpa), float(strength), int(iters),
              *((_ptr(out[t]) for t in NAMES[:4]) if tables else (None,) * 4), int(k), _ptr(out["idx"]), _ptr(out["scores"]) if scores_ptr else None)
    stream = int(torch.cuda.current_stream(0).cuda_stream)
    OUT, IN = _lib.MMC_OUT_HOST, _lib.MMC_IN_HOST
    if route == "proba":
        st = lib.mmc_cover_proba(_ptr(src), n, K, *common, 0, IN | OUT, stream)
    elif route == "proba_dev":
        st = lib.mmc_cover_proba(src.data_ptr(), n, K, *common, 0, OUT, stream)
    elif route == "head":
        head, X = src
        st = lib.mmc_head_cover(None if head is None else head._h, _ptr(X), n, G, *common, IN | OUT, stream)
    elif route == "head_dev":
        head, X = src
        st = lib.mmc_head_cover(head._h, X.data_ptr(), n, G, *common, OUT, stream)
    else:
        head, fs = src
        st = lib.mmc_head_cover_set(head._h, None if fs is None else fs._handle(), 0, n, G, *common, OUT, stream)
    return st, out


def ok_cover(*a, **kw):
    from mermaid_classifier_amd import _lib
    st, out = abi_cover(*a, **kw)
    _lib.check(st)
    return out


def check_against_rows(out, proba, offsets, tp, strength, iters, k):
    """The checks of cases 2 and 4: ``out`` against the checker run on the predict rows ``proba``."""
    K = proba.shape[1]
    sizes = np.diff(offsets)
    count, soft, unusable, prior = cc.cover(proba, offsets, tp, strength, iters)
    assert np.array_equal(out["unusable"], unusable)
    assert np.array_equal(out["count"], count)                                         # the argmax of the predict rows
    assert np.array_equal(out["soft"], soft)                                           # llrint of those rows, exact integers
    atol = cc.prior_atol(iters, sizes.max())
    _, _, _, wide = cc.cover(proba, offsets, tp, strength, iters, dtype=np.longdouble)
    spread = float(np.abs(prior - wide.astype(np.float64)).max())
    err = float(np.abs(out["prior"] - prior).max())
    print(f"K {K} iters {iters} strength {strength}: prior max|device - checker| {err:.3g}, atol {atol:.3g}, checker f64-vs-longdouble {spread:.3g}")
    assert spread < atol / 64
    assert err <= atol
    if k:
        want_i, want_s, allsc = cc.adapted_topk(proba, offsets, prior, tp, k)
        top = -np.sort(-allsc, axis=1)[:, :k + 1]                                      # (all finite here: usable rows only below)
        usable = cc.usable_rows(proba)
        decidable = usable & (cc.ulp_distance(top[:, :-1], top[:, 1:]).min(axis=1) > 4)
        left_out = int((usable & ~decidable).sum())
        print(f"  adapted top-{k}: {left_out} of {len(proba)} rows have checker scores within 4 ulp of each other")
        assert left_out <= 0.02 * len(proba)
        assert np.array_equal(out["idx"][decidable], want_i[decidable])
        assert cc.ulp_distance(out["scores"][usable], want_s[usable]).max() <= 2
        for r in np.flatnonzero(~usable):                                              # k distinct classes even for unusable rows
            assert len(set(out["idx"][r].tolist())) == k and 0 <= out["idx"][r].min() and out["idx"][r].max() < K


# ---- 1. the label-shift recipe on the device ----

def test_mixture_trials_as_eight_groups():
    v, y, off = cc.mixture_trials()
    out = ok_cover("proba", v, len(v), v.shape[1], off, None, 1.0, 50, 0)
    check_against_rows(out, v, off, None, 1.0, 50, 0)
    l1 = cc.label_shift_l1(out["count"], out["soft"], out["prior"], y, off)
    print("L1 hard / soft / adapted:\n", l1)
    assert (l1[:, 2] < 0.5 * np.minimum(l1[:, 0], l1[:, 1])).all()
    import torch
    dev = ok_cover("proba_dev", torch.from_numpy(v).cuda(), len(v), v.shape[1], off, None, 1.0, 50, 0)   # probabilities read in place
    assert same_bits(out, dev)


# ---- 2. head108: each side of the slab edge ----

SIZES_108 = [1, 2, 63, 64, 65, 61]


@pytest.fixture(scope="module")
def head108():
    head = _load("head108")._head
    X = np.load(GOLDEN / "head108_io.npz")["X"]
    proba, _ = head.predict(X)
    tp = np.random.default_rng(108).dirichlet(np.full(head.n_classes, 2.0))
    return head, X, proba, tp


@pytest.mark.parametrize("strength", [0.0, 1.0])
@pytest.mark.parametrize("iters", [0, 1, 8])
def test_head108_groups_around_the_slab_edge(head108, iters, strength):
    head, X, proba, tp = head108
    off = np.concatenate([[0], np.cumsum(SIZES_108)])
    assert off[-1] == len(X) == 256
    out = ok_cover("head", (head, X), 256, 108, off, tp, strength, iters, 4)
    check_against_rows(out, proba, off, tp, strength, iters, 4)
    if iters == 0:
        assert np.array_equal(out["prior"], np.tile(tp, (6, 1)))


def test_one_nan_feature_row_is_counted_and_enters_nothing_else(head108):
    """A one-layer head with head108's class count, groups and train prior: head108 itself has a hidden ReLU, which turns a NaN
    feature into 0 before it reaches the probabilities (as in test_gpu_validation's NaN test), so its rows cannot become unusable
    through the features."""
    from mermaid_classifier_amd.inference import DeviceHead, HeadParams
    rng = np.random.default_rng(1080)
    tp = head108[3]
    head = DeviceHead(HeadParams([rng.normal(0, 0.5, (108, 16)).astype(np.float32)], [rng.normal(0, 0.3, 108).astype(np.float32)],
                                 rng.uniform(-40, -10, 108).astype(np.float32), rng.uniform(1, 3, 108).astype(np.float32)))
    X = rng.normal(0, 1, (256, 16)).astype(np.float32)
    proba, _ = head.predict(X)
    off = np.concatenate([[0], np.cumsum(SIZES_108)])
    row, grp = 70, 3                                                                   # inside the 64-point group (rows 66 .. 129)
    bad = X.copy()
    bad[row] = np.nan
    iters, k = 8, 4
    out = ok_cover("head", (head, bad), 256, 108, off, tp, 1.0, iters, k)
    clean = ok_cover("head", (head, X), 256, 108, off, tp, 1.0, iters, k)
    assert out["unusable"].tolist() == [0, 0, 0, 1, 0, 0]
    others = np.arange(6) != grp
    for name in ("count", "soft", "prior"):                                            # the other groups: the bits of the clean call
        assert np.array_equal(bits(out[name][others]), bits(clean[name][others])), name
    # its own group's tables equal those of the call without that row
    keep = np.arange(256) != row
    off2 = off.copy()
    off2[grp + 1:] -= 1
    less = ok_cover("head", (head, np.ascontiguousarray(X[keep])), 255, 108, off2, tp, 1.0, iters, k)
    assert np.array_equal(out["count"], less["count"]) and np.array_equal(out["soft"], less["soft"])
    assert np.abs(out["prior"] - less["prior"]).max() <= cc.prior_atol(iters, 65)
    # neighbours: rows of other groups keep their bits; rows of its own group are those of the call without the row (the group's
    # sums are taken in another order there, so: within the checker's standard)
    in_grp = (np.arange(256) >= off[grp]) & (np.arange(256) < off[grp + 1])
    assert np.array_equal(out["idx"][~in_grp], clean["idx"][~in_grp]) and np.array_equal(bits(out["scores"][~in_grp]), bits(clean["scores"][~in_grp]))
    mine = in_grp & keep
    assert cc.ulp_distance(out["scores"][mine], less["scores"][in_grp[keep]]).max() <= 2
    pb, _ = head.predict(bad)
    assert not np.isfinite(pb[row]).any() and np.array_equal(bits(pb[keep]), bits(proba[keep]))
    check_against_rows(out, pb, off, tp, 1.0, iters, k)
    head.close()


# ---- 3. K = 5 < 64 lanes, padded input, a group across the chunk boundary ----

def test_a_group_across_the_chunk_boundary_and_three_routes():
    import torch
    from mermaid_classifier_amd import FeatureSet
    head = _load("head_fixture")._head
    io = np.load(GOLDEN / "head_fixture_io.npz")
    rng = np.random.default_rng(70001)
    n = 70001
    X = (io["X"][rng.integers(0, 512, n)] + rng.normal(0, 0.05, (n, 8))).astype(np.float32)
    sizes = [66000] + [25] * 160 + [1]
    off = np.concatenate([[0], np.cumsum(sizes)])
    assert off[-1] == n and 66000 > 65536
    tp = np.array([0.1, 0.3, 0.2, 0.25, 0.15])
    args = (n, 5, off, tp, 1.0, 3, 2)
    host = ok_cover("head", (head, X), *args)
    dev = ok_cover("head_dev", (head, torch.from_numpy(X).cuda()), *args)
    fs = FeatureSet(8, [0]).append(X, np.zeros(n, np.int64))
    st = ok_cover("set", (head, fs), *args)
    again = ok_cover("head", (head, X), *args)
    fs.close()
    assert same_bits(host, dev) and same_bits(host, st) and same_bits(host, again)
    proba, _ = head.predict(X)
    check_against_rows(host, proba, off, tp, 1.0, 3, 2)
    # the same stage on the predict rows themselves
    direct = ok_cover("proba", proba, *args)
    assert same_bits(host, direct)


# ---- 4. K = 257: five classes per lane, ragged ----

def test_a_head_with_257_classes():
    from mermaid_classifier_amd.inference import DeviceHead, HeadParams
    rng = np.random.default_rng(257)
    K, d = 257, 12
    head = DeviceHead(HeadParams([rng.normal(0, 0.5, (K, d)).astype(np.float32)], [rng.normal(0, 0.3, K).astype(np.float32)],
                                 rng.uniform(-40, -10, K).astype(np.float32), rng.uniform(1, 3, K).astype(np.float32)))
    X = rng.normal(0, 1, (256, d)).astype(np.float32)
    proba, _ = head.predict(X)
    tp = rng.dirichlet(np.full(K, 2.0))
    off = np.concatenate([[0], np.cumsum(SIZES_108)])
    for strength in (0.0, 1.0):
        out = ok_cover("head", (head, X), 256, K, off, tp, strength, 3, 4)
        check_against_rows(out, proba, off, tp, strength, 3, 4)
    head.close()


# ---- 5. two views per point ----

def test_two_views_per_point_is_the_stage_on_the_view_means(head108):
    head, X, _, tp = head108
    _, _, means = head.topk(X, 1, want_proba=True, views_per_point=2)
    off = np.array([0, 1, 3, 66, 128], np.int64)
    views = ok_cover("head", (head, X), 128, 108, off, tp, 1.0, 5, 3, G=2)
    direct = ok_cover("proba", means, 128, 108, off, tp, 1.0, 5, 3)
    assert same_bits(views, direct)
    check_against_rows(views, means, off, tp, 1.0, 5, 3)


# ---- 6. images -> cover ----

def test_cover_images_is_extract_images_then_estimate_cover(checkpoint_path):
    from mermaid_classifier_amd import PointClassifier, estimate_cover, grouped_validate
    from mermaid_classifier_amd.backbone import Backbone
    from mermaid_classifier_amd.pipeline import BatchedExtractor
    bb = Backbone(str(checkpoint_path), device=0, max_batch=16)
    pred = _load("head108")
    rng = np.random.default_rng(2024)
    images = [rng.integers(0, 256, (229, 241, 3), dtype=np.uint8), rng.integers(0, 256, (300, 260, 3), dtype=np.uint8),
              rng.integers(0, 256, (229, 241, 3), dtype=np.uint8)]
    rowcols = [[(0, 0), (228, 240), (114, 120), (3, 237), (200, 17)], [(0, 259), (150, 130), (299, 0)], [(10, 10), (100, 200)]]
    tp = rng.dirichlet(np.full(108, 2.0))
    pc = PointClassifier(bb, pred, batch_patches=4)                                    # the first image spans two passes
    feats = np.concatenate(BatchedExtractor(bb, batch_patches=4).extract_images(images, rowcols))
    for group_of_image, off, ids in ((None, [0, 5, 8, 10], [0, 1, 2]), (["t1", "t1", "t2"], [0, 8, 10], ["t1", "t2"])):
        got = pc.cover_images(images, rowcols, group_of_image, train_prior=tp, strength=1.0, iters=6, k=3)
        want = estimate_cover(pred, feats, off, tp, 1.0, 6, 3)
        assert got.groups == ids
        for name in ("counts", "soft_q32", "unusable", "n", "prior"):
            assert np.array_equal(bits(getattr(got, name)), bits(getattr(want, name))), name
        assert np.array_equal(got.topk.indices, want.topk.indices) and np.array_equal(got.topk.scores, want.topk.scores)
        assert got.topk.rowcols == [p for rc in rowcols for p in rc] and got.topk.labels == want.topk.labels
    # hard cover against the grouped validation's cover statistics
    got = pc.cover_images(images, rowcols, train_prior=tp)
    yi = rng.integers(0, 108, 10)
    yi[:4] = pred._head.predict(feats)[1][:4]
    sizes = [5, 3, 2]
    gv = grouped_validate(pred, (feats, np.asarray(pred.classes)[yi]), sizes)
    true_counts = np.stack([np.bincount(yi[a:b], minlength=108) for a, b in zip([0, 5, 8], [5, 8, 10])])
    mine = got.compare(true_counts, "hard")
    assert mine.n_images_used == gv.cover.n_images_used == 3
    assert np.allclose(mine.sums, gv.cover.sums, rtol=0, atol=1e-12)
    views = PointClassifier(bb, pred, batch_patches=5, views=(0, 5)).cover_images(images, rowcols, train_prior=tp, k=1)
    fv = np.concatenate(BatchedExtractor(bb, batch_patches=5).extract_images(images, rowcols, views=(0, 5)))
    wv = estimate_cover(pred, fv, [0, 5, 8, 10], tp, k=1, views_per_point=2)
    assert np.array_equal(bits(views.prior), bits(wv.prior)) and np.array_equal(views.counts, wv.counts)
    assert np.array_equal(views.topk.indices, wv.topk.indices)
    bb.close()


# ---- 7. every rejected argument ----

def test_rejected_arguments_return_err_arg_and_zero_the_outputs(head108):
    from mermaid_classifier_amd import FeatureSet, _lib
    head, X, proba, tp = head108
    n, K = 256, 108
    off = np.concatenate([[0], np.cumsum(SIZES_108)])
    nan_tp, neg_tp, off_tp = tp.copy(), tp.copy(), tp.copy()
    nan_tp[3], neg_tp[5], off_tp[0] = np.nan, 0.0, tp[0] + 1e-5
    small_set = FeatureSet(1280, [0]).append(X[:10], np.zeros(10, np.int64))
    narrow_set = FeatureSet(8, [0]).append(np.zeros((4, 8), np.float32), np.zeros(4, np.int64))
    cases = {
        "offsets do not start at 0": dict(offsets=off + np.r_[1, np.zeros(6, np.int64)]),
        "offsets decrease": dict(offsets=np.array([0, 10, 5, 66, 130, 195, 256])),
        "offsets do not end at n": dict(offsets=np.r_[off[:-1], 255]),
        "offsets NULL": dict(offsets_ptr=False),
        "negative n_groups": dict(n_groups=-1),
        "a NaN prior entry": dict(tp=nan_tp),
        "a zero prior entry": dict(tp=neg_tp),
        "a prior that does not sum to 1": dict(tp=off_tp),
        "negative strength": dict(strength=-1.0),
        "infinite strength": dict(strength=float("inf")),
        "NaN strength": dict(strength=float("nan")),
        "negative iters": dict(iters=-1),
        "too many iters": dict(iters=_lib.MMC_COVER_MAX_ITERS + 1),
        "k above K": dict(k=K + 1),
    }
    base = dict(offsets=off, tp=tp, strength=1.0, iters=2, k=4)
    for what, change in cases.items():
        for route, src in (("proba", proba), ("head", (head, X))):
            a = {**base, **change}
            st, out = abi_cover(route, src, n, K, a.pop("offsets"), a.pop("tp"), a.pop("strength"), a.pop("iters"), a.pop("k"), fill=7, **a)
            assert st == _lib.MMC_ERR_ARG, (what, route)
            assert _lib.lib().mmc_last_error()
            for name in NAMES:
                if out[name] is not None and out[name].size and not (name in ("idx", "scores") and what == "k above K"):
                    assert not out[name].any(), (what, route, name)
    # arguments of one route only
    big = _lib.MMC_COVER_MAX_CELLS // K + 1
    only = [
        ("negative n", "proba", proba, dict(n=-1, k=0)),
        ("n * K above the cap", "proba", proba, dict(n=big, offsets=np.array([0, big]), k=0)),      # (rejected before anything is read)
        ("K = 0", "proba", proba, dict(K=0, k=0)),
        ("NULL head", "head", (None, X), {}),
        ("G = 0", "head", (head, X), dict(G=0)),
        ("G = 17", "head", (head, X), dict(G=17)),
        ("NULL set", "set", (head, None), {}),
        ("a set shorter than the call", "set", (head, small_set), {}),
        ("a set of another width", "set", (head, narrow_set), dict(n=4, offsets=np.array([0, 4]))),
        ("NULL tables", "proba", proba, dict(tables=False)),
        ("idx without scores", "proba", proba, dict(scores_ptr=False)),
    ]
    for what, route, src, change in only:
        a = {**base, "n": n, "K": K, **change}
        st, out = abi_cover(route, src, a.pop("n"), a.pop("K"), a.pop("offsets"), a.pop("tp"), a.pop("strength"), a.pop("iters"), a.pop("k"),
                            fill=7, **a)
        assert st == _lib.MMC_ERR_ARG, what
        if what not in ("NULL head", "NULL tables"):                                   # (no K to size the tables by / no tables)
            for name in NAMES[:4]:
                assert not out[name].any(), (what, name)
    small_set.close()
    narrow_set.close()
    # and a good call still works afterwards; n = 0 is MMC_OK with train_prior in every row
    check_against_rows(ok_cover("head", (head, X), n, K, off, tp, 1.0, 2, 4), proba, off, tp, 1.0, 2, 4)
    st, out = abi_cover("proba", proba, 0, K, np.array([0, 0, 0]), tp, 1.0, 2, 0, fill=7)
    assert st == _lib.MMC_OK and not out["count"].any() and not out["soft"].any() and np.array_equal(out["prior"], np.tile(tp, (2, 1)))
