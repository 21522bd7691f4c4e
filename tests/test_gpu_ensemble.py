"""-m gpu: head ensembles (include/mmc.h, "head ensembles") through the C ABI and the Python front-ends.

Bit for bit wherever the definition is in float32: the means against tests/ensemble_checker.py fed with each member's own
mmc_head_predict rows, idx / scores against a stable host sort of those means, votes against first maxima; M = 1 against the
single-head calls.  The three entropy stats are compared with float64 references under the checker's derived bound, and every
measured error-to-bound ratio is printed."""

import json

import numpy as np
import pytest

import ensemble_checker as ec
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _load(name):
    from mermaid_classifier_amd import load_predictor
    return load_predictor(GOLDEN / name / "model.pt", GOLDEN / name / "model.json")


def make_member(rng, dims, scale=0.5, classes=None):
    """A random-weight CalibratedMLP: Linear widths ``dims`` (input, hidden ..., K), Platt a in [-3, -0.5], b in [-1, 1]."""
    from mermaid_classifier_amd import CalibratedMLP
    K = dims[-1]
    W = [rng.normal(0, scale, (dims[i + 1], dims[i])).astype(np.float32) for i in range(len(dims) - 1)]
    b = [rng.normal(0, 0.2, dims[i + 1]).astype(np.float32) for i in range(len(dims) - 1)]
    return CalibratedMLP(W, b, [f"c{i}" for i in range(K)] if classes is None else classes, rng.uniform(-3, -0.5, K), rng.uniform(-1, 1, K))


HIDDEN = [(), (24,), (10, 6)]


def make_members(seed, M, dim, K, scale=0.5):
    rng = np.random.default_rng(seed)
    return [make_member(rng, (dim,) + HIDDEN[j % 3] + (K,), scale) for j in range(M)]


class CEnsemble:
    """mmc_ensemble_create over DeviceHead handles (kept alive here)."""

    def __init__(self, heads):
        import ctypes as C
        from mermaid_classifier_amd import _lib
        self.heads = list(heads)
        arr = (C.c_void_p * len(self.heads))(*[h._h.value for h in self.heads])
        self.h = C.c_void_p()
        _lib.check(_lib.lib().mmc_ensemble_create(arr, len(self.heads), C.byref(self.h)))
        self.K = self.heads[0].n_classes

    def close(self):
        from mermaid_classifier_amd import _lib
        if self.h.value:
            _lib.lib().mmc_ensemble_destroy(self.h)
            self.h.value = None

    def topk(self, X, n_points, G, k, device=False, proba=True, stats=True):
        """-> dict idx, scores, proba, stats, votes (host arrays), from host arguments or from device tensors."""
        import torch
        from mermaid_classifier_amd import _lib
        X = np.ascontiguousarray(X, np.float32)
        shapes = dict(idx=((n_points, k), np.int32), scores=((n_points, k), np.float32))
        if proba:
            shapes["proba"] = ((n_points, self.K), np.float32)
        if stats:
            shapes.update(stats=((n_points, 3), np.float32), votes=((n_points,), np.int32))
        if device:
            xd = torch.from_numpy(X).cuda()
            out = {k_: torch.full(sh, -7, dtype=getattr(torch, np.dtype(dt).name), device="cuda") for k_, (sh, dt) in shapes.items()}
            p = {k_: v.data_ptr() for k_, v in out.items()}
            src, flags = xd.data_ptr(), 0
        else:
            out = {k_: np.full(sh, -7, dt) for k_, (sh, dt) in shapes.items()}
            p = {k_: v.ctypes.data for k_, v in out.items()}
            src, flags = X.ctypes.data, _lib.MMC_IN_HOST | _lib.MMC_OUT_HOST
        _lib.check(_lib.lib().mmc_ensemble_topk(self.h, src, n_points, G, k, p["idx"], p["scores"], p.get("proba"), p.get("stats"),
                                                p.get("votes"), flags, None))
        if device:
            torch.cuda.synchronize()
            out = {k_: v.cpu().numpy() for k_, v in out.items()}
        return out

    def evaluate(self, X, y, lmap=None, device=False, fs=None, first=0):
        """mmc_ensemble_evaluate on host or device rows, or (``fs``) mmc_ensemble_evaluate_set on rows [first, first + len(y))."""
        import torch
        from mermaid_classifier_amd import _lib
        n, K = len(y), self.K
        o = dict(est=np.full(n, -7, np.int32), score=np.full(n, -7, np.float32), rank=np.full(n, -7, np.int32),
                 p_true=np.full(n, -7, np.float32), stats=np.full((n, 3), -7, np.float32), votes=np.full(n, -7, np.int32),
                 totals=np.full(5, -7, np.int64), confusion=np.full((K, K), -7, np.int64), rank_hist=np.full(K, -7, np.int64))
        outs = [o[k_].ctypes.data for k_ in ("est", "score", "rank", "p_true", "stats", "votes", "totals", "confusion", "rank_hist")]
        margs = (_ptr(lmap), 0 if lmap is None else len(lmap))
        if fs is not None:
            _lib.check(_lib.lib().mmc_ensemble_evaluate_set(self.h, fs._handle(), first, n, *margs, *outs, None))
            return o
        X = np.ascontiguousarray(X, np.float32)
        y = np.ascontiguousarray(y, np.int32)
        if device:
            xd = torch.from_numpy(X).cuda()
            src, flags = xd.data_ptr(), 0
        else:
            src, flags = X.ctypes.data, _lib.MMC_IN_HOST
        _lib.check(_lib.lib().mmc_ensemble_evaluate(self.h, src, y.ctypes.data, n, *margs, *outs, flags, None))
        return o


def c_ensemble(members):
    return CEnsemble([m._device_head() if hasattr(m, "_device_head") else m._head for m in members])


def member_rows(members, X):
    """Each member's own mmc_head_predict rows: (M, rows, K) float32."""
    return np.stack([(m._device_head() if hasattr(m, "_device_head") else m._head).predict(np.ascontiguousarray(X, np.float32),
                                                                                         want_argmax=False)[0] for m in members])


RATIOS = []


def check_definition(got, want, K, M, what, rows=None):
    """idx / scores / proba bits, votes, and the stats inside the checker's bound (ratios printed and recorded)."""
    sel = slice(None) if rows is None else rows
    assert np.array_equal(bits(got["proba"][sel]), bits(want["e"][sel])), what
    assert np.array_equal(got["idx"][sel], want["idx"][sel]), what
    assert np.array_equal(bits(got["scores"][sel]), bits(want["scores"][sel])), what
    assert np.array_equal(got["votes"][sel], want["votes"][sel]), what
    bound = ec.stats_bound(want["stats"][sel], K, M)
    err = np.abs(got["stats"][sel].astype(np.float64) - want["stats"][sel])
    ratio = float((err / bound).max())
    RATIOS.append(ratio)
    print(f"ensemble stats {what}: max error/bound = {ratio:.3f} (max abs error {err.max():.3e})")
    assert np.all(err <= bound), what


# ---- 1. M = 1, G = 1 is the single head, bit for bit ----

def _single_cases():
    io = np.load(GOLDEN / "head108_io.npz")
    rng = np.random.default_rng(11)
    small = make_member(rng, (10, 7))
    return [("head108", _load("head108"), io["X"][:101]), ("10->7", small, rng.normal(0, 1, (37, 10)).astype(np.float32))]


@pytest.mark.parametrize("case", [0, 1])
def test_one_member_one_view_is_mmc_head_topk_and_mmc_head_evaluate(case):
    from mermaid_classifier_amd import _lib
    name, model, X = _single_cases()[case]
    head = model._device_head() if hasattr(model, "_device_head") else model._head
    K, n, k = head.n_classes, len(X), 3
    ens = CEnsemble([head])
    assert _lib.lib().mmc_ensemble_size(ens.h) == 1 and _lib.lib().mmc_ensemble_num_classes(ens.h) == K
    assert _lib.lib().mmc_ensemble_input_dim(ens.h) == head.input_dim
    wi, ws, wp = head.topk(X, k, want_proba=True)
    got = ens.topk(X, n, 1, k)
    assert np.array_equal(got["idx"], wi) and np.array_equal(bits(got["scores"]), bits(ws)) and np.array_equal(bits(got["proba"]), bits(wp))
    assert np.array_equal(got["votes"], np.ones(n, np.int32))
    assert np.array_equal(bits(got["stats"][:, 0]), bits(got["stats"][:, 1])) and np.all(got["stats"][:, 2] == 0)
    # evaluate: every per-row output and every table, nll included
    y = np.random.default_rng(5).integers(0, K, n).astype(np.int32)
    w = dict(est=np.empty(n, np.int32), score=np.empty(n, np.float32), rank=np.empty(n, np.int32), p_true=np.empty(n, np.float32),
             totals=np.empty(5, np.int64), confusion=np.empty((K, K), np.int64), rank_hist=np.empty(K, np.int64))
    _lib.check(_lib.lib().mmc_head_evaluate(head._h, X.ctypes.data, y.ctypes.data, n, None, 0, *[w[q].ctypes.data for q in w],
                                            _lib.MMC_IN_HOST, None))
    e = ens.evaluate(X, y)
    for q in ("est", "rank", "totals", "confusion", "rank_hist"):
        assert np.array_equal(e[q], w[q]), (name, q)
    for q in ("score", "p_true"):
        assert np.array_equal(bits(e[q]), bits(w[q])), (name, q)
    assert np.array_equal(bits(e["stats"]), bits(got["stats"])) and np.array_equal(e["votes"], got["votes"])
    ens.close()


# ---- 2. M = 1, G = 3 is mmc_head_topk_views ----

def test_one_member_three_views_is_mmc_head_topk_views():
    name, model, X = _single_cases()[0]
    head = model._head
    X = X[:99]
    wi, ws, wp = head.topk(X, 4, want_proba=True, views_per_point=3)
    ens = CEnsemble([head])
    got = ens.topk(X, 33, 3, 4)
    assert np.array_equal(got["idx"], wi) and np.array_equal(bits(got["scores"]), bits(ws)) and np.array_equal(bits(got["proba"]), bits(wp))
    ens.close()


# ---- 3. the definition ----

@pytest.mark.parametrize("dim", [10, 1280])              # 10: the padded input path and the GEMM's K tail; 1280: the backbone's width
@pytest.mark.parametrize("n_points", [1, 5, 9])
@pytest.mark.parametrize("K", [3, 7, 64, 65, 130])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("M", [2, 3, 16])
def test_definition_against_the_members_own_rows(M, G, K, n_points, dim):
    members = make_members(1000 + 37 * M + 5 * G + K, M, dim, K, scale=0.5 if dim == 10 else 0.05)
    X = np.random.default_rng(K).normal(0, 1, (n_points * G, dim)).astype(np.float32)
    k = min(K, 5)
    want = ec.definition(member_rows(members, X), G, k)
    ens = c_ensemble(members)
    for device in (False, True):
        got = ens.topk(X, n_points, G, k, device=device)
        check_definition(got, want, K, M, f"M={M} G={G} K={K} P={n_points} dim={dim} device={device}")
    # without the optional outputs the required ones keep their bits
    bare = ens.topk(X, n_points, G, k, proba=False, stats=False)
    assert np.array_equal(bare["idx"], want["idx"]) and np.array_equal(bits(bare["scores"]), bits(want["scores"]))
    ens.close()


def test_widest_class_list_fills_the_lds_rows():
    """K = 2048, the create-time limit: the two rows per wave are the whole 64 KB of a workgroup's dynamic LDS, and evaluate keeps
    its rank histogram in memory instead (the other path of the launcher)."""
    K, M, n = 2048, 2, 6
    members = make_members(77, M, 10, K)
    X = np.random.default_rng(3).normal(0, 1, (n, 10)).astype(np.float32)
    want = ec.definition(member_rows(members, X), 1, 4)
    ens = c_ensemble(members)
    check_definition(ens.topk(X, n, 1, 4), want, K, M, "K=2048")
    y = np.arange(n, dtype=np.int32) * 300
    e = ens.evaluate(X, y)
    assert np.array_equal(e["est"], want["idx"][:, 0]) and np.array_equal(bits(e["p_true"]), bits(want["e"][np.arange(n), y]))
    ranks = 1 + (np.argsort(-want["e"].astype(np.float64), axis=1, kind="stable") == y[:, None]).argmax(1)
    assert np.array_equal(e["rank"], ranks) and np.array_equal(e["rank_hist"], np.bincount(ranks - 1, minlength=K))
    assert e["totals"][:4].tolist() == [n, int((e["est"] == y).sum()), 0, 0]
    ens.close()


# ---- 4. ties and NaN ----

def test_uniform_rows_rank_in_class_order_and_every_member_votes():
    from mermaid_classifier_amd import CalibratedMLP
    K, M = 9, 3
    rng = np.random.default_rng(2)
    members = [CalibratedMLP([np.zeros((K, 10), np.float32)], [np.zeros(K, np.float32)], list(range(K)), np.full(K, -1.0 - j), np.full(K, 0.25 * j))
               for j in range(M)]
    X = rng.normal(0, 1, (5, 10)).astype(np.float32)
    ens = c_ensemble(members)
    got = ens.topk(X, 5, 1, 4)
    assert np.array_equal(got["idx"], np.tile(np.arange(4, dtype=np.int32), (5, 1)))
    assert np.array_equal(got["votes"], np.full(5, M, np.int32))
    assert np.allclose(got["proba"], 1.0 / K, rtol=1e-6) and np.allclose(got["stats"][:, 0], np.log(K), rtol=1e-6)
    ens.close()


def test_a_nan_row_gets_distinct_classes_and_enters_no_table():
    K, M, n = 7, 3, 6
    members = make_members(9, M, 10, K)
    X = np.random.default_rng(4).normal(0, 1, (n, 10)).astype(np.float32)
    X[2, 3] = np.nan
    y = (np.arange(n) % K).astype(np.int32)
    ens = c_ensemble(members)
    got = ens.topk(X, n, 1, K)
    assert sorted(got["idx"][2].tolist()) == list(range(K))
    clean = np.delete(np.arange(n), 2)
    want = ec.definition(member_rows(members, X[clean]), 1, K)
    check_definition({q: v[clean] for q, v in got.items()}, want, K, M, "rows beside a NaN row")
    e = ens.evaluate(X, y)
    ec_clean = ens.evaluate(X[clean], y[clean])
    assert e["totals"][3] == 1 and e["totals"][0] == n and e["totals"][2] == 0
    assert e["totals"][1] == ec_clean["totals"][1] and e["totals"][4] == ec_clean["totals"][4]
    assert np.array_equal(e["confusion"], ec_clean["confusion"]) and np.array_equal(e["rank_hist"], ec_clean["rank_hist"])
    assert e["confusion"].sum() == n - 1
    ens.close()


# ---- 5. chunk boundary ----

def test_a_call_across_the_chunk_boundary_equals_two_halves_and_the_definition():
    from mermaid_classifier_amd import _lib
    M, G, K, dim = 2, 3, 5, 8
    rng = np.random.default_rng(21)
    members = [make_member(rng, (dim, 16, K)), make_member(rng, (dim, K))]
    ens = c_ensemble(members)
    rows = _lib.lib().mmc_ensemble_chunk_rows(ens.h, G)
    assert rows % G == 0 and rows == 65536 // M // G * G
    per = rows // G
    n_points = per + 3
    X = rng.normal(0, 1, (n_points * G, dim)).astype(np.float32)
    whole = ens.topk(X, n_points, G, 2)
    cut = per // 2 + 1
    a, b = ens.topk(X[: cut * G], cut, G, 2), ens.topk(X[cut * G:], n_points - cut, G, 2)
    for q in whole:
        both = np.concatenate([a[q], b[q]])
        same = np.array_equal(bits(both), bits(whole[q])) if both.dtype == np.float32 else np.array_equal(both, whole[q])
        assert same, q
    around = np.arange(per - 4, n_points)
    want = ec.definition(member_rows(members, X[around[0] * G:]), G, 2)
    check_definition({q: v[around] for q, v in whole.items()}, want, K, M, "rows around the chunk boundary")
    ens.close()


# ---- 6. host, device and feature-set arguments ----

def test_host_device_and_set_arguments_give_the_same_bits():
    from mermaid_classifier_amd import FeatureSet
    M, K, dim, n = 3, 7, 10, 40
    members = make_members(31, M, dim, K)
    rng = np.random.default_rng(8)
    X = rng.normal(0, 1, (n, dim)).astype(np.float32)
    ens = c_ensemble(members)
    # a data class list of K + 1 names: data class j < K is model class (j + 1) % K, data class K is one the ensemble lacks
    lmap = np.append((np.arange(K, dtype=np.int32) + 1) % K, np.int32(-1))
    y = rng.integers(0, K + 1, n).astype(np.int32)
    y[:3] = K
    host = ens.evaluate(X, y, lmap)
    dev = ens.evaluate(X, y, lmap, device=True)
    fs = FeatureSet(dim, list(range(K + 1))).append(X, y)
    st = ens.evaluate(None, y, lmap, fs=fs)
    part = ens.evaluate(None, y[5:], lmap, fs=fs, first=5)
    for other in (dev, st):
        for q in host:
            same = np.array_equal(bits(host[q]), bits(other[q])) if host[q].dtype == np.float32 else np.array_equal(host[q], other[q])
            assert same, q
    assert np.array_equal(part["est"], host["est"][5:]) and np.array_equal(bits(part["stats"]), bits(host["stats"][5:]))
    unknown = y == K
    assert host["totals"][2] == unknown.sum() and np.all(host["rank"][unknown] == 0) and np.all(host["rank"][~unknown] >= 1)
    want = ec.definition(member_rows(members, X), 1, 1)
    assert np.array_equal(host["est"], want["idx"][:, 0]) and np.array_equal(host["votes"], want["votes"])
    g = lmap[y]
    assert np.array_equal(bits(host["p_true"][~unknown]), bits(want["e"][np.arange(n)[~unknown], g[~unknown]]))
    assert host["totals"][1] == int((host["est"] == g)[~unknown].sum())
    fs.close()
    ens.close()


# ---- 7. patches -> ensemble ----

@pytest.fixture(scope="module")
def backbone(checkpoint_path):
    from mermaid_classifier_amd.backbone import Backbone
    bb = Backbone(str(checkpoint_path), device=0, max_batch=16)
    yield bb
    bb.close()


@pytest.fixture(scope="module")
def wide_members():
    return make_members(55, 3, 1280, 12, scale=0.05)


def test_classify_patches_is_extract_plus_ensemble_topk(backbone, wide_members):
    from mermaid_classifier_amd import _lib
    patches = np.random.default_rng(6).integers(0, 256, (6, 224, 224, 3), dtype=np.uint8)
    ens = c_ensemble(wide_members)
    feats = backbone.extract(patches)
    want = ens.topk(np.asarray(feats), 3, 2, 4, proba=False)
    idx, sc = np.full((3, 4), -7, np.int32), np.full((3, 4), -7, np.float32)
    stats, votes = np.full((3, 3), -7, np.float32), np.full(3, -7, np.int32)
    _lib.check(_lib.lib().mmc_ensemble_classify_patches(backbone._h, ens.h, patches.ctypes.data, 3, 2, 4, idx.ctypes.data, sc.ctypes.data,
                                                        stats.ctypes.data, votes.ctypes.data, _lib.MMC_IN_HOST | _lib.MMC_OUT_HOST, None))
    assert np.array_equal(idx, want["idx"]) and np.array_equal(bits(sc), bits(want["scores"]))
    assert np.array_equal(bits(stats), bits(want["stats"])) and np.array_equal(votes, want["votes"])
    ens.close()


# ---- 8. Python ----

def test_head_ensemble_topk_and_uncertainty():
    import torch
    from mermaid_classifier_amd import HeadEnsemble
    M, K, dim, G, n_points = 3, 7, 10, 3, 5
    members = make_members(61, M, dim, K)
    X = np.random.default_rng(9).normal(0, 1, (n_points * G, dim)).astype(np.float32)
    want = ec.definition(member_rows(members, X), G, 3)
    ens = HeadEnsemble(members)
    idx, sc, proba = ens.topk(X, 3, views_per_point=G, want_proba=True)
    assert np.array_equal(idx, want["idx"]) and np.array_equal(bits(sc), bits(want["scores"])) and np.array_equal(bits(proba), bits(want["e"]))
    u = ens.uncertainty(X, views_per_point=G)
    assert np.array_equal(u.votes, want["votes"])
    bound = ec.stats_bound(want["stats"], K, M)
    assert np.all(np.abs(u.entropy - want["stats"][:, 0]) <= bound[:, 0])
    assert np.all(np.abs(u.expected_entropy - want["stats"][:, 1]) <= bound[:, 1])
    # clamping at 0 moves a value no further from the (clamped) reference than it was from the unclamped one
    assert np.all(u.mutual_information >= 0)
    assert np.all(np.abs(u.mutual_information - np.maximum(want["stats"][:, 2], 0)) <= bound[:, 2])
    di, ds = ens.topk(torch.from_numpy(X).cuda(), 3, views_per_point=G)
    assert np.array_equal(di.cpu().numpy(), idx) and np.array_equal(bits(ds.cpu().numpy()), bits(sc))
    one = ec.definition(member_rows(members, X), 1, 1)
    assert np.array_equal(ens.predict_proba(X), one["e"].astype(np.float64))
    assert ens.predict(X) == [f"c{i}" for i in one["idx"][:, 0]]
    ens.close()


def test_point_classifier_with_an_ensemble_fills_the_new_fields(backbone, wide_members):
    from mermaid_classifier_amd import HeadEnsemble, PointClassifier
    from mermaid_classifier_amd.pipeline import BatchedExtractor
    image = np.random.default_rng(12).integers(0, 256, (300, 310, 3), dtype=np.uint8)
    rowcols = [(120, 130), (150, 160), (170, 140), (130, 170), (160, 150)]
    ens = HeadEnsemble(wide_members)
    pc = PointClassifier(backbone, ens, batch_patches=4)
    pred = pc.classify_image(image, rowcols, k=3)
    feats = BatchedExtractor(backbone, batch_patches=4).extract_images([image], [rowcols])[0]
    idx, sc = ens.topk(np.asarray(feats, np.float32), 3)
    u = ens.uncertainty(np.asarray(feats, np.float32))
    assert np.array_equal(pred.indices, idx) and np.array_equal(pred.scores, sc.astype(np.float64))
    assert np.array_equal(bits(pred.entropy), bits(u.entropy)) and np.array_equal(bits(pred.mutual_information), bits(u.mutual_information))
    assert np.array_equal(pred.votes, u.votes) and pred.votes.min() >= 0 and pred.votes.max() <= 3
    single = PointClassifier(backbone, wide_members[0].predictor(), batch_patches=4).classify_image(image, rowcols, k=3)
    assert single.entropy is None and single.mutual_information is None and single.votes is None
    ens.close()


def _labelled(seed, n, dim, K):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 2.0, (K, dim))
    y = rng.integers(0, K, n)
    return (centres[y] + rng.normal(0, 1.0, (n, dim))).astype(np.float32), y


def test_ensemble_validate_table_and_risk_coverage():
    from mermaid_classifier_amd import HeadEnsemble, ensemble_validate, validate
    M, K, dim, n = 3, 7, 10, 120
    members = make_members(71, M, dim, K)
    X, y = _labelled(1, n, dim, K)
    labels = np.array([f"c{i}" for i in y])
    ens = HeadEnsemble(members)
    ev = ensemble_validate(ens, (X, labels))
    table = ev.table()
    assert [r["member"] for r in table] == [0, 1, 2, "ensemble"]
    for j, m in enumerate(members):
        v = validate(m, (X, labels), rows=False)
        cs = v.class_scores()
        assert table[j] == {"member": j, "accuracy": v.accuracy, "balanced_accuracy": cs.balanced_accuracy, "f1_macro": cs.f1_macro,
                            "log_loss": v.log_loss}
    want = ec.definition(member_rows(members, X), 1, 1)
    v = ev.validation
    assert np.array_equal(v.est, want["idx"][:, 0]) and np.array_equal(v.gt, y.astype(np.int32)) and v.n == n
    assert np.array_equal(bits(v.p_true), bits(want["e"][np.arange(n), y]))
    assert np.array_equal(ev.uncertainty.votes, want["votes"])
    assert v.class_scores().balanced_accuracy == table[3]["balanced_accuracy"] and len(v.val_results().gt) == n
    # Jensen, per row and in the mean: the ensemble's log-loss is at most the members' mean log-loss (float32 rounding of e allowed for)
    assert v.log_loss <= np.mean([t["log_loss"] for t in table[:3]]) + (M + 1) * 2.0 ** -23
    for by, key in (("entropy", ev.uncertainty.entropy), ("votes", -ev.uncertainty.votes.astype(np.float64)), ("score", -v.scores)):
        rc = ev.risk_coverage(by=by, levels=[0.25, 0.5, 1.0])
        assert np.allclose(rc["accuracy"], ec.risk_coverage(v.est == v.gt, key, [0.25, 0.5, 1.0]), rtol=0, atol=1e-15), by
        assert rc["accuracy"][-1] == v.accuracy
    totals_only = ensemble_validate(ens, (X, labels), rows=False)
    assert totals_only.uncertainty is None and np.array_equal(totals_only.validation.confusion, v.confusion)
    ens.close()


def test_export_then_load_gives_the_same_bits(tmp_path):
    from mermaid_classifier_amd import HeadEnsemble, export_ensemble, load_ensemble
    members = make_members(81, 3, 10, 7)
    X = np.random.default_rng(13).normal(0, 1, (20, 10)).astype(np.float32)
    ens = HeadEnsemble(members)
    manifest = export_ensemble(ens, tmp_path / "ens", X)
    assert manifest["members"] == ["member_00", "member_01", "member_02"] and manifest["input_dim"] == 10
    assert json.loads((tmp_path / "ens" / "ensemble.json").read_text()) == manifest
    back = load_ensemble(tmp_path / "ens")
    a, b = ens.topk(X, 3, want_proba=True), back.topk(X, 3, want_proba=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[2]), bits(b[2]))
    ua, ub = ens.uncertainty(X), back.uncertainty(X)
    assert np.array_equal(bits(ua.entropy), bits(ub.entropy)) and np.array_equal(ua.votes, ub.votes)
    assert back.classes == ens.classes
    ens.close()
    back.close()


def test_from_sweep_keeps_the_best_configurations():
    from mermaid_classifier_amd import FeatureSet, HeadEnsemble, SweepConfig, train_sweep
    K, dim = 4, 12
    X, y = _labelled(3, 300, dim, K)
    classes = list(range(K))
    train = FeatureSet(dim, classes).append(X[:200], y[:200])
    ref = FeatureSet(dim, classes).append(X[200:250], y[200:250])
    val = FeatureSet(dim, classes).append(X[250:], y[250:])
    configs = [SweepConfig(hidden_layer_sizes=(16,), learning_rate_init=1e-2), SweepConfig(hidden_layer_sizes=(8,), learning_rate_init=1e-3),
               SweepConfig(hidden_layer_sizes=(16, 8), learning_rate_init=3e-3)]
    results = train_sweep(train, ref, val, configs, 2, batch_size=50)
    ens = HeadEnsemble.from_sweep(results, val, top=2)
    assert len(ens) == 2 and len(ens.ranking) == 3
    assert [r["config"] for r in ens.ranking[:2]] == [results.index(next(r for r in results if r[0] is m)) for m in ens.members]
    idx, _ = ens.topk(X[250:], 1)
    assert idx.shape == (50, 1) and idx.min() >= 0 and idx.max() < K
    for fs in (train, ref, val):
        fs.close()
    ens.close()


def test_estimate_cover_takes_the_ensembles_probabilities():
    from mermaid_classifier_amd import HeadEnsemble, estimate_cover
    members = make_members(91, 3, 10, 7)
    X = np.random.default_rng(14).normal(0, 1, (30, 10)).astype(np.float32)
    ens = HeadEnsemble(members)
    proba = ens.predict_proba(X)
    est = estimate_cover(proba, None, [0, 12, 30], iters=0)
    arg = proba.argmax(1)
    want = np.stack([np.bincount(arg[:12], minlength=7), np.bincount(arg[12:], minlength=7)])
    assert np.array_equal(est.counts, want)
    ens.close()


# ---- 9. argument errors ----

def test_every_argument_error_is_reported_before_anything_is_written():
    import ctypes as C
    from mermaid_classifier_amd import _lib
    from mermaid_classifier_amd import CalibratedMLP
    lib = _lib.lib()
    rng = np.random.default_rng(17)
    base = make_member(rng, (10, 7))
    heads = [base._device_head()]
    ARG = _lib.MMC_ERR_ARG

    def create(ptrs, count):
        arr = (C.c_void_p * max(1, len(ptrs)))(*ptrs)
        h = C.c_void_p(12345)
        r = lib.mmc_ensemble_create(arr, count, C.byref(h))
        return r, h
    h0 = heads[0]._h.value
    for ptrs, count in (([h0], 0), ([h0] * 17, 17), ([h0, None], 2)):
        r, h = create(ptrs, count)
        assert r == ARG and not h.value and lib.mmc_last_error()
    assert lib.mmc_ensemble_create(None, 1, C.byref(C.c_void_p())) == ARG
    other_k, other_dim = make_member(rng, (10, 8))._device_head(), make_member(rng, (12, 7))._device_head()
    for other in (other_k, other_dim):
        r, h = create([h0, other._h.value], 2)
        assert r == ARG and not h.value
    wide = CalibratedMLP([np.zeros((2049, 4), np.float32)], [np.zeros(2049, np.float32)], list(range(2049)), -np.ones(2049), np.zeros(2049))
    r, h = create([wide._device_head()._h.value], 1)
    assert r == ARG and not h.value and b"2048" in lib.mmc_last_error()
    ens = CEnsemble(heads)
    assert lib.mmc_ensemble_chunk_rows(ens.h, 0) == 0 and lib.mmc_ensemble_chunk_rows(ens.h, 17) == 0 and lib.mmc_ensemble_chunk_rows(None, 1) == 0
    X = rng.normal(0, 1, (6, 10)).astype(np.float32)
    idx, sc = np.full((6, 8), -7, np.int32), np.full((6, 8), -7, np.float32)
    proba, stats, votes = np.full((6, 7), -7, np.float32), np.full((6, 3), -7, np.float32), np.full(6, -7, np.int32)
    flags = _lib.MMC_IN_HOST | _lib.MMC_OUT_HOST

    def topk(e=ens.h, x=X.ctypes.data, n=6, G=1, k=2, i=idx.ctypes.data, s=sc.ctypes.data):
        return lib.mmc_ensemble_topk(e, x, n, G, k, i, s, proba.ctypes.data, stats.ctypes.data, votes.ctypes.data, flags, None)
    for bad in (dict(e=None), dict(G=0), dict(G=17), dict(k=0), dict(k=8), dict(n=-1), dict(x=None), dict(i=None), dict(s=None)):
        assert topk(**bad) == ARG, bad
        assert lib.mmc_last_error()
    for a in (idx, sc, proba, stats, votes):
        assert np.all(a == -7)
    assert topk(n=0, x=None, i=None, s=None) == _lib.MMC_OK
    y = np.zeros(6, np.int32)
    o = dict(est=np.full(6, -7, np.int32), score=np.full(6, -7, np.float32), rank=np.full(6, -7, np.int32), p_true=np.full(6, -7, np.float32),
             stats=np.full((6, 3), -7, np.float32), votes=np.full(6, -7, np.int32), totals=np.full(5, -7, np.int64),
             confusion=np.full((7, 7), -7, np.int64), rank_hist=np.full(7, -7, np.int64))

    def evaluate(e=ens.h, x=X.ctypes.data, yy=y, n=6, lmap=None, n_labels=0, totals=o["totals"].ctypes.data):
        outs = [o[q].ctypes.data for q in ("est", "score", "rank", "p_true", "stats", "votes")] + [totals, o["confusion"].ctypes.data, o["rank_hist"].ctypes.data]
        return lib.mmc_ensemble_evaluate(e, x, _ptr(yy), n, _ptr(lmap), n_labels, *outs, _lib.MMC_IN_HOST, None)
    bad_map = np.array([0, 7], np.int32)
    for bad in (dict(e=None), dict(n=-1), dict(totals=None), dict(x=None), dict(yy=None), dict(yy=np.full(6, 7, np.int32)), dict(n_labels=3),
                dict(lmap=bad_map, n_labels=2), dict(lmap=np.zeros(2, np.int32), n_labels=0)):
        assert evaluate(**bad) == ARG, bad
    for a in o.values():
        assert np.all(a == -7)
    ens.close()
